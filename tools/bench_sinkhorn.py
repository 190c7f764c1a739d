"""Sinkhorn divergence (csrc/sinkhorn.hip) on one GPU: call times at (64, 1024, 1024), the reconstruct() shape
(64, 2048, 1024) and the limit (1, 8192, 8192) at the defaults (eps_rel = 2^-6, 16 iterations: 22 steps), forward and
forward + backward, beside the same procedure composed from torch ops on the same GPU: what a user of the package
without the kernels would run (cost matrices stored once, one logsumexp over a (P, n, m) tensor per half-step, the
gradient from softmax and bmm).  Where the composed route does not fit the device, that is recorded instead.

Every time is a call time: device events around ``reps`` back-to-back calls (reps sized so that a window lasts about
0.2 s), 5 windows per operation taken in alternation over the operations, median and spread.  The composed route's
values are compared with the kernels' at every shape, so the two columns time the same computation.

``exp``: the exponentials the kernels evaluate per call, counted from the shapes (one per cost and one rescale per eight
costs, in every half-step of the three problems, in the marginal-error pass and in the gradient walks), and the rate that
implies: exp / call time, a whole-call figure that includes the launches and the tails of every half-step.

``--ratios`` adds, for every case of tests/test_gpu_sinkhorn.py, the error of the kernels against the float64 run of
tests/sinkhorn_ref.py over the error of its float32 run (gpu_error / ref_error): the figures the test margin is set by.

    python tools/bench_sinkhorn.py [--ratios] [--out profiles/sinkhorn.json]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import measure  # noqa: E402

SHAPES = [(64, 1024, 1024), (64, 2048, 1024), (1, 8192, 8192)]
EPS_REL, ITERS = 2.0 ** -6, 16


def inputs(pairs, n, m, dev):
    g = torch.Generator().manual_seed(n + m)
    x = torch.randn(pairs, n, 3, generator=g)
    y = 0.75 * torch.randn(pairs, m, 3, generator=g) + torch.tensor([0.5, -0.25, 0.125])
    return x.to(dev), y.to(dev)


def exp_count(pairs, n, m, steps, backward):
    per_cost = 1.0 + 1.0 / 8.0
    fwd = pairs * per_cost * (2 * steps * (n * m + n * n + m * m) + n * m)
    bwd = pairs * per_cost * ((n * m + n * n) + (n * m + m * m))
    return fwd + (bwd if backward else 0.0)


def composed(x, y, eps_rel, iters, grad):
    """The procedure of include/simamba.h in torch ops -> div, or (div, dx, dy) with the potentials held fixed."""
    pairs, n, m = x.shape[0], x.shape[1], y.shape[1]
    pts = torch.cat([x, y], 1)
    e = pts.amax(1) - pts.amin(1)
    d2 = (e * e).sum(-1).clamp_min(1e-30).view(pairs, 1, 1)
    steps = math.ceil(math.log2(1.0 / eps_rel))
    eps_list = [d2 * 2.0 ** -t for t in range(steps)] + [d2 * eps_rel] * iters

    def cost(a, b):
        return ((a[:, :, None, :] - b[:, None, :, :]) ** 2).sum(-1)

    def solve(c):
        nr, nc = c.shape[1], c.shape[2]
        ct = c.transpose(1, 2)
        f = torch.zeros(pairs, nr, device=x.device)
        g = torch.zeros(pairs, nc, device=x.device)
        for eps in eps_list:
            f = -eps[:, :, 0] * torch.logsumexp((g[:, None, :] - c) / eps - math.log(nc), 2)
            g = -eps[:, :, 0] * torch.logsumexp((f[:, None, :] - ct) / eps - math.log(nr), 2)
        return f, g

    cxy, cxx, cyy = cost(x, y), cost(x, x), cost(y, y)
    (f_xy, g_xy), (f_xx, g_xx), (f_yy, g_yy) = solve(cxy), solve(cxx), solve(cyy)
    ot = lambda f, g: f.mean(1) + g.mean(1)                                                 # noqa: E731
    div = ot(f_xy, g_xy) - 0.5 * ot(f_xx, g_xx) - 0.5 * ot(f_yy, g_yy)
    if not grad:
        return div
    eps = eps_list[-1]

    def mean_of(pot, c, cols):
        return torch.bmm(torch.softmax((pot[:, None, :] - c) / eps, 2), cols)

    dx = (2.0 / n) * (mean_of(g_xx, cxx, x) - mean_of(g_xy, cxy, y))
    dy = (2.0 / m) * (mean_of(f_yy, cyy, y) - mean_of(f_xy, cxy.transpose(1, 2), x))
    return div, dx, dy


def timings():
    from si_mamba_amd import sinkhorn_divergence
    from si_mamba_amd.sinkhorn import scaling_steps
    dev = torch.device("cuda:0")
    steps = scaling_steps(EPS_REL) + ITERS
    rows = []
    for pairs, n, m in SHAPES:
        x, y = inputs(pairs, n, m, dev)

        def fwd_bwd():
            xa, ya = x.detach().requires_grad_(), y.detach().requires_grad_()
            sinkhorn_divergence(xa, ya).sum().backward()
            return xa.grad, ya.grad

        ops = {"sinkhorn_fwd": lambda: sinkhorn_divergence(x, y), "sinkhorn_fwd_bwd": fwd_bwd}
        row = dict(shape=[pairs, n, m], eps_rel=EPS_REL, iters=ITERS, steps=steps)
        div, ot_xy, merr = sinkhorn_divergence(x, y, return_info=True)
        dx, dy = fwd_bwd()
        row.update(div_mean=float(div.mean()), merr_max=float(merr.max()))
        try:
            cdiv, cdx, cdy = composed(x, y, EPS_REL, ITERS, True)
            row["composed_vs_kernels_max_abs"] = dict(div=float((cdiv - div).abs().max()),
                                                      dx=float((cdx - dx).abs().max()),
                                                      dy=float((cdy - dy).abs().max()))
            del cdiv, cdx, cdy
            ops["composed_fwd"] = lambda: composed(x, y, EPS_REL, ITERS, False)
            ops["composed_fwd_bwd"] = lambda: composed(x, y, EPS_REL, ITERS, True)
            row["composed_tensor_mb"] = round(4.0 * pairs * n * m / 2 ** 20, 1)
        except torch.cuda.OutOfMemoryError as err:
            row["composed"] = f"does not fit: {str(err).splitlines()[0]}"
            torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        row["ms_median_min_max"] = ms = {k: measure.stats(v, 4) for k, v in measure.alternate(ops).items()}
        row["peak_mb_all_ops"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
        row["exp"] = {}
        for name, back in (("sinkhorn_fwd", False), ("sinkhorn_fwd_bwd", True)):
            cnt = exp_count(pairs, n, m, steps, back)
            row["exp"][name] = dict(count=cnt, per_s=round(cnt / (ms[name][0] * 1e-3), 0))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return rows


def ratios():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sinkhorn_ref as sr
    from si_mamba_amd import sinkhorn_divergence
    dev = torch.device("cuda:0")
    out = []
    cases = [s + st for s in sr.SIZES for st in sr.SETTINGS] + [sr.LIMIT_CASE]
    for case in cases:
        x, y, _, r64 = sr.reference(*case)
        err = sr.ref_error(case)
        xd, yd = x.to(dev).requires_grad_(), y.to(dev).requires_grad_()
        div, ot_xy, _ = sinkhorn_divergence(xd, yd, eps_rel=case[3], iters=case[4], return_info=True)
        div.sum().backward()
        got = dict(div=div, ot_xy=ot_xy, dx=xd.grad, dy=yd.grad)
        row = dict(case=list(case))
        for k, v in got.items():
            e = float((v.detach().cpu().double() - r64[k]).abs().max())
            row[k] = dict(gpu_error=e, ref_error=err[k], ratio=round(e / err[k], 3) if err[k] else None)
        out.append(row)
    worst = max(r[k]["ratio"] for r in out for k in ("div", "ot_xy", "dx", "dy") if r[k]["ratio"] is not None)
    return dict(cases=out, worst_ratio=worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ratios", action="store_true", help="gpu_error / ref_error for every case of the GPU tests")
    args = ap.parse_args()
    measure.require_gpu("bench_sinkhorn.py")
    res = dict(what="sinkhorn_divergence (fp32, gaussian sets, defaults: eps_rel 2^-6, 16 iterations, 22 steps) and the "
                    "same procedure composed from torch ops, one MI355X; call times (events around back-to-back calls, "
                    "5 windows of ~0.2 s per operation, the operations alternating): [median, min, max] ms; exp: "
                    "exponentials per call counted from the shapes and count / median call time",
               device=torch.cuda.get_device_name(0), timings=timings())
    if args.ratios:
        res["error_ratios"] = ratios()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
