"""Whole-cloud Chamfer distance (csrc/chamfer_large.hip) on one GPU: forward and forward + backward (both gradients) of
mae.chamfer_distance at three shapes, against the composed torch form on the device where its (pairs, n, m, 3)
intermediate fits, and against the kernels' own VALU count.

Every time is a call time: device events around `reps` back-to-back calls (reps sized so that a window lasts about
0.2 s), median of 5 windows after a warm-up, so launches and the small reduction kernel are inside it.  The VALU model
is 9 lane-operations per point pair and direction (3 subtractions, a multiply, 2 fused multiply-adds, a compare, 2
selects; the one v_mov of the index per target, shared by a thread's queries, is left out); the peak is 256 CUs x 4
SIMDs x 32 lanes x 2.4 GHz = 78.6e12 lane-operations / s.  `fwd_call_rate_over_valu_peak` divides the model's
operations by the CALL time (four allocations, two launches and the reduction kernel included): a lower bound of the
kernel's own share of peak, not that share; the kernel time is what a rocprofv3 --kernel-trace --stats run reports.

    python tools/bench_chamfer.py [--out profiles/chamfer_large.json]
prints one JSON line and, with --out, writes it there.

    python tools/bench_chamfer.py --ragged [--parent DIR] [--runs 5] [--out profiles/chamfer_ragged.json]
times, at the same three shapes, the plain call, the ragged call (x_lengths / y_lengths) at full lengths and the ragged
call with lengths spread over [n/2, n] and [m/2, m], next to the share of the n * m point pairs that remains.  DIR is a
built checkout of the parent commit: its plain call is timed too, `runs` times in alternation with this tree, every
run a fresh process, so that the two trees see the same machine in the same minutes.  Without --parent that
comparison is reported as not measured.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--child" in sys.argv:                        # a timing process of --ragged: the tree whose package it imports
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--child") + 1])
sys.path.insert(0, ROOT)
from si_mamba_amd.mae import chamfer_distance  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # measure: always this tree's
from tools import measure  # noqa: E402

SHAPES = [(64, 1024, 1024), (64, 2048, 1024), (16, 8192, 8192)]
PEAK_LANE_OPS = 256 * 4 * 32 * 2.4e9
OPS_PER_PAIR = 9
TORCH_MAX_BYTES = 4 << 30           # of the (pairs, n, m, 3) fp32 difference tensor


def clouds(B, N, seed, dev):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(B, N, 3, generator=g)
    p = p - p.mean(1, keepdim=True)
    return (p / p.norm(dim=-1).max(dim=1)[0][:, None, None]).to(dev)


def timeit(fn):
    """(median, min, max) ms per call over 5 windows of about 0.2 s, after a warm-up of 3 calls."""
    ts = measure.alternate({"op": fn}, target_ms=200.0, windows=5, warmup=3)["op"]
    return measure.median(ts), min(ts), max(ts)


def torch_form(x, y):
    d = ((x[:, :, None] - y[:, None]) ** 2).sum(-1)
    return d.min(2)[0].mean(1) + d.min(1)[0].mean(1)


def half_to_full(size, pairs, seed):
    """`pairs` lengths spread evenly over [size / 2, size], both ends included, in a fixed shuffled order."""
    ln = torch.linspace(size / 2, size, pairs).round().long()
    return ln[torch.randperm(pairs, generator=torch.Generator().manual_seed(seed))]


def ragged_child():
    """One process of --ragged: the plain call of the tree it imported and, where that tree has them, the ragged calls.
    Prints one JSON line."""
    import inspect
    dev = torch.device("cuda:0")
    has_lengths = "x_lengths" in inspect.signature(chamfer_distance).parameters
    rows = []
    for pairs, n, m in SHAPES:
        x, y = clouds(pairs, n, 1, dev), clouds(pairs, m, 2, dev)
        w = torch.rand(pairs, device=dev)
        modes = {"plain": {}}
        if has_lengths:
            nx, ny = half_to_full(n, pairs, 3), half_to_full(m, pairs, 4)
            modes["ragged_full"] = dict(x_lengths=torch.full((pairs,), n, device=dev),
                                        y_lengths=torch.full((pairs,), m, device=dev))
            modes["ragged_half_to_full"] = dict(x_lengths=nx.to(dev), y_lengths=ny.to(dev))
        row = dict(shape=[pairs, n, m])
        for name, kw in modes.items():
            def fwd_bwd():
                xa, ya = x.detach().requires_grad_(), y.detach().requires_grad_()
                (chamfer_distance(xa, ya, **kw) * w).sum().backward()

            row[name + "_fwd_ms"] = round(timeit(lambda: chamfer_distance(x, y, **kw))[0], 4)
            row[name + "_fwd_bwd_ms"] = round(timeit(fwd_bwd)[0], 4)
        if has_lengths:
            row["half_to_full_share_of_point_pairs"] = round(float((nx * ny).sum()) / (pairs * n * m), 4)
            same = torch.equal(chamfer_distance(x, y), chamfer_distance(x, y, **modes["ragged_full"]))
            row["ragged_full_equals_plain_bitwise"] = bool(same)
        rows.append(row)
    print(json.dumps(dict(tree=ROOT, device=torch.cuda.get_device_name(0), rows=rows)))


def ragged_main(args):
    """Alternate fresh timing processes of the parent tree and of this one; one JSON line of medians and every run."""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    trees = ([("parent", os.path.abspath(args.parent))] if args.parent else []) + [("this", here)]
    runs = measure.fresh_processes([(name, None, [sys.executable, os.path.abspath(__file__), "--child", tree])
                                    for name, tree in trees], args.runs, timeout_s=600)
    rows = []
    for i, shape in enumerate(SHAPES):
        row = dict(shape=list(shape))
        for name in runs:
            for key in runs[name][0]["rows"][i]:
                if key.endswith("_ms"):
                    vals = [r["rows"][i][key] for r in runs[name]]
                    row[f"{name}_{key}"] = dict(median=measure.median(vals), runs=vals)
                elif key != "shape":
                    row[key] = runs[name][-1]["rows"][i][key]
        for k in ("fwd_ms", "fwd_bwd_ms"):
            plain = row[f"this_plain_{k}"]["median"]
            if args.parent:
                row[f"a_plain_over_parent_{k}"] = round(plain / row[f"parent_plain_{k}"]["median"], 4)
            else:
                row[f"a_plain_over_parent_{k}"] = "not measured (no --parent)"
            row[f"b_ragged_full_over_plain_{k}"] = round(row[f"this_ragged_full_{k}"]["median"] / plain, 4)
            row[f"c_ragged_half_to_full_over_plain_{k}"] = round(row[f"this_ragged_half_to_full_{k}"]["median"] / plain,
                                                                 4)
        rows.append(row)
    line = json.dumps(dict(what="chamfer_distance, plain and ragged calls, fp32, one MI355X; call times (events around "
                                "back-to-back calls, median of 5 windows of ~0.2 s) per process, then the median over "
                                f"{args.runs} processes per tree, parent and this tree alternating",
                           device=runs["this"][0]["device"], parent_measured=bool(args.parent), rows=rows))
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (with --ragged)")
    ap.add_argument("--runs", type=int, default=5, help="timing processes per tree (with --ragged)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.ragged and not args.child:
        return ragged_main(args)                 # starts the timing processes; opens no device itself
    measure.require_gpu("bench_chamfer.py")
    if args.child:
        return ragged_child()
    dev = torch.device("cuda:0")
    rows = []
    for pairs, n, m in SHAPES:
        x, y = clouds(pairs, n, 1, dev), clouds(pairs, m, 2, dev)
        w = torch.rand(pairs, device=dev)

        def fwd_bwd(f=chamfer_distance):
            xa, ya = x.detach().requires_grad_(), y.detach().requires_grad_()
            (f(xa, ya) * w).sum().backward()

        lane_ops = 2 * pairs * n * m * OPS_PER_PAIR
        t_f = timeit(lambda: chamfer_distance(x, y))
        t_fb = timeit(fwd_bwd)
        row = dict(shape=[pairs, n, m], fwd_ms=round(t_f[0], 4), fwd_ms_min_max=[round(t_f[1], 4), round(t_f[2], 4)],
                   fwd_bwd_ms=round(t_fb[0], 4), fwd_bwd_ms_min_max=[round(t_fb[1], 4), round(t_fb[2], 4)],
                   fwd_lane_ops=lane_ops,
                   fwd_call_rate_over_valu_peak=round(lane_ops / (t_f[0] * 1e-3) / PEAK_LANE_OPS, 4))
        if pairs * n * m * 3 * 4 <= TORCH_MAX_BYTES:
            err = float(((chamfer_distance(x, y) - torch_form(x, y)).abs() / torch_form(x, y)).max())
            row.update(torch_fwd_ms=round(timeit(lambda: torch_form(x, y))[0], 4),
                       torch_fwd_bwd_ms=round(timeit(lambda: fwd_bwd(torch_form))[0], 4), rel_diff_vs_torch=err)
        else:
            row.update(torch_fwd_ms=None, torch_fwd_bwd_ms=None,
                       note="composed torch form not run: its difference tensor exceeds 4 GiB")
        rows.append(row)
    line = json.dumps(dict(what="chamfer_distance, whole clouds, fp32, one MI355X; call times (events around "
                                "back-to-back calls, median of 5 windows of ~0.2 s)",
                           device=torch.cuda.get_device_name(0), valu_model="9 lane-ops per point pair and direction",
                           peak_lane_ops_per_s=PEAK_LANE_OPS, rows=rows))
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
