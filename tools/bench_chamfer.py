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
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from si_mamba_amd.mae import chamfer_distance  # noqa: E402

SHAPES = [(64, 1024, 1024), (64, 2048, 1024), (16, 8192, 8192)]
PEAK_LANE_OPS = 256 * 4 * 32 * 2.4e9
OPS_PER_PAIR = 9
TORCH_MAX_BYTES = 4 << 30           # of the (pairs, n, m, 3) fp32 difference tensor


def clouds(B, N, seed, dev):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(B, N, 3, generator=g)
    p = p - p.mean(1, keepdim=True)
    return (p / p.norm(dim=-1).max(dim=1)[0][:, None, None]).to(dev)


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def timeit(fn, target_ms=200.0, windows=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps = max(1, min(2000, int(target_ms / max(window_ms(fn, 3), 1e-3))))
    ts = sorted(window_ms(fn, reps) for _ in range(windows))
    return ts[len(ts) // 2], ts[0], ts[-1]


def torch_form(x, y):
    d = ((x[:, :, None] - y[:, None]) ** 2).sum(-1)
    return d.min(2)[0].mean(1) + d.min(1)[0].mean(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_chamfer.py needs a ROCm device: a time from anything else says nothing")
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
