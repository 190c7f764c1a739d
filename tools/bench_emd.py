"""Earth mover's distance (csrc/emd.hip) on one GPU: call times and round counts at the pre-training loss shape
(39 424 pairs of 32 points: 64 clouds x 616 masked tokens) and at (64 pairs, 1024 points), the one-wave Chamfer kernel at
the first shape for scale, and the MAE pre-training step (tools/bench_mae.py) with ``loss: cdl2`` and ``loss: emd``.

Every kernel time is a call time: device events around ``reps`` back-to-back calls (reps sized so that a window lasts
about 0.2 s), 5 windows per operation taken in alternation over the operations, median and spread.  The step times are
those of fresh tools/bench_mae.py processes, ``--runs`` per variant, the variants alternating so that they see the same
machine in the same minutes.  ``--parent DIR`` (a built checkout of the parent commit) adds that tree's cdl2 step to the
alternation: no code on the cdl2 path changes, so the two must agree within their own spread.

    python tools/bench_emd.py [--parent DIR] [--runs 3] [--out profiles/emd.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import measure  # noqa: E402

SHAPES = [(39424, 32), (64, 1024)]


def kernels():
    from si_mamba_amd import earth_movers_distance
    from si_mamba_amd.emd import default_max_rounds
    from si_mamba_amd.mae import chamfer_distance
    dev = torch.device("cuda:0")
    rows = []
    for pairs, n in SHAPES:
        g = torch.Generator().manual_seed(n)
        x, y = torch.randn(pairs, n, 3, generator=g).to(dev), torch.randn(pairs, n, 3, generator=g).to(dev)
        w = torch.rand(pairs, device=dev)

        def fwd_bwd(f):
            xa = x.detach().requires_grad_()
            (f(xa, y) * w).sum().backward()

        ops = {"emd_fwd": lambda: earth_movers_distance(x, y), "emd_fwd_bwd": lambda: fwd_bwd(earth_movers_distance)}
        if n <= 64:
            ops["chamfer_patch_fwd"] = lambda: chamfer_distance(x, y)
            ops["chamfer_patch_fwd_bwd"] = lambda: fwd_bwd(chamfer_distance)
        row = dict(shape=[pairs, n], ms_median_min_max={k: measure.stats(v, 4) for k, v in measure.alternate(ops).items()})
        dist, assign, rounds, conv = earth_movers_distance(x, y, return_assignment=True)
        row.update(rounds_mean=round(float(rounds.float().mean()), 1), rounds_max=int(rounds.max()),
                   max_rounds=default_max_rounds(n), converged_share=float(conv.float().mean()))
        rows.append(row)
    return rows


def steps(parent, runs):
    variants = [("this_cdl2", ROOT, ["--loss", "cdl2"]), ("this_emd", ROOT, ["--loss", "emd"])]
    if parent:
        variants.insert(0, ("parent_cdl2", os.path.abspath(parent), []))
    out = measure.fresh_processes(
        [(name, tree, [sys.executable, os.path.join(tree, "tools", "bench_mae.py")] + extra)
         for name, tree, extra in variants], runs, timeout_s=600,
        parse=lambda txt: measure.last_json_line(txt)["ms_per_step"])
    res = {name: dict(median=measure.median(v), runs=v) for name, v in out.items()}
    if not parent:
        res["parent_cdl2"] = "not measured (no --parent)"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--runs", type=int, default=3, help="bench_mae.py processes per variant")
    ap.add_argument("--no-steps", action="store_true", help="kernel times only")
    args = ap.parse_args()
    measure.require_gpu("bench_emd.py")
    # the step processes first: this process has not opened the device yet, so they have the GPU to themselves
    step_ms = None if args.no_steps else steps(args.parent, args.runs)
    line = json.dumps(dict(what="earth_movers_distance and the one-wave chamfer_distance, fp32, gaussian clouds, one "
                                "MI355X; call times (events around back-to-back calls, 5 windows of ~0.2 s per "
                                "operation, the operations alternating): [median, min, max] ms; MAE step (B = 64, bf16, "
                                "fwd + bwd + AdamW) per fresh process, variants alternating",
                           device=torch.cuda.get_device_name(0), kernels=kernels(), mae_step_ms=step_ms))
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
