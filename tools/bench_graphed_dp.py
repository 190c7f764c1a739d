"""The graphed data-parallel step against the single-process graph and against eager DDP, on the two
launch-bound workloads: part segmentation (B = 16, 2048 points, bf16, HLT) and MAE pre-training (B = 64, bf16).

    python tools/bench_graphed_dp.py --parent <built checkout of the parent commit> --out profiles/graphed_dp.json

  (a) `--graph` of the parent checkout's tool, single process     (b) `--graph --dp`     (c) `--dp` (eager, wrap_ddp)

(b) and (c) at world size 1 (a one-rank RCCL group).  Every figure is a fresh process; the variants alternate, three
rounds; ms per step of 60 timed steps, median [min, max].  This driver never opens the GPU itself and stops at the
first process that fails."""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import measure

ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True)
ap.add_argument("--out", required=True)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=60)
args = ap.parse_args()
WORK = {"part_segmentation": ("bench_seg.py", ["--batch", "16", "--npoints", "2048", "--dtype", "bf16", "--method", "HLT"]),
        "mae_pretrain": ("bench_mae.py", ["--batch", "64", "--dtype", "bf16"])}
VARIANTS = [("a_parent_graph", os.path.abspath(args.parent), ["--graph"]), ("b_graph_dp", ROOT, ["--graph", "--dp"]),
            ("c_eager_dp", ROOT, ["--dp"])]
runs = measure.fresh_processes(
    [(f"{w} {v}", root, [sys.executable, os.path.join(root, "tools", tool)] + base + flags + ["--steps", str(args.steps)])
     for w, (tool, base) in WORK.items() for v, root, flags in VARIANTS], args.rounds, timeout_s=200,
    parse=lambda txt: measure.last_json_line(txt)["ms_per_step"])
ms = {w: {v: runs[f"{w} {v}"] for v, _, _ in VARIANTS} for w in WORK}
for rnd in range(args.rounds):
    for w, vs in ms.items():
        for v, x in vs.items():
            print(rnd, w, v, x[rnd], flush=True)
res = {"what": __doc__, "world_size": 1, "steps_per_run": args.steps, "ms_per_step": ms, "median_min_max": {
    w: {v: [measure.median(x), min(x), max(x)] for v, x in vs.items()} for w, vs in ms.items()}}
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res["median_min_max"]))
