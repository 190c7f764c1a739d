"""Part-segmentation scoring (csrc/part_metrics.hip, si_mamba_amd/seg_metrics.py) on one GPU: one evaluation pass of
180 batches of (16, 2048, 50) random fp32 scores -- ShapeNetPart's 2 874 test shapes at the reference's batch -- scored
two ways:

  device  PartSegMetrics.update per batch and one compute() at the end: no host read until then
  host    what the reference's evaluation loop does: the scores copied to the host, then the numpy restatement of the
          tests (tests/part_metrics_ref.py): restricted argmax, per-label counts, per-shape part IoUs

Both routes start from the same scores on the device (8 distinct batches, taken in turn) and end with the four averages
on the host; a round is timed with the host clock from the first batch to the result, the device idle before it.
5 rounds of each, the routes alternating; median, min and max.  ``kernel_us`` is the simamba_part_seg_eval kernel
alone (a pair of device events around each launch), ``part_seg_eval_call_us`` back-to-back part_seg_eval calls: what
is left of ``device`` per batch is the launch of the torch operations around the kernel (table lookups, the one-hot
sums, the state updates).

    python tools/bench_seg_eval.py [--batches 180] [--rounds 5] [--out profiles/seg_eval.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools import measure  # noqa: E402

B, N, C = 16, 2048, 50
DISTINCT = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=180)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_eval.json"))
    args = ap.parse_args()
    measure.require_gpu("bench_seg_eval.py")
    import part_metrics_ref as pr
    from si_mamba_amd import SHAPENETPART, PartSegMetrics, part_seg_eval
    dev = torch.device("cuda:0")
    table = pr.Table(SHAPENETPART.as_label_lists())
    g = torch.Generator().manual_seed(0)
    data = []
    for _ in range(DISTINCT):
        cat = torch.randint(0, len(SHAPENETPART), (B,), generator=g)
        first, count = torch.tensor(SHAPENETPART.first)[cat], torch.tensor(SHAPENETPART.count)[cat]
        target = first[:, None] + (torch.rand(B, N, generator=g) * count[:, None]).long()
        data.append((torch.randn(B, N, C, generator=g).to(dev), target.to(dev)))

    def timed_pass(acc, add, result):
        """ms from the first batch to the averages on the host (both routes end in a host read), and the averages"""
        res = []

        def one_pass():
            for i in range(args.batches):
                add(acc, *data[i % DISTINCT])
            res.append(result(acc))
        return measure.host_clock(one_pass, steps=1, warmup=0), res[0]

    def device_round():
        return timed_pass(PartSegMetrics(device=dev), lambda a, s, t: a.update(s, t), lambda a: a.compute())

    def host_round():
        return timed_pass(pr.Pass(table), lambda a, s, t: a.add(s.cpu().numpy(), t.cpu().numpy()), lambda a: a.result())

    device_round()                                    # warm-up: the table on the device, every kernel loaded
    ms = dict(device=[], host=[])
    for _ in range(args.rounds):
        t, got = device_round()
        ms["device"].append(t)
        t, want = host_round()
        ms["host"].append(t)
    same = all(abs(got[k] - want[k]) <= args.batches * B * 2.0 ** -52 * abs(want[k])
               for k in ("accuracy", "class_avg_accuracy", "class_avg_iou", "inctance_avg_iou"))

    scores, target = data[0]
    kernel = [measure.window(lambda: part_seg_eval(scores, target, return_pred=False), 200) * 1e3
              for _ in range(args.rounds)]

    from si_mamba_amd import _lib
    _lib.enable_kernel_timing(True, only=["part_seg_eval"])
    for _ in range(50):
        part_seg_eval(scores, target, return_pred=False)
    torch.cuda.synchronize()
    launches, kernel_ms = _lib.kernel_times()["part_seg_eval"]
    _lib.enable_kernel_timing(False)

    line = json.dumps(dict(
        what=f"one evaluation pass: {args.batches} batches of ({B}, {N}, {C}) random fp32 scores already on the device "
             f"-> the four averages on the host; host clock per pass, {args.rounds} rounds, the routes alternating: "
             "[median, min, max] ms.  part_seg_eval_call_us: back-to-back part_seg_eval calls (the kernel and the "
             "torch operations that prepare its arguments) between device events; kernel_us: the kernel alone, a pair "
             f"of events around each of {launches} launches, mean",
        kernel_us=round(kernel_ms * 1e3, 2),
        device=torch.cuda.get_device_name(0), batches=args.batches, pass_ms_device=measure.stats(ms["device"], 3),
        pass_ms_host=measure.stats(ms["host"], 3),
        per_batch_ms_device=round(measure.stats(ms["device"], 3)[0] / args.batches, 4),
        per_batch_ms_host=round(measure.stats(ms["host"], 3)[0] / args.batches, 4),
        part_seg_eval_call_us=measure.stats(kernel, 3),
        averages_agree=bool(same), averages=got and {k: got[k] for k in got if k != "category_iou"}))
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
