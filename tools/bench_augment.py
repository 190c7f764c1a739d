"""Sampling + augmentation in front of a step (csrc/augment.hip, si_mamba_amd/transforms.py) on one GPU: B = 64 clouds of
N in {1024, 2048, 8192} points, rotate and scale-and-translate, three ways:

  fused         sample_and_augment(points, [transform]): one launch (and the one-lane step kernel), no host read
  gather_fused  the same with the runner's sampling in front, in the same launch: idx (B, M) farthest-point-style
                indices, M = the reference's point_all for N (1200, 2400, 8192), and sel = randperm(M)[:N] drawn on
                the device inside the timed call, as a training step draws it
  eager_loop    the shape of the reference's datasets/data_transforms.py, written anew: a Python loop over the batch
                that draws with numpy on the host, copies one small array per cloud to the device and applies it with
                torch operations, in place

Every route starts from points on the device and ends with the augmented batch on the device.  A round is `--calls`
calls between a device synchronise in front and one behind, timed with the host clock (so the number is what a training
loop waits for, enqueue included); rounds of the three routes alternate; median, min and max per call.  `kernel_us` is
the augmentation kernel alone, between a pair of device events around each launch.  `launches_per_call` and
`h2d_copies_per_call` are counted from the code, not measured.

    python tools/bench_augment.py [--calls 200] [--rounds 5] [--out profiles/augment.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import measure  # noqa: E402

B = 64
SIZES = {1024: 1200, 2048: 2400, 8192: 8192}         # N -> M (runner_finetune.py:191-203)


def eager_rotate(pc, rng):
    for i in range(pc.shape[0]):
        angle = rng.uniform() * 2 * np.pi
        c, s = np.cos(angle), np.sin(angle)
        rot = torch.from_numpy(np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float32)).to(pc.device)
        pc[i] = pc[i] @ rot
    return pc


def eager_scale_translate(pc, rng, lo=2. / 3., hi=3. / 2., tr=0.2):
    for i in range(pc.shape[0]):
        both = np.concatenate([rng.uniform(lo, hi, 3), rng.uniform(-tr, tr, 3)]).astype(np.float32)
        both = torch.from_numpy(both).to(pc.device)          # one copy per cloud (the reference makes two)
        pc[i] = pc[i] * both[:3] + both[3:]
    return pc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment.json"))
    ap.add_argument("--deviations", default=None,
                    help="JSON file with the deviations the GPU tests printed, copied into the result")
    args = ap.parse_args()
    measure.require_gpu("bench_augment.py")
    from si_mamba_amd import _lib, transforms as T
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    state = T.AugmentState(0, dev)
    ops = {"rotate": (T.PointcloudRotate(), eager_rotate),
           "scale_translate": (T.PointcloudScaleAndTranslate(), eager_scale_translate)}
    g = torch.Generator().manual_seed(0)

    rows = []
    for N, M in SIZES.items():
        raw = (torch.rand(B, M, 3, generator=g) * 2 - 1).to(dev)
        pts = raw[:, :N].contiguous()
        idx = torch.stack([torch.randperm(M, generator=g) for _ in range(B)]).to(dev).int()
        out = torch.empty(B, N, 3, device=dev)
        for name, (fused_t, eager_fn) in ops.items():
            routes = {
                "fused": lambda: T.sample_and_augment(pts, [fused_t], state=state, out=out),
                "gather_fused": lambda: T.sample_and_augment(
                    raw, [fused_t], idx=idx, sel=torch.randperm(M, device=dev)[:N], state=state, out=out),
                "eager_loop": lambda: eager_fn(pts, rng),
            }
            for fn in routes.values():                       # warm-up: every kernel loaded, the allocator settled
                for _ in range(3):
                    fn()
            us = measure.rounds({k: (lambda fn=fn: measure.host_clock(fn, steps=args.calls, warmup=0) * 1e3)
                                 for k, fn in routes.items()}, args.rounds)
            _lib.enable_kernel_timing(True, only=["augment_points"])
            for _ in range(50):
                routes["gather_fused"]()
            torch.cuda.synchronize()
            launches, kernel_ms = _lib.kernel_times()["augment_points"]
            _lib.enable_kernel_timing(False)
            rows.append(dict(N=N, M=M, op=name, fused_us=measure.stats(us["fused"], 2),
                             gather_fused_us=measure.stats(us["gather_fused"], 2),
                             eager_loop_us=measure.stats(us["eager_loop"], 2), kernel_us=round(kernel_ms * 1e3, 2)))
            print(json.dumps(rows[-1]), flush=True)

    deviations = None
    if args.deviations:
        with open(args.deviations) as fh:
            deviations = json.load(fh)
    line = json.dumps(dict(
        what=f"B = {B} clouds already on the device -> the augmented batch on the device; host clock over {args.calls} "
             f"calls between two device synchronises, {args.rounds} rounds, the routes alternating: [median, min, max] us "
             "per call.  fused: sample_and_augment, one op; gather_fused: the same with idx (B, M) and a randperm(M)[:N] "
             "drawn on the device inside the call; eager_loop: a per-cloud Python loop with numpy draws and one "
             "host-to-device copy per cloud.  kernel_us: the fused kernel and the step kernel behind it between a pair "
             "of device events around each of 50 gather_fused launches, mean.  deviations: the largest the GPU tests "
             "(tests/test_gpu_augment.py) observed, against their bounds",
        device=torch.cuda.get_device_name(0), batch=B, calls=args.calls, rounds=args.rounds,
        launches_per_call=dict(fused=2, gather_fused="2 + randperm and its slice", eager_loop=f"about {4 * B} (B = {B})"),
        h2d_copies_per_call=dict(fused=0, gather_fused=0, eager_loop=B), rows=rows, deviations=deviations))
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
