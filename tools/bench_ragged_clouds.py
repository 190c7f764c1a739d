#!/usr/bin/env python3
"""Ragged point-cloud batches (per-cloud lengths in farthest-point sampling and the k-NN grouping): what they cost and
what they save, in one process, the variants of a comparison alternated round by round.

    python tools/bench_ragged_clouds.py [--parent-lib PATH] [--rounds 5] [--reps 20] [--out profiles/ragged_clouds.json]

``--parent-lib``: a libsimamba_hip.so built from the commit before the ragged kernels (it only needs the two plain
entry points).  Without it the "parent" columns are left out and the single-cloud calls go through this build's
plain entry points.

Shapes (B, N, patches / group size): (64, 1024, 128 / 32) and (64, 8192, 512 / 32).  Per shape:
  fixed     the plain entry points (no lengths), parent build against this build: is the fixed-length path unchanged?
            (with the parent build timed a second time in every round as a control: what the same code does to itself)
  ragged    ONE call on 64 clouds padded to N, lengths uniform in [N/2, N], against 64 single-cloud calls of the
            fixed-length kernels at the true lengths, enqueued back to back (what a ragged batch costs without lengths)
  full      the ragged kernels at lengths == N against the fixed-length kernels (the price of the length handling)
Times: device events around ``reps`` calls enqueued back to back, per call, in microseconds; median [min, max] over
the rounds.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from si_mamba_amd import _lib  # noqa: E402
from tools import measure  # noqa: E402

SHAPES = [(64, 1024, 128, 32), (64, 8192, 512, 32)]
PLAIN = ("simamba_farthest_point_sample", "simamba_knn_group")


def load_plain(path):
    lib = ctypes.CDLL(path)
    for name in PLAIN:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def compare(variants, rounds, reps, stream):
    """variants: name -> callable; every variant warmed up, then ``rounds`` rounds that run them in turn, in the
    opposite order every other round; us per call."""
    acc = measure.alternate(variants, windows=rounds, reps=reps, warmup=2, reverse_odd=True,
                            window=lambda fn, n: measure.window(fn, n, stream) * 1e3)
    return {k: measure.summary(v, 2) for k, v in acc.items()}


def checked(rc):
    if rc != 0:
        raise RuntimeError(f"library call failed: {rc}")


def bench_shape(new, parent, B, N, G, M, args, dev):
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    g = torch.Generator().manual_seed(N)
    pts = torch.randn(B, N, 3, generator=g)
    pts = (pts / pts.norm(dim=-1).max(dim=1)[0][:, None, None]).to(dev)
    lens_cpu = torch.randint(N // 2, N + 1, (B,), generator=g)
    lens, full = lens_cpu.to(dev), torch.full((B,), N, device=dev)
    idx = torch.empty(B, G, dtype=torch.int64, device=dev)
    cen = torch.empty(B, G, 3, device=dev)
    nn_idx = torch.empty(B, G, M, dtype=torch.int64, device=dev)
    p, i, c, k = pts.data_ptr(), idx.data_ptr(), cen.data_ptr(), nn_idx.data_ptr()

    def fps_plain(lib):
        return lambda: checked(lib.simamba_farthest_point_sample(p, i, c, B, N, G, sp))

    def knn_plain(lib):
        return lambda: checked(lib.simamba_knn_group(p, c, k, B, N, G, M, sp))

    def fps_ragged(ln):
        return lambda: checked(new.simamba_farthest_point_sample_ex(p, ln.data_ptr(), None, i, c, B, N, G, sp))

    def knn_ragged(ln):
        return lambda: checked(new.simamba_knn_group_ex(p, c, ln.data_ptr(), None, k, B, N, G, M, sp))

    # one cloud per call at its true length: cloud b's real points are the first lens[b] rows of its padded slot
    single = parent or new
    per = [(p + b * N * 12, i + b * G * 8, c + b * G * 12, k + b * G * M * 8, int(n)) for b, n in
           enumerate(lens_cpu.tolist())]

    def fps_single():
        for pb, ib, cb, _, n in per:
            checked(single.simamba_farthest_point_sample(pb, ib, cb, 1, n, G, sp))

    def knn_single():
        for pb, _, cb, kb, n in per:
            checked(single.simamba_knn_group(pb, cb, kb, 1, n, G, M, sp))

    out = {"lengths": {"min": int(lens_cpu.min()), "max": int(lens_cpu.max()), "mean": float(lens_cpu.float().mean())}}
    fps_plain(new)()                                     # centres for the k-NN calls below
    torch.cuda.synchronize()
    for op, plain, ragged, one in (("fps", fps_plain, fps_ragged, fps_single), ("knn_group", knn_plain, knn_ragged,
                                                                                knn_single)):
        res = {}
        if parent is not None:
            # "parent_again": the parent build a second time per round, the spread of one instruction stream
            r = compare({"parent": plain(parent), "this": plain(new), "parent_again": plain(parent)}, args.rounds,
                        args.reps, stream)
            r["this_median_inside_parent_range"] = r["parent"]["min"] <= r["this"]["median"] <= r["parent"]["max"]
            r["parent_again_median_inside_parent_range"] = \
                r["parent"]["min"] <= r["parent_again"]["median"] <= r["parent"]["max"]
            res["fixed_us"] = r
        r = compare({"ragged_one_call": ragged(lens), "single_cloud_calls": one}, args.rounds, args.reps, stream)
        r["speedup_median"] = round(r["single_cloud_calls"]["median"] / r["ragged_one_call"]["median"], 2)
        r["single_cloud_calls_from"] = "parent build" if parent is not None else "this build"
        res["ragged_us"] = r
        r = compare({"fixed": plain(new), "ragged_full_length": ragged(full)}, args.rounds, args.reps, stream)
        r["ratio_median"] = round(r["ragged_full_length"]["median"] / r["fixed"]["median"], 4)
        res["full_length_us"] = r
        out[op] = res
        print(f"({B}, {N}, {G}/{M}) {op}", json.dumps(res), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    measure.require_gpu("bench_ragged_clouds.py")
    dev = torch.device("cuda:0")
    new = _lib.load()
    parent = load_plain(args.parent_lib) if args.parent_lib else None
    out = {"device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "reps": args.reps,
           "unit": "us per call (device events around reps calls)", "parent_lib": bool(parent), "shapes": {}}
    with torch.cuda.device(dev):
        for B, N, G, M in SHAPES:
            out["shapes"][f"{B}x{N}_{G}x{M}"] = bench_shape(new, parent, B, N, G, M, args, dev)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
