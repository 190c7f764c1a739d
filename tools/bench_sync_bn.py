"""Patch encoder forward + backward with nn.SyncBatchNorm (--sync_bn) at the model shape: which route its two
BatchNorm+ReLU layers take.

  module   nn.SyncBatchNorm called as a module behind a materialised x + gterm.repeat_interleave(n): the route
           bn_relu_fn gave every module that was not nn.BatchNorm1d before the kernels had stages
  sync     encoder_ops.sync_bn_relu_fn: the staged HIP kernels with one all-gather forward and one all-reduce
           backward per layer, here in a process group of ONE rank (the collectives run, over one rank)
  local    plain nn.BatchNorm1d on the fused kernels (bn_relu_fn): what the sync route costs on top is two small
           collectives and the extra launches

Times are medians over --iters forward + backward passes per route, the routes taken in turn inside every iteration,
device-synchronised on both sides; peak memory is torch's allocator peak over one forward + backward.

    python tools/bench_sync_bn.py --out profiles/sync_bn.json
"""
import argparse
import json
import os
import sys
import tempfile

import torch
import torch.distributed as dist
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from si_mamba_amd import encoder_ops, point_mamba  # noqa: E402
from si_mamba_amd.point_mamba import Encoder  # noqa: E402
from tools import measure  # noqa: E402


def module_route(x, bn, gterm=None, group=0):
    if gterm is not None:
        x = x + gterm.to(x.dtype).repeat_interleave(group, dim=0)
    return torch.relu(bn(x))


ROUTES = {"module": (True, module_route), "sync": (True, encoder_ops.sync_bn_relu_fn),
          "local": (False, encoder_ops.bn_relu_fn)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--groups", type=int, default=128)
    ap.add_argument("--points", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    measure.require_gpu("bench_sync_bn.py")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    store = tempfile.mkdtemp()
    dist.init_process_group("nccl", init_method=f"file://{store}/store", rank=0, world_size=1)
    result = dict(shape=dict(batch=args.batch, groups=args.groups, points=args.points, encoder_channel=384),
                  iters=args.iters, warmup=args.warmup, world_size=1, device=torch.cuda.get_device_name(dev))
    try:
        torch.manual_seed(0)
        pts = torch.randn(args.batch, args.groups, args.points, 3, device=dev)
        dy = torch.randn(args.batch, args.groups, 384, device=dev)
        base = Encoder(384).to(dev).train()
        encs = {}
        for name, (convert, _) in ROUTES.items():
            e = Encoder(384).to(dev).train()
            e.load_state_dict(base.state_dict())
            encs[name] = nn.SyncBatchNorm.convert_sync_batchnorm(e) if convert else e

        def step(name, autocast):
            point_mamba.bn_relu_fn = ROUTES[name][1]
            p = pts.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                y = encs[name](p)
            y.backward(dy.to(y.dtype))
            return y

        for label, autocast in (("fp32", False), ("bf16_autocast", True)):
            times = {k: [] for k in ROUTES}
            peaks, outs = {}, {}
            for it in range(args.warmup + args.iters):
                for name in ROUTES:
                    for p in encs[name].parameters():
                        p.grad = None
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats(dev)
                    before = torch.cuda.memory_allocated(dev)
                    y = []
                    ms = measure.host_clock(lambda: y.append(step(name, autocast)), steps=1, warmup=0)
                    if it >= args.warmup:
                        times[name].append(ms)
                    peaks[name] = (torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20
                    outs[name] = y.pop().detach().float()
            ref = outs["local"]
            result[label] = {
                name: dict(ms_median=round(measure.median(times[name]), 3), ms_min=round(min(times[name]), 3),
                           ms_max=round(max(times[name]), 3), peak_mib_above_start=round(peaks[name], 1),
                           max_abs_diff_vs_local=float((outs[name] - ref).abs().max()))
                for name in ROUTES}
            result[label]["sync_over_module_time"] = round(
                result[label]["sync"]["ms_median"] / result[label]["module"]["ms_median"], 3)
            result[label]["sync_over_local_time"] = round(
                result[label]["sync"]["ms_median"] / result[label]["local"]["ms_median"], 3)
    finally:
        point_mamba.bn_relu_fn = encoder_ops.bn_relu_fn
        dist.destroy_process_group()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
