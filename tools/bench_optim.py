"""The optimizer tail (csrc/optim.hip, si_mamba_amd/optim/) against torch's on one GPU.

(a) The tail alone on the parameter set of default_config()'s PointMamba (the classifier of bench.py), both captured in
    hipGraphs: ``clip_grad_norm_(foreach=True)`` + ``torch.optim.AdamW(fused=True, capturable=True).step()`` against
    ``si_mamba_amd.optim.AdamW.step(clip=10)``, on gradients as a backward leaves them (separate tensors) and, for the
    HIP tail, also on slices of one flat buffer (the data-parallel step: every alignment).  Device events around
    back-to-back replays, 5 windows per variant, the variants alternating (measure.alternate); kernel launches per tail
    counted by torch's profiler on one eager call after a first.
(b) The bf16 graphed training step (GraphedTrainStep, 64 clouds of 1024 points, clip 10) in clouds/s with either tail:
    fresh processes, ``--runs`` per variant, alternating (measure.fresh_processes).

    python tools/bench_optim.py [--runs 3] [--no-steps] [--out profiles/optim.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import measure  # noqa: E402

CLIP, LR, WD = 10.0, 5e-4, 0.05
BATCH, NPOINTS = 64, 1024


def _model(dev):
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    return PointMamba(default_config()).to(dev).train()


def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def _kernel_nodes(fn):
    """Kernel launches of one eager call of ``fn``, counted by torch's profiler; None where it is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()                                                  # the first call allocates the optimizer's state
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                   and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception as exc:                                  # a profiler without device support: the count is left out
        print(f"launch count not available: {exc}", file=sys.stderr)
        return None


def tails():
    from si_mamba_amd import _lib, optim
    from si_mamba_amd.dist import FlatGradients
    dev = torch.device("cuda:0")
    model = _model(dev)
    shapes = [p.shape for p in model.parameters()]
    n_elem = sum(p.numel() for p in model.parameters())
    gen = torch.Generator().manual_seed(1)
    init = [0.02 * torch.randn(s, generator=gen) for s in shapes]
    grads = [torch.randn(s, generator=gen) for s in shapes]
    del model

    def params_with_grads(flat=False):
        ps = [t.to(dev).requires_grad_(True) for t in init]
        for p, g in zip(ps, grads):
            p.grad = g.to(dev)
        keep = FlatGradients(ps) if flat else None
        return ps, keep

    def groups(ps):
        return [dict(params=[p for p in ps if p.dim() == 1], weight_decay=0.0),
                dict(params=[p for p in ps if p.dim() != 1], weight_decay=WD)]

    pt, _ = params_with_grads()
    ot = torch.optim.AdamW(groups(pt), lr=LR, fused=True, capturable=True)

    def torch_tail():
        torch.nn.utils.clip_grad_norm_(pt, CLIP, foreach=True)
        ot.step()

    ph, _ = params_with_grads()
    oh = optim.AdamW(groups(ph), lr=LR)
    pf, keep = params_with_grads(flat=True)
    of = optim.AdamW(groups(pf), lr=LR)
    pz, _ = params_with_grads()
    oz = optim.AdamW(groups(pz), lr=LR)
    fns = {"torch_clip_foreach_adamw_fused": torch_tail,
           "hip_tail": lambda: oh.step(clip=CLIP),
           "hip_tail_flat_gradients": lambda: of.step(clip=CLIP),
           "hip_tail_zero_grads": lambda: oz.step(clip=CLIP, zero_grads=True)}
    launches = {k: _kernel_nodes(fn) for k, fn in fns.items()}
    graphs = {k: _capture(fn) for k, fn in fns.items()}
    acc = measure.alternate({k: g.replay for k, g in graphs.items()}, target_ms=100.0, windows=5, reverse_odd=True)
    us = {k: measure.summary([1e3 * x for x in v], 2) for k, v in acc.items()}
    # p, g, m, v read and p, m, v written by the update, g read once more by the norm: 32 bytes per parameter
    upd_bytes, norm_bytes = 28 * n_elem, 4 * n_elem
    return dict(parameters=n_elem, tensors=len(shapes), chunk=_lib.OPTIM_CHUNK, kernel_launches=launches,
                us_per_tail=us, bytes_update=upd_bytes, bytes_norm=norm_bytes,
                hip_tail_tb_per_s=round((upd_bytes + norm_bytes) / (us["hip_tail"]["median"] * 1e-6) / 1e12, 3),
                floor_us_at_6p3_tb_per_s=round((upd_bytes + norm_bytes) / 6.3e12 * 1e6, 1))


def child(tail, steps, warmup):
    """One bf16 graphed training step series; prints a JSON line with clouds_per_s."""
    from si_mamba_amd import optim
    from si_mamba_amd.graphed import GraphedTrainStep
    from si_mamba_amd.synthetic import make_clouds
    dev = torch.device("cuda:0")
    model = _model(dev)
    pts = make_clouds(BATCH, NPOINTS, 1, dev)
    gt = torch.randint(0, 15, (BATCH,), generator=torch.Generator().manual_seed(2)).to(dev)
    if tail == "hip":
        opt = optim.AdamW(optim.reference_param_groups(model, WD), lr=LR)
    else:
        opt = torch.optim.AdamW(optim.reference_param_groups(model, WD), lr=LR, fused=True, capturable=True)

    def loss_fn(p, y):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return model.get_loss_acc(model(p), y)[0]

    step = GraphedTrainStep(loss_fn, opt, (pts, gt), clip=CLIP, warmup=3)
    ms = measure.host_clock(lambda: step(pts, gt), steps=steps, warmup=warmup)
    print(json.dumps(dict(tail=tail, ms_per_step=round(ms, 4), clouds_per_s=round(BATCH / ms * 1e3, 1))))


def steps(runs, n_steps, warmup):
    me = os.path.abspath(__file__)
    variants = [(f"{t}_tail", ROOT, [sys.executable, me, "--child", t, "--steps", str(n_steps), "--warmup", str(warmup)])
                for t in ("torch", "hip")]
    out = measure.fresh_processes(variants, runs, timeout_s=300, parse=lambda txt: measure.last_json_line(txt))
    return {name: dict(clouds_per_s=measure.summary([r["clouds_per_s"] for r in v], 1),
                       ms_per_step=measure.summary([r["ms_per_step"] for r in v], 3)) for name, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3, help="fresh processes per tail for (b)")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true", help="(a) only")
    ap.add_argument("--child", choices=["hip", "torch"], default=None)
    args = ap.parse_args()
    measure.require_gpu("bench_optim.py")
    if args.child:
        child(args.child, args.steps, args.warmup)
        return
    # the step processes first: this process has not opened the device yet, so they have the GPU to themselves
    step_res = None if args.no_steps else steps(args.runs, args.steps, args.warmup)
    line = json.dumps(dict(
        what="optimizer tail of the classifier (PointMamba default_config), fp32 parameters, one MI355X.  (a) the tail "
             "alone, captured in a hipGraph, us per replay: events around back-to-back replays, 5 windows of ~0.1 s per "
             "variant, the variants alternating; kernel launches counted by torch's profiler on one eager call.  (b) the "
             "bf16 graphed training step (64 clouds x 1024 points, clip 10) with either tail, fresh processes "
             "alternating, host clock between synchronises",
        device=torch.cuda.get_device_name(0), tail=tails(), graphed_bf16_step=step_res))
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
