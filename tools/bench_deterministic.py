#!/usr/bin/env python3
"""Cost of the deterministic backward (SIMAMBA_BWD_DETERMINISTIC) against the atomic one, in one process, the two
modes alternated round by round.

    python tools/bench_deterministic.py [--rounds 5] [--reps 10] [--steps 8] [--out profiles/deterministic.json]

Per-call event times (_lib.enable_kernel_timing: the library call, i.e. the backward kernel plus, in the deterministic
mode, its sum pass; workspace allocation is outside the events):
  scan_seq_f32   selective_scan_fn backward, sequential kernel, (64, 768, 1024, 16) fp32, z / D / delta_bias
  scan_dt_bf16   the bf16 mixer's scan backward (delta formed in the kernel) + its conv1d backward, (64, 768, 1024)
  scan_row_f32   selective_scan_fn backward, row-scan kernel, (16, 768, 1024, 16) fp32
  conv_f32       causal_conv1d_fn backward (width 4, SiLU), (64, 768, 1024) fp32
PointMamba train step (B = 64, 1024 points, 12 blocks, AdamW, clip), fp32 and bf16 autocast, clouds/s for: the default
mode; torch.use_deterministic_algorithms(True) (which turns the library's mode on) with
torch.utils.deterministic.fill_uninitialized_memory on (torch's default) and off.
Every figure: median over rounds, with min and max.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from si_mamba_amd import _lib  # noqa: E402
from tools import measure  # noqa: E402


def scan_case(B, D, L, dtype, ckpt, dev):
    from si_mamba_amd import selective_scan_fn
    g = torch.Generator(device=dev).manual_seed(0)
    act = dict(device=dev, dtype=dtype)
    u, delta, z = (torch.randn(B, D, L, generator=g, **act).requires_grad_(True) for _ in range(3))
    Bm, Cm = (torch.randn(B, 16, L, generator=g, **act).requires_grad_(True) for _ in range(2))
    A = (-torch.rand(D, 16, generator=g, device=dev) - 0.5).requires_grad_(True)
    Dp, bias = (0.1 * torch.randn(D, generator=g, device=dev)).requires_grad_(True), \
        (0.1 * torch.randn(D, generator=g, device=dev)).requires_grad_(True)
    with _lib.scan_ckpt(ckpt):
        out = selective_scan_fn(u, delta, A, Bm, Cm, Dp, z, bias, delta_softplus=True)
    dout = torch.randn_like(out)
    ins = [u, delta, A, Bm, Cm, Dp, z, bias]
    return lambda: torch.autograd.grad(out, ins, dout, retain_graph=True)


def dt_case(dev):
    from si_mamba_amd.mamba_inner import mamba_inner_fn
    g = torch.Generator(device=dev).manual_seed(0)
    B, D, L, N, R = 64, 768, 1024, 16, 24
    xz = torch.randn(B, 2 * D, L, generator=g, device=dev).to(torch.bfloat16).requires_grad_(True)
    ps = [0.3 * torch.randn(D, 4, generator=g, device=dev), 0.1 * torch.randn(D, generator=g, device=dev),
          0.05 * torch.randn(R + 2 * N, D, generator=g, device=dev), 0.2 * torch.randn(D, R, generator=g, device=dev),
          -torch.rand(D, N, generator=g, device=dev) - 0.5, torch.randn(D, generator=g, device=dev),
          0.1 * torch.randn(D, generator=g, device=dev)]
    ps = [p.requires_grad_(True) for p in ps]
    y = mamba_inner_fn(xz, ps[0], ps[1], ps[2], ps[3], None, None, ps[4], ps[5], ps[6])
    dy = torch.randn_like(y)
    return lambda: torch.autograd.grad(y, [xz] + ps, dy, retain_graph=True)


def conv_case(dev):
    from si_mamba_amd import causal_conv1d_fn
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(64, 768, 1024, generator=g, device=dev).requires_grad_(True)
    w = (0.3 * torch.randn(768, 4, generator=g, device=dev)).requires_grad_(True)
    b = (0.1 * torch.randn(768, generator=g, device=dev)).requires_grad_(True)
    out = causal_conv1d_fn(x, w, b, "silu")
    dout = torch.randn_like(out)
    return lambda: torch.autograd.grad(out, [x, w, b], dout, retain_graph=True)


def time_calls(fn, reps, names):
    _lib.enable_kernel_timing(True, only=names)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    t = _lib.kernel_times()
    _lib.enable_kernel_timing(False)
    return {k: t[k][1] * 1e3 for k in names if k in t}            # us per call


def kernels(args, dev):
    cases = {"scan_seq_f32": (lambda: scan_case(64, 768, 1024, torch.float32, _lib.CKPT_SEQ, dev), ["scan_bwd"]),
             "scan_dt_bf16": (lambda: dt_case(dev), ["scan_bwd", "conv1d_bwd"]),
             "scan_row_f32": (lambda: scan_case(16, 768, 1024, torch.float32, _lib.CKPT_ROW, dev), ["scan_bwd"]),
             "conv_f32": (lambda: conv_case(dev), ["conv1d_bwd"])}
    res = {}
    for name, (make, calls) in cases.items():
        fn = make()
        for on in (False, True):                                   # warm-up, both modes
            with _lib.deterministic(on):
                fn()
        torch.cuda.synchronize()
        acc = {(m, c): [] for m in ("atomic", "deterministic") for c in calls}
        for _ in range(args.rounds):
            for on, m in ((False, "atomic"), (True, "deterministic")):
                with _lib.deterministic(on):
                    t = time_calls(fn, args.reps, calls)
                for c in calls:
                    acc[(m, c)].append(t[c])
        out = {}
        for c in calls:
            a, d = measure.summary(acc[("atomic", c)], 4), measure.summary(acc[("deterministic", c)], 4)
            out[c] = {"atomic_us": a, "deterministic_us": d, "ratio_median": round(d["median"] / a["median"], 4)}
        res[name] = out
        del fn
        torch.cuda.empty_cache()
        print(name, json.dumps(out), flush=True)
    return res


def train_steps(args, dev):
    import torch.utils.deterministic as tud
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    m = PointMamba(default_config()).to(dev).train()
    opt = torch.optim.AdamW(m.parameters(), lr=5e-4, weight_decay=0.05)
    g = torch.Generator().manual_seed(1)
    pts = torch.randn(64, 1024, 3, generator=g)
    pts = (pts / pts.norm(dim=-1).max(dim=1)[0][:, None, None]).to(dev)
    gt = torch.randint(0, 15, (64,), generator=g).to(dev)
    fill0 = tud.fill_uninitialized_memory

    def run(amp, steps):
        def step():
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                loss = m.get_loss_acc(m(pts), gt)[0]
            loss.backward()
            torch.nn.utils.clip_grad_norm_(m.parameters(), 10.0)
            opt.step()
        torch.cuda.synchronize()
        return 64 / (measure.window(step, steps) / 1e3)

    modes = [("default", False, True), ("torch_deterministic_fill_on", True, True),
             ("torch_deterministic_fill_off", True, False)]
    res = {}
    try:
        for amp in (False, True):
            acc = {k: [] for k, _, _ in modes}
            for k, det, fill in modes:                             # warm-up of every mode
                torch.use_deterministic_algorithms(det)
                tud.fill_uninitialized_memory = fill
                run(amp, 2)
            for _ in range(args.rounds):
                for k, det, fill in modes:
                    torch.use_deterministic_algorithms(det)
                    tud.fill_uninitialized_memory = fill
                    acc[k].append(run(amp, args.steps))
            key = "bf16" if amp else "fp32"
            res[key] = {k: measure.summary(v, 4) for k, v in acc.items()}
            base = res[key]["default"]["median"]
            for k in acc:
                res[key][k]["vs_default"] = round(res[key][k]["median"] / base, 4)
            print(key, json.dumps(res[key]), flush=True)
    finally:
        torch.use_deterministic_algorithms(False)
        tud.fill_uninitialized_memory = fill0
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    measure.require_gpu("bench_deterministic.py")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "reps": args.reps, "steps": args.steps,
           "unit_kernels": "us per library call", "unit_train": "clouds/s", "kernels": kernels(args, dev)}
    if not args.no_train:
        out["train_step"] = train_steps(args, dev)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
