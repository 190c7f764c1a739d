"""RMSNorm (SIMAMBA_NORM_RMS) against LayerNorm on the same kernels, one MI355X:
  * add + norm forward and backward (csrc/add_norm.hip) at (64, 1024, 384), fp32 and bf16 I/O;
  * the fused out_proj + add + norm kernel (csrc/out_norm_bf16.hip) at (64, 768 -> 384, 1024);
  * the bf16-autocast PointMamba train step (bench.py's step: B = 64, 1024 points, 12 blocks, AdamW) with
    rms_norm=True against False.
Kernel calls are timed with device events over 50 launches after a warm-up, train steps over 10 steps after 3; every
measurement alternates the two modes for 5 rounds and reports the median [min, max].  One JSON document on stdout
(and to --out)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from si_mamba_amd import _lib  # noqa: E402
from tools import measure  # noqa: E402

ROUNDS = 5


def events_us(fn):
    return measure.calls(fn, warmup=5, reps=50) * 1e3


def ab(fns):
    """{name: fn} -> {name: [median, min, max]} over ROUNDS alternating rounds"""
    return {k: measure.stats(v, 2) for k, v in measure.rounds(fns, ROUNDS).items()}


def add_norm_calls(dev, dtype, B=64, L=1024, d=384):
    lib = _lib.load()
    code = _lib.dtype_code(dtype)
    g = torch.Generator(device=dev).manual_seed(0)
    h = torch.randn(B, L, d, device=dev, generator=g).to(dtype)
    r = torch.randn(B, L, d, device=dev, generator=g)
    w, b = torch.ones(d, device=dev), torch.zeros(d, device=dev)
    ro, nm = torch.empty(B, L, d, device=dev), torch.empty(B, L, d, device=dev, dtype=dtype)
    mean, rstd = torch.empty(B * L, device=dev), torch.empty(B * L, device=dev)
    dn = torch.randn(B, L, d, device=dev, generator=g).to(dtype)
    dro = torch.randn(B, L, d, device=dev, generator=g)
    dres, dhid = torch.empty(B, L, d, device=dev), torch.empty(B, L, d, device=dev, dtype=dtype)
    part = torch.empty(lib.simamba_add_layer_norm_grid(B, L), 2, d, device=dev)
    st = _lib.stream_ptr(dev)

    def fwd(flags):
        rc = lib.simamba_add_layer_norm_fwd_ex(h.data_ptr(), r.data_ptr(), None, w.data_ptr(),
                                               None if flags else b.data_ptr(), ro.data_ptr(), nm.data_ptr(),
                                               None if flags else mean.data_ptr(), rstd.data_ptr(), B, L, d, 1e-5,
                                               code, code, flags, st)
        assert rc == 0, rc

    def bwd(flags):
        rc = lib.simamba_add_layer_norm_bwd_ex(dn.data_ptr(), dro.data_ptr(), ro.data_ptr(),
                                               None if flags else mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), None,
                                               dres.data_ptr(), dhid.data_ptr(), part.data_ptr(), B, L, d, code, code,
                                               flags, st)
        assert rc == 0, rc

    fwd(0)                          # mean / rstd / residual_out for the backward
    fwd(_lib.NORM_RMS)
    # HBM bytes: forward reads hidden + residual, writes residual_out + normed; backward reads dnormed, dresidual_out,
    # residual_out and writes dresidual + dhidden
    s = 2 if dtype == torch.bfloat16 else 4
    mb_f = B * L * d * (s + 4 + 4 + s) / 1e6
    mb_b = B * L * d * (s + 4 + 4 + 4 + s) / 1e6
    return fwd, bwd, mb_f, mb_b


def out_norm_calls(dev, B=64, C=384, L=1024):
    lib = _lib.load()
    K = 2 * C
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.randn(B, K, L, device=dev, generator=g).bfloat16()
    w = (torch.randn(C, K, device=dev, generator=g) * K ** -0.5).bfloat16()
    res = torch.randn(B, L, C, device=dev, generator=g)
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    ro, nm = torch.empty(B, L, C, device=dev), torch.empty(B, L, C, device=dev, dtype=torch.bfloat16)
    mean, rstd = torch.empty(B * L, device=dev), torch.empty(B * L, device=dev)
    st = _lib.stream_ptr(dev)

    def run(flags):
        rc = lib.simamba_out_proj_add_ln_fwd_ex(y.data_ptr(), w.data_ptr(), res.data_ptr(), None, gamma.data_ptr(),
                                                None if flags else beta.data_ptr(), ro.data_ptr(), nm.data_ptr(),
                                                None if flags else mean.data_ptr(), rstd.data_ptr(), B, K, L, C, 1e-5,
                                                _lib.BF16, flags, st)
        assert rc == 0, rc
    return run


def train_steps(dev, rms, batch=64, npoints=1024):
    from si_mamba_amd.point_mamba import PointMamba, default_config
    from si_mamba_amd.synthetic import make_clouds
    torch.manual_seed(0)
    cfg = default_config(rms_norm=rms)
    model = PointMamba(cfg).to(dev).train()
    opt = torch.optim.AdamW(model.parameters(), lr=5e-4, weight_decay=0.05, fused=True)
    pts = make_clouds(batch, npoints, seed=0, device=dev)
    gt = torch.randint(0, cfg.cls_dim, (batch,), generator=torch.Generator().manual_seed(0)).to(dev)
    params = list(model.parameters())
    init = [p.detach().clone() for p in params]

    def step():
        with torch.no_grad():
            torch._foreach_copy_(params, init)
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss, _ = model.get_loss_acc(model(pts), gt)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 10.0)
        opt.step()
        last["loss"] = loss
    last = {}

    def timed(steps=10, warm=3):
        ms = measure.host_clock(step, steps=steps, warmup=warm)
        assert torch.isfinite(last["loss"]).item()
        return ms
    return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the JSON document to this path")
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    args = ap.parse_args()
    measure.require_gpu("bench_rms_norm.py")
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(dev), "rounds": ROUNDS,
           "note": "median [min, max] over alternating rounds; us per call (device events), ms per train step"}
    for dtype, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        fwd, bwd, mb_f, mb_b = add_norm_calls(dev, dtype)
        t = ab({"ln_fwd": lambda: events_us(lambda: fwd(0)), "rms_fwd": lambda: events_us(lambda: fwd(1)),
                "ln_bwd": lambda: events_us(lambda: bwd(0)), "rms_bwd": lambda: events_us(lambda: bwd(1))})
        t["hbm_mb_fwd"], t["hbm_mb_bwd"] = round(mb_f, 1), round(mb_b, 1)
        for k in ("ln", "rms"):
            t[f"{k}_fwd_tb_s"] = round(mb_f / t[f"{k}_fwd"][0], 2)          # MB / us = TB/s
            t[f"{k}_bwd_tb_s"] = round(mb_b / t[f"{k}_bwd"][0], 2)
        doc[f"add_norm_(64,1024,384)_{tag}"] = t
        print(json.dumps({tag: t}), file=sys.stderr, flush=True)
    on = out_norm_calls(dev)
    doc["out_proj_add_norm_bf16_(64,768->384,1024)"] = ab({"ln": lambda: events_us(lambda: on(0)),
                                                          "rms": lambda: events_us(lambda: on(1))})
    print(json.dumps(doc["out_proj_add_norm_bf16_(64,768->384,1024)"]), file=sys.stderr, flush=True)
    if not args.no_step:
        steps = {"layernorm": train_steps(dev, False), "rmsnorm": train_steps(dev, True)}
        _lib.counters.clear()
        steps["rmsnorm"](steps=1, warm=0)
        routes = dict(_lib.counters)
        doc["pointmamba_bf16_train_step_ms_(B=64)"] = ab(steps)
        doc["pointmamba_bf16_train_step_ms_(B=64)"]["rms_routes_per_step"] = routes
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
