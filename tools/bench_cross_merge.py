"""The per-layer cross-merge of add_after_layer=True (csrc/cross_merge.hip) against the reference's own sequence of
torch ops (cross_merge.cross_merge_composed, what MixerModel_add.composed runs), one MI355X:
  * forward and forward + backward of the op at (64, 1024, 384) (G = 128, k = 4) and (32, 512, 384) (G = 64), fp32 and
    bf16, with the achieved bytes/s over the algorithmic traffic 2 B L C sizeof(T) per pass;
  * for information, the PointMamba train step (bench.py's step: B = 64, 1024 points, 12 blocks, AdamW, bf16 autocast
    and fp32) with the option on, kernel against composed.
Op calls are timed with device events over 50 calls after a warm-up, train steps over 10 steps after 3; every
measurement alternates the two forms for 5 rounds and reports the median [min, max].  Before anything is timed the two
forms are compared on the timed inputs (fp32 forward: bit for bit).  One JSON document on stdout (and to --out)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from si_mamba_amd.cross_merge import cross_merge, cross_merge_composed, cross_merge_maps  # noqa: E402
from tools import measure  # noqa: E402

ROUNDS = 5
SHAPES = [(64, 128, 4, 384), (32, 64, 4, 384)]          # (B, G, k, C): L = 2 k G


def events_us(fn):
    return measure.calls(fn, warmup=5, reps=50) * 1e3


def ab(fns):
    """{name: fn} -> {name: [median, min, max]} over ROUNDS alternating rounds"""
    return {k: measure.stats(v, 2) for k, v in measure.rounds(fns, ROUNDS).items()}


def op_calls(dev, dtype, B, G, k, C):
    g = torch.Generator(device=dev).manual_seed(0)
    L = 2 * k * G
    order = torch.rand(B, k, G, device=dev, generator=g).argsort(dim=-1)
    maps = cross_merge_maps(order)
    x = torch.randn(B, L, C, device=dev, generator=g).to(dtype)
    dout = torch.randn(B, L, C, device=dev, generator=g).to(dtype)
    xg = x.clone().requires_grad_(True)

    def fwd_kernel():
        return cross_merge(x, maps)

    def fwd_composed():
        return cross_merge_composed(x, order)

    def both(f):
        def run():
            xg.grad = None
            f(xg).backward(dout)
            return xg.grad
        return run
    fb_kernel = both(lambda t: cross_merge(t, maps))
    fb_composed = both(lambda t: cross_merge_composed(t, order))
    # the two forms compute the same thing on the timed inputs.  fp32 forward: bit for bit.  The composed backward is
    # autograd's (its own order of the same 2k - 1 additions) and the composed bf16 form rounds after every addition
    # where the kernel rounds once: both within 2 * 2k roundings of a sum of 2k terms.
    a, b = fwd_kernel(), fwd_composed()
    ga, gb = fb_kernel().clone(), fb_composed().clone()
    if dtype == torch.float32:
        assert torch.equal(a, b)
    eps = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -8
    for got, want, terms in ((a, b, x), (ga, gb, dout)):
        assert float((got.float() - want.float()).abs().max()) <= 4 * k * eps * 2 * k * float(terms.float().abs().max())
    mb = 2 * B * L * C * x.element_size() / 1e6            # one pass: L rows read, L rows written
    return {"fwd_kernel": fwd_kernel, "fwd_composed": fwd_composed, "fwd_bwd_kernel": fb_kernel,
            "fwd_bwd_composed": fb_composed}, mb


def train_steps(dev, composed, autocast, batch=64, npoints=1024):
    from si_mamba_amd.point_mamba import PointMamba, default_config
    from si_mamba_amd.synthetic import make_clouds
    torch.manual_seed(0)
    cfg = default_config(add_after_layer=True)
    model = PointMamba(cfg).to(dev).train()
    model.blocks.composed = composed
    opt = torch.optim.AdamW(model.parameters(), lr=5e-4, weight_decay=0.05, fused=True)
    pts = make_clouds(batch, npoints, seed=0, device=dev)
    gt = torch.randint(0, cfg.cls_dim, (batch,), generator=torch.Generator().manual_seed(0)).to(dev)
    params = list(model.parameters())
    init = [p.detach().clone() for p in params]

    def step():
        with torch.no_grad():
            torch._foreach_copy_(params, init)
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
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
    ap.add_argument("--no-step", action="store_true", help="the op only")
    args = ap.parse_args()
    measure.require_gpu("bench_cross_merge.py")
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(dev), "rounds": ROUNDS,
           "note": "median [min, max] over alternating rounds; us per call (device events), ms per train step; "
                   "tb_s = passes * 2 B L C sizeof(T) over the median (fwd: 1 pass, fwd_bwd: 2)"}
    for B, G, k, C in SHAPES:
        for dtype, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
            fns, mb = op_calls(dev, dtype, B, G, k, C)
            t = ab({name: (lambda f=f: events_us(f)) for name, f in fns.items()})
            t["mb_per_pass"] = round(mb, 1)
            for name in fns:
                passes = 2 if name.startswith("fwd_bwd") else 1
                t[f"{name}_tb_s"] = round(passes * mb / t[name][0], 2)         # MB / us = TB/s
            t["kernel_no_slower"] = bool(t["fwd_kernel"][0] <= t["fwd_composed"][0]
                                         and t["fwd_bwd_kernel"][0] <= t["fwd_bwd_composed"][0])
            doc[f"cross_merge_({B},{2 * k * G},{C})_{tag}"] = t
            print(json.dumps({f"({B},{2 * k * G},{C})_{tag}": t}), file=sys.stderr, flush=True)
    if not args.no_step:
        for autocast, tag in ((True, "bf16"), (False, "f32")):
            steps = {"kernel": train_steps(dev, False, autocast), "composed": train_steps(dev, True, autocast)}
            doc[f"pointmamba_add_after_layer_{tag}_train_step_ms_(B=64)"] = ab(steps)
            print(json.dumps(doc[f"pointmamba_add_after_layer_{tag}_train_step_ms_(B=64)"]), file=sys.stderr, flush=True)
            del steps
            torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
