"""Mixing augmentations (csrc/mix.hip, si_mamba_amd.mixing) on one GPU, beside what a user did without them and
beside the closest kernel the tree already had.

Two batches, 64 clouds x 1024 points and 16 clouds x 8192 points.  Per batch and op (cutmix R, cutmix K at lambda = 0.5,
pointwolf with 4 anchors, mixup at N <= 1024):
  kernel_us        the op, eager calls back to back and one replay of its hipGraph; device events around 5 windows of
                   ~50 ms per variant, the variants alternating (measure.alternate)
  torch_us         the same thing composed from torch ops on the device (rand / topk / sort / gather for cutmix, an
                   argmax loop and einsum for pointwolf), in the same alternation.  It draws other random numbers and
                   rounds differently; it is the yardstick for "no kernel", nothing more
  host_loop_ms     the numpy restatement (tests/mix_ref.py) cloud by cloud with the copy to the host in front and the
                   copy back behind it; wall clock, the median of 3 passes.  The restatement is written to be read
  drop_local_us    corruptions.corrupt(..., "drop_local", total = N / 2, max_clusters = 1) at the same shape in the
                   same alternation: one 45-pass counting select over the cloud against cutmix K's two
and, once:
  expf             the largest relative error of the device library's expf, as csrc/mix.hip's flags compile it
                   (tools/expf_probe.hip), against float64 over [-80, 0]: 2^24 uniform arguments and 2^22 log-uniform
                   ones in [-1, -1e-8].  tests/mix_ref.py's EPS_EXP is twice this figure
  error_over_bound the largest error of pointwolf (and of the normalisation behind it) as a fraction of the bound
                   tests/test_gpu_mix.py holds it to: the test's own checks, run here on the test's clouds and on the
                   first batch

``SIMAMBA_LIB=<path>`` times another build of the library (measure.use_lib_from_env).

    python tools/bench_mix.py [--out profiles/mix.json]
"""
import argparse
import ctypes
import json
import math
import os
import subprocess
import sys
import tempfile
import time
from statistics import median

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools import measure  # noqa: E402

SHAPES = ((64, 1024), (16, 8192))
ANCHORS = 4
WOLF = dict(sigma=0.5, rot=math.radians(10), scale=3.0, trans=0.25)


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


# ---- the torch-ops compositions --------------------------------------------------------------------------------------
def torch_cutmix(pts, partner, m, mode):
    B, N, _ = pts.shape
    other = pts[partner]
    if mode == "r":
        own_key, other_key = torch.rand(B, N, device=pts.device), torch.rand(B, N, device=pts.device)
    else:
        seeds = torch.randint(0, N, (B, 2), device=pts.device)
        rows = torch.arange(B, device=pts.device)
        own_key = (pts - pts[rows, seeds[:, 0]].unsqueeze(1)).square().sum(-1)
        other_key = (other - other[rows, seeds[:, 1]].unsqueeze(1)).square().sum(-1)
    keep = own_key.topk(N - m, dim=1, largest=True).indices.sort(1).values
    take = other_key.topk(m, dim=1, largest=False).indices.sort(1).values
    pick = lambda t, i: torch.gather(t, 1, i.unsqueeze(-1).expand(-1, -1, 3))      # noqa: E731
    return torch.cat([pick(pts, keep), pick(other, take)], 1)


def torch_pointwolf(pts, M, sigma, rot, scale, trans):
    B, N, _ = pts.shape
    dev = pts.device
    rows = torch.arange(B, device=dev)
    idx = torch.randint(0, N, (B,), device=dev)
    anchors = [pts[rows, idx]]
    mind = (pts - anchors[0].unsqueeze(1)).square().sum(-1)
    for _ in range(1, M):
        anchors.append(pts[rows, mind.argmax(1)])
        mind = torch.minimum(mind, (pts - anchors[-1].unsqueeze(1)).square().sum(-1))
    a = torch.stack(anchors, 1)                                      # (B, M, 3)
    ang = (2 * torch.rand(B, M, 3, device=dev) - 1) * rot
    f = 1 + torch.rand(B, M, 3, device=dev) * (scale - 1)
    f = torch.where(torch.rand(B, M, 1, device=dev) < 0.5, 1 / f, f)
    t = (2 * torch.rand(B, M, 3, device=dev) - 1) * trans
    c, s = ang.cos(), ang.sin()
    one, zero = torch.ones_like(c[..., 0]), torch.zeros_like(c[..., 0])
    Rx = torch.stack([one, zero, zero, zero, c[..., 0], -s[..., 0], zero, s[..., 0], c[..., 0]], -1).view(B, M, 3, 3)
    Ry = torch.stack([c[..., 1], zero, s[..., 1], zero, one, zero, -s[..., 1], zero, c[..., 1]], -1).view(B, M, 3, 3)
    Rz = torch.stack([c[..., 2], -s[..., 2], zero, s[..., 2], c[..., 2], zero, zero, zero, one], -1).view(B, M, 3, 3)
    R = Rz @ Ry @ Rx
    d = pts.unsqueeze(1) - a.unsqueeze(2)                            # (B, M, N, 3)
    q = torch.einsum("bmij,bmnj->bmni", R, d * f.unsqueeze(2)) + (a + t).unsqueeze(2)
    d2 = d.square().sum(-1)
    w = torch.exp(-(d2 - d2.min(1, keepdim=True).values) / (2 * sigma * sigma)).unsqueeze(-1)
    out = (w * q).sum(1) / w.sum(1)
    out = out - out.mean(1, keepdim=True)
    return out / out.norm(dim=-1).max(1).values.view(B, 1, 1)


# ---- the host loops --------------------------------------------------------------------------------------------------
def host_cutmix(pts, mode, seed, step):
    import mix_ref as mr
    host = pts.cpu().numpy()
    q = mr.partner_map(len(host), seed, step)
    out = np.stack([mr.cutmix_cloud(host[b], host[q[b]], mr.MODE[mode], 0.5, seed, step, b)["out"]
                    for b in range(len(host))])
    return torch.from_numpy(out).to(pts.device)


def host_pointwolf(pts, seed, step):
    import mix_ref as mr
    from dataset_ref import unit_sphere64
    host = pts.cpu().numpy()
    par = [WOLF[k] for k in ("sigma", "rot", "scale", "trans")]
    out = np.stack([unit_sphere64(mr.pointwolf_cloud(host[b], ANCHORS, par, seed, step, b)["out"])[0]
                    for b in range(len(host))])
    return torch.from_numpy(out.astype(np.float32)).to(pts.device)


def host_ms(fn):
    got = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        got.append(1e3 * (time.perf_counter() - t0))
    return round(median(got), 2)


def shape_figures(B, N, dev):
    from si_mamba_amd import corruptions, mixing
    from si_mamba_amd.transforms import AugmentState
    import mix_ref as mr
    g = torch.Generator().manual_seed(0)
    pts = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(dev)
    st = AugmentState(1, dev)
    half = torch.full((B,), 0.5, device=dev)
    partner = torch.randperm(B, generator=g).to(dev)
    out = torch.empty_like(pts)
    wolf_out = torch.empty_like(pts)
    drop_out = torch.empty_like(pts)
    ops = {
        "cutmix_r": lambda: mixing.cutmix(pts, "r", lam=half, state=st, out=out),
        "cutmix_k": lambda: mixing.cutmix(pts, "k", lam=half, state=st, out=out),
        "pointwolf": lambda: mixing.pointwolf(pts, anchors=ANCHORS, state=st, out=wolf_out, **WOLF),
        "drop_local": lambda: corruptions.corrupt(pts, "drop_local", total=N // 2, max_clusters=1, state=st,
                                                  out=drop_out),
    }
    torch_ops = {
        "cutmix_r": lambda: torch_cutmix(pts, partner, N // 2, "r"),
        "cutmix_k": lambda: torch_cutmix(pts, partner, N // 2, "k"),
        "pointwolf": lambda: torch_pointwolf(pts, ANCHORS, **WOLF),
    }
    if N <= 1024:
        ops["mixup"] = lambda: mixing.mixup(pts, lam=half, state=st)
    timed = {}
    for name, fn in ops.items():
        timed[name + "/eager"] = fn
        timed[name + "/graph"] = _capture(fn).replay
    for name, fn in torch_ops.items():
        timed[name + "/torch"] = fn
    acc = measure.alternate(timed, target_ms=50.0, windows=5, reverse_odd=True)
    us = {k: measure.summary([1e3 * x for x in v], 2) for k, v in acc.items()}
    host = {
        "cutmix_r": host_ms(lambda: host_cutmix(pts, "r", mr.SEED, mr.STEP)),
        "cutmix_k": host_ms(lambda: host_cutmix(pts, "k", mr.SEED, mr.STEP)),
        "pointwolf": host_ms(lambda: host_pointwolf(pts, mr.SEED, mr.STEP)),
    }
    res = dict(B=B, N=N, drop_local_us=dict(eager=us["drop_local/eager"], graph=us["drop_local/graph"]), ops={})
    for name in ops:
        if name == "drop_local":
            continue
        row = dict(kernel_us=dict(eager=us[name + "/eager"], graph=us[name + "/graph"]))
        if name + "/torch" in us:
            row["torch_us"] = us[name + "/torch"]
            row["torch_over_kernel"] = round(us[name + "/torch"]["median"] / us[name + "/eager"]["median"], 1)
        if name in host:
            row["host_loop_ms"] = host[name]
            row["host_loop_over_kernel"] = round(1e3 * host[name] / us[name + "/eager"]["median"], 1)
        row["over_drop_local"] = round(us[name + "/graph"]["median"] / us["drop_local/graph"]["median"], 2)
        res["ops"][name] = row
    return res


def expf_error(dev):
    """The probe built beside this file if it is not there yet (hipcc, the flags of csrc/mix.hip)."""
    here = os.path.dirname(os.path.abspath(__file__))
    lib = os.path.join(here, "expf_probe.so")
    tmp = None
    if not os.path.exists(lib):
        tmp = tempfile.TemporaryDirectory()
        lib = os.path.join(tmp.name, "expf_probe.so")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC",
                        "--offload-arch=gfx950", "-ffp-contract=off", "-shared", os.path.join(here, "expf_probe.hip"),
                        "-o", lib], check=True)
    probe = ctypes.CDLL(lib).expf_probe
    probe.restype = ctypes.c_int
    probe.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
    g = torch.Generator().manual_seed(0)
    x = torch.cat([-80.0 * torch.rand(1 << 24, generator=g),
                   -torch.exp(torch.rand(1 << 22, generator=g, dtype=torch.float64) * math.log(1e-8)).float(),
                   torch.tensor([0.0, -0.0, -80.0])]).to(dev)
    y = torch.empty_like(x)
    code = probe(x.data_ptr(), y.data_ptr(), x.numel(), None)
    torch.cuda.synchronize()
    assert code == 0, code
    want = torch.exp(x.double())
    rel = ((y.double() - want).abs() / want)
    worst = int(rel.argmax())
    ulp = (y.double() - want).abs() / (torch.nextafter(y, torch.full_like(y, float("inf"))) - y).double()
    return dict(range=[-80.0, 0.0], samples=x.numel(), max_relative_error=float(rel.max()), at=float(x[worst]),
                max_ulp=round(float(ulp.max()), 3), eps_exp_used_by_the_tests=2 * float(rel.max()))


def error_ratios(dev):
    """tests/test_gpu_mix.py's own checks: on its clouds, and on the first batch of this tool."""
    import test_gpu_mix as tg
    tg.MEASURED.clear()
    for lengths in tg.WOLF_LENGTHS:
        for anchors, sigma in ((1, 0.5), (4, 0.5), (8, 0.3)):
            pts = tg.padded(lengths, seed=sum(lengths) + anchors)
            ln = torch.tensor(lengths, device=dev)
            tg.check_wolf(pts, lengths, anchors, tg.wolf_run(pts.to(dev), ln, anchors, sigma=sigma), sigma=sigma)
    for lengths in tg.WOLF_LENGTHS[:2]:
        tg.test_pointwolf_renorm_within_the_dataset_routine_bound(dev, lengths)
    B, N = SHAPES[0]
    g = torch.Generator().manual_seed(0)
    pts = torch.rand(B, N, 3, generator=g) * 2 - 1
    tg.check_wolf(pts, [N] * B, ANCHORS, tg.wolf_run(pts.to(dev), None, ANCHORS))
    return {k: round(v, 4) for k, v in tg.MEASURED.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("expf", "errors", "times"), default=None)
    args = ap.parse_args()
    measure.require_gpu("bench_mix.py")
    measure.use_lib_from_env()
    dev = torch.device("cuda:0")
    res = dict(
        what="mixing augmentations on one MI355X: mixing.cutmix (R and K, lambda = 0.5), mixing.pointwolf (4 anchors, "
             "normalised) and mixing.mixup in us per batch, eager calls back to back and hipGraph replays, events "
             "around 5 windows of ~50 ms per variant, all variants of a shape alternating; torch_us: the same "
             "composed from torch ops on the device; host_loop_ms: the per-cloud numpy restatement with both copies, "
             "wall clock (median of 3); drop_local_us: corruptions.corrupt drop_local (total = N / 2, one cluster) at "
             "the same shape in the same alternation, one counting select against cutmix K's two; expf: the device "
             "library's expf against float64; error_over_bound: pointwolf's largest error as a fraction of the bound "
             "tests/test_gpu_mix.py holds it to",
        device=torch.cuda.get_device_name(0))
    if args.only in (None, "expf"):
        res["expf"] = expf_error(dev)
    if args.only in (None, "errors"):
        res["error_over_bound"] = error_ratios(dev)
    if args.only in (None, "times"):
        res["shapes"] = [shape_figures(B, N, dev) for B, N in SHAPES]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
