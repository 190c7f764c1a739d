"""Point-cloud corruptions (csrc/corrupt.hip, si_mamba_amd.corruptions) on one GPU, beside what a user did without them:
copy the batch to the host, run numpy cloud by cloud, pad, copy back.

One batch of 64 clouds of 1024 points, every kind at severity 5.  Per kind:
  kernel_us        corruptions.corrupt, eager calls back to back and one replay of its hipGraph; device events around 5
                   windows of ~0.1 s per variant, the variants alternating (measure.alternate)
  host_loop_ms     the numpy restatement (tests/corrupt_ref.py) over the 64 clouds with the copy to the host in front
                   and the padded copy back behind it; wall clock, the median of 3 passes.  The restatement is written
                   to be read, not to be fast: it is the yardstick for "a per-cloud loop on the host", nothing more
  error_over_bound the largest error of the kernel's batch against the restatement as a fraction of the bound
                   tests/test_gpu_corrupt.py holds that kind to (its own check, run here on this batch); the exact parts
                   (lengths, sources, copied rows, the zero tail) are asserted by the same check
and ``renorm``: the same fraction for the unit-sphere normalisation behind every kind.

``SIMAMBA_LIB=<path>`` times another build of the library (measure.use_lib_from_env).

    python tools/bench_corrupt.py [--out profiles/corrupt.json]
"""
import argparse
import json
import os
import sys
import time
from statistics import median

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools import measure  # noqa: E402

B, N, SEVERITY_LEVEL = 64, 1024, 5


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


def host_loop(pts, kind, params, seed, step):
    """The pattern the kernel replaces: to the host, numpy per cloud, pad, back to the device."""
    import corrupt_ref as cf
    code, names = cf.KIND[kind]
    host = pts.cpu().numpy()
    res = [cf.corrupt_cloud(host[b], code, [params[k] for k in names], seed, step, b, renorm=(kind == "scale"))["out"]
           for b in range(len(host))]
    K = max(len(r) for r in res)
    out = np.zeros((len(res), K, 3), dtype=np.float32)
    for b, r in enumerate(res):
        out[b, :len(r)] = r
    lengths = torch.tensor([len(r) for r in res])
    return torch.from_numpy(out).to(pts.device), lengths.to(pts.device)


def kind_figures(kind, pts, errors):
    from si_mamba_amd import corruptions
    from si_mamba_amd.transforms import AugmentState
    import test_gpu_corrupt as tg
    params = corruptions.SEVERITY[kind][SEVERITY_LEVEL - 1]
    st = AugmentState(1, pts.device)
    adds = {"add_global": params.get("count"), "add_local": params.get("total")}.get(kind, 0)
    out = torch.empty(B, N + adds, 3, device=pts.device)
    kernel = lambda: corruptions.corrupt(pts, kind, SEVERITY_LEVEL, state=st, out=out)   # noqa: E731
    graph = _capture(kernel)
    acc = measure.alternate({"eager": kernel, "graph": graph.replay}, target_ms=100.0, windows=5, reverse_odd=True)
    us = {k: measure.summary([1e3 * x for x in v], 2) for k, v in acc.items()}
    host = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_loop(pts, kind, params, tg.SEED, tg.STEP)
        torch.cuda.synchronize()
        host.append(1e3 * (time.perf_counter() - t0))
    # the test's own check on this batch: exact parts asserted, the rest as a fraction of its bound
    tg.MEASURED.clear()
    cpu, lengths = pts.cpu(), [N] * B
    tg.check(cpu, lengths, kind, tg.run(pts, kind, **params), **params)
    errors[kind] = round(tg.MEASURED[kind], 4)
    raw = tg.run(pts, kind, **params)
    nrm = tg.run(pts, kind, **{**params, "renorm": True})
    worst = 0.0
    for b in range(B):
        n = int(nrm[1][b])
        want, bound = tg.unit_sphere64(raw[0][b, :n].double().cpu().numpy())
        worst = max(worst, float(np.abs(nrm[0][b, :n].double().cpu().numpy() - want).max() / bound))
    errors["renorm"] = round(max(errors.get("renorm", 0.0), worst), 4)
    return dict(kind=kind, params=params, K=out.shape[1], kernel_us=us, host_loop_ms=round(median(host), 2),
                host_loop_over_kernel=round(1e3 * median(host) / us["eager"]["median"], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    measure.require_gpu("bench_corrupt.py")
    measure.use_lib_from_env()
    from si_mamba_amd import corruptions
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    pts = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(dev)
    errors = {}
    kinds = [kind_figures(k, pts, errors) for k in corruptions.KINDS]
    line = json.dumps(dict(
        what="point-cloud corruptions, one batch of 64 clouds x 1024 points, every kind at severity 5, one MI355X: "
             "corruptions.corrupt (one launch + the step kernel) in us per batch, eager calls back to back and hipGraph "
             "replays, events around 5 windows of ~0.1 s per variant, the variants alternating; beside it the per-cloud "
             "numpy restatement on the host with both copies, wall-clock ms per batch (median of 3); error_over_bound: "
             "the kernel's largest error against the restatement as a fraction of the bound tests/test_gpu_corrupt.py "
             "holds the kind to",
        device=torch.cuda.get_device_name(0), B=B, N=N, severity=SEVERITY_LEVEL, kinds=kinds, error_over_bound=errors))
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
