#!/usr/bin/env python
"""Times the device t-SNE (si_mamba_amd.TSNE) at the size of the reference's feature map of the ModelNet40 test split --
2 468 rows of 384 features, 40 class-mean blobs built as tools/bench_svm.py builds them -- and scikit-learn's TSNE on
the same data when it is importable on the host.  Updates one JSON file (default profiles/tsne.json) and prints it.

    python tools/bench_tsne.py [--out profiles/tsne.json] [--sizes 2468,16384] [--repeat 3]
    python tools/bench_tsne.py --host-only                    # scikit-learn's two fits alone; needs no device
    python tools/bench_tsne.py --iterations-only              # a short run of iterations, for a kernel trace
    python tools/bench_tsne.py --no-device --kernel-stats <rocprofv3 *_kernel_stats.csv> --errors-log <pytest -s log>

Sections of the file, each written by the mode that measures it and left alone by the others:
  device     fit time (host clock around a synchronised fit, Gram matrix, calibration and PCA inside), calibrate time,
             and per size the time of one iteration inside a run of 200 enqueued back to back (two events round the
             call) beside the host time the call took to enqueue them
  kernels    the mean duration of each tsne_* kernel from a rocprofv3 kernel trace of --iterations-only
  errors     the "tsne-err" lines tests/test_gpu_tsne.py prints: measured error and bound of every case
  host       scikit-learn's default (Barnes-Hut) and method='exact' fits
No GPU: the device modes fail, they do not fall back."""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import measure  # noqa: E402

ITERS = 200


def make(n, d, nc, spread, seed):
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((nc, d))
    y = np.arange(n) % nc
    return (means[y] + spread * rng.standard_normal((n, d))).astype(np.float32), y


def knn1(Y, y):
    import torch
    Y = torch.as_tensor(Y, dtype=torch.float64)
    d = torch.cdist(Y, Y)
    d.fill_diagonal_(float("inf"))
    return float((torch.as_tensor(y)[d.argmin(1)] == torch.as_tensor(y)).double().mean())


def iteration_times(X, a):
    """One size: the state after the exaggerated stage, then ITERS iterations of the second stage in one call."""
    import torch
    from si_mamba_amd.manifold import tsne
    dev = X.device
    n = X.shape[0]
    cond, _ = tsne.calibrate(tsne.squared_distances(X), a.perplexity)
    P, s = tsne.joint_probabilities(cond)
    del cond
    Y = tsne.pca_init(X).contiguous()
    upd, gains = torch.zeros_like(Y), torch.ones_like(Y)
    ws, lr = tsne.workspace(n, dev), max(n / 12.0 / 4.0, 50.0)
    st = tsne.new_status(dev, 0)
    tsne.run(P, Y, upd, gains, st, s, 0, 250, exaggeration=12.0, momentum=0.5, learning_rate=lr, ws=ws,
             n_iter_without_progress=250)
    upd.zero_()
    gains.fill_(1.0)
    st = tsne.new_status(dev, 250)
    torch.cuda.synchronize()
    ev, host, first = [], [], [250]

    def call():
        t0 = time.perf_counter()
        tsne.run(P, Y, upd, gains, st, s, first[0], ITERS, exaggeration=1.0, momentum=0.8, learning_rate=lr, ws=ws,
                 n_iter_without_progress=10 ** 6, min_grad_norm=0.0)
        host.append((time.perf_counter() - t0) * 1e6 / ITERS)
        first[0] += ITERS
    for _ in range(a.repeat):
        ev.append(measure.window(call, 1) * 1e3 / ITERS)
    assert st.tolist()[tsne.ST_STOPPED] == 0.0
    g = lambda: tsne.gradient(P, Y, 1.0, s, ws)                  # noqa: E731
    return dict(n=n, iteration_us=measure.summary(ev, 2), enqueue_us_per_iteration=measure.summary(host, 2),
                gradient_call_us=round(measure.calls(g, warmup=3, reps=50) * 1e3, 2),
                pairs=n * n, p_bytes=4 * n * n, workspace_floats=int(ws.numel()))


def device_section(a):
    import torch
    measure.require_gpu("bench_tsne.py")
    from si_mamba_amd import TSNE
    from si_mamba_amd.manifold import tsne
    dev = torch.device("cuda:0")
    Xn, y = make(a.n, a.dim, a.classes, a.spread, a.seed)
    X = torch.from_numpy(Xn).to(dev)
    if a.iterations_only:
        print(json.dumps(iteration_times(X, a)))
        return None
    TSNE(perplexity=a.perplexity).fit(X)                          # warm-up: code objects, the GEMM's choice, eigh
    fits = []
    for _ in range(a.repeat):
        out = []
        fits.append(measure.host_clock(lambda: out.append(TSNE(perplexity=a.perplexity).fit(X)), steps=1, warmup=0) / 1e3)
    m = out[0]
    d2 = tsne.squared_distances(X)
    cal = measure.calls(lambda: tsne.calibrate(d2, a.perplexity), warmup=1, reps=5)
    res = dict(device=torch.cuda.get_device_name(0), n=a.n, dim=a.dim, classes=a.classes, spread=a.spread,
               perplexity=a.perplexity, max_iter=m.max_iter, fit_s=min(fits), fit_s_all=fits, n_iter=m.n_iter_,
               kl_divergence=m.kl_divergence_, knn1_accuracy=knn1(m.embedding_.cpu(), y), calibrate_ms=round(cal, 3),
               sizes=[])
    for n in a.sizes:
        Xs = X if n == a.n else torch.from_numpy(make(n, a.dim, a.classes, a.spread, a.seed)[0]).to(dev)
        res["sizes"].append(iteration_times(Xs, a))
    return res


def host_section(a):
    try:
        import sklearn
        from sklearn.manifold import TSNE
    except ImportError:
        return dict(sklearn="not importable on this host")
    Xn, y = make(a.n, a.dim, a.classes, a.spread, a.seed)
    res = dict(sklearn=sklearn.__version__, host_cpus=os.cpu_count(), n=a.n, dim=a.dim)
    for method in ("barnes_hut", "exact"):
        t0 = time.perf_counter()
        m = TSNE(n_components=2, init="pca", random_state=0, perplexity=a.perplexity, method=method).fit(Xn)
        res[method] = dict(fit_s=round(time.perf_counter() - t0, 2), n_iter=int(m.n_iter_),
                           kl_divergence=float(m.kl_divergence_), knn1_accuracy=knn1(m.embedding_, y))
    return res


def kernel_section(path):
    """Mean duration of the tsne_* kernels from rocprofv3's kernel stats (Name, Calls, TotalDurationNs, AverageNs, ...)."""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name", "")
            if "tsne_" in name:
                short = re.sub(r"^.*?(tsne_\w+)(<[^>]*>)?.*$", r"\1\2", name)
                out[short] = dict(calls=int(row["Calls"]), mean_us=round(float(row["AverageNs"]) / 1e3, 2))
    return out


def errors_section(path):
    out = {}
    with open(path) as fh:
        for what, err, bound in re.findall(r"tsne-err (.+?): err (\S+) bound (\S+)", fh.read()):
            out[what] = dict(err=float(err), bound=float(bound))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne.json"))
    ap.add_argument("--n", type=int, default=2468)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--spread", type=float, default=1.0)
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sizes", type=lambda s: [int(v) for v in s.split(",")], default=[2468, 16384])
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--iterations-only", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--kernel-stats-size", type=int, default=2468, help="the N the kernel trace was taken at")
    ap.add_argument("--errors-log")
    a = ap.parse_args()
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.load(fh)
    res["bench"] = "tsne"
    if a.host_only:
        res["host"] = host_section(a)
    elif not a.no_device:
        dev = device_section(a)
        if dev is None:
            return
        res["device"] = dev
    if a.kernel_stats:
        res.setdefault("kernels", {})[f"n{a.kernel_stats_size}"] = kernel_section(a.kernel_stats)
    if a.errors_log:
        res["errors"] = errors_section(a.errors_log)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
