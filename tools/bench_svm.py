#!/usr/bin/env python
"""Times the device linear SVC (si_mamba_amd.OvOLinearSVC) at the size of the reference's pre-training validation on
ModelNet40 -- 9 843 train rows, 2 468 test rows, 384 features, 40 classes -- on synthetic class-mean features with a
fixed seed, and scikit-learn's SVC(C=0.01, kernel='linear') on the same data beside it when it is importable on the
host.  Prints one JSON line and saves it (default profiles/svm.json).

    python tools/bench_svm.py [--out profiles/svm.json] [--spread 1.0] [--repeat 5]

Device times are host clocks around work that ends in a synchronise, after one warm-up fit + predict; the Gram matrix
(a library GEMM) is inside the fit time.  No GPU: the tool fails, it does not fall back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import measure  # noqa: E402


def make(n_train, n_test, d, nc, spread, seed):
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((nc, d))
    ytr, yte = np.arange(n_train) % nc, np.arange(n_test) % nc
    rng.shuffle(ytr)
    Xtr = means[ytr] + spread * rng.standard_normal((n_train, d))
    Xte = means[yte] + spread * rng.standard_normal((n_test, d))
    return Xtr.astype(np.float32), ytr.astype(np.int64), Xte.astype(np.float32), yte.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svm.json"))
    ap.add_argument("--n-train", type=int, default=9843)
    ap.add_argument("--n-test", type=int, default=2468)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--spread", type=float, default=1.0, help="noise std per feature; the class means are unit normal")
    ap.add_argument("--C", type=float, default=0.01)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    measure.require_gpu("bench_svm.py")
    from si_mamba_amd import OvOLinearSVC
    dev = torch.device("cuda:0")
    Xtr, ytr, Xte, yte = make(a.n_train, a.n_test, a.dim, a.classes, a.spread, a.seed)
    X, y, Xt, yt = (torch.from_numpy(v).to(dev) for v in (Xtr, ytr, Xte, yte))

    def sync_time(fn):
        out = []
        ms = measure.host_clock(lambda: out.append(fn()), steps=1, warmup=0)
        return out[0], ms / 1e3

    clf = OvOLinearSVC(C=a.C).fit(X, y)          # warm-up: code objects, the GEMM's choice of algorithm
    clf.predict(Xt)
    fit_s, pred_s = [], []
    for _ in range(a.repeat):
        clf, t = sync_time(lambda: OvOLinearSVC(C=a.C).fit(X, y))
        fit_s.append(t)
        pred, t = sync_time(lambda: clf.predict(Xt))
        pred_s.append(t)
    acc = clf.score(Xt, yt)
    res = dict(bench="svm", n_train=a.n_train, n_test=a.n_test, dim=a.dim, classes=a.classes, spread=a.spread, C=a.C,
               seed=a.seed, device=torch.cuda.get_device_name(0), repeat=a.repeat,
               device_fit_s=min(fit_s), device_fit_s_all=fit_s, device_predict_s=min(pred_s),
               device_predict_s_all=pred_s, device_accuracy=acc, n_iter_max=int(clf.n_iter_.max()),
               n_iter_sum=int(clf.n_iter_.sum()), pairs=int(clf.n_iter_.numel()),
               unconverged_pairs=int((clf.converged_ == 0).sum()))
    if not a.no_sklearn:
        try:
            from sklearn.svm import SVC
        except ImportError:
            res["sklearn"] = "not importable on this host"
        else:
            import sklearn
            t0 = time.perf_counter()
            ref = SVC(C=a.C, kernel="linear").fit(Xtr, ytr)
            t1 = time.perf_counter()
            ref_pred = ref.predict(Xte)
            t2 = time.perf_counter()
            res.update(sklearn=sklearn.__version__, sklearn_fit_s=t1 - t0, sklearn_predict_s=t2 - t1,
                       sklearn_accuracy=float((ref_pred == yte).mean()),
                       predictions_equal=int((ref_pred == pred.cpu().numpy()).sum()), host_cpus=os.cpu_count())
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
