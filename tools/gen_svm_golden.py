#!/usr/bin/env python
"""Writes tests/golden/svm_<problem>_<c>.npz: small one-vs-one linear SVC problems solved by scikit-learn's
SVC(C, kernel='linear', decision_function_shape='ovo', tol=1e-9) (libsvm), the fixtures of tests/test_oracle_svm.py and
tests/test_gpu_svm.py.  Needs scikit-learn; run once, commit the files.

Each file holds X (N, d) float32, y (N,) int64, Xt (M, d) float32, C, dec (M, P) float64 in libsvm's sign (scikit-learn's
is negated for two classes), pred (M,) int64 and cpu_gap: the largest |dec - dec of tests/svm_ref.py at tol = 1e-7|.
A draw is kept only when min |dec| > 40 * max(cpu_gap, 1e-7), so that no prediction hangs on a value inside the
tolerances the tests use; otherwise the next seed is drawn.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svm_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
C_VALUES = {"c001": 0.01, "c1": 1.0}
N_TEST = 24


def blobs(rng, sizes, labels, d, spread):
    """Gaussian classes around random means; ``spread`` is the noise relative to the distance of the means."""
    means = rng.standard_normal((len(sizes), d))
    X = np.concatenate([m + spread * rng.standard_normal((n, d)) for m, n in zip(means, sizes)])
    y = np.concatenate([np.full(n, l) for l, n in zip(labels, sizes)])
    cls = rng.integers(0, len(sizes), N_TEST)
    Xt = means[cls] + spread * rng.standard_normal((N_TEST, d))
    return X, y, Xt


def uneven(rng):
    return blobs(rng, [40, 25, 17, 9, 5], [0, 1, 2, 3, 4], 24, 0.8)


def equal(rng):
    return blobs(rng, [30, 30, 30], [0, 1, 2], 16, 2.5)          # heavy overlap: many alpha at C


def tiny_classes(rng):
    X, y, Xt = blobs(rng, [64, 3, 1, 20], [0, 1, 2, 3], 8, 0.7)
    perm = rng.permutation(len(y))
    return X[perm], y[perm], Xt


def two(rng):
    X, y, Xt = blobs(rng, [1, 1], [5, 2], 4, 0.5)                # labels 5 then 2: class 0 is the SECOND row
    return X, y, Xt


def dup(rng):
    X, y, Xt = blobs(rng, [10, 10, 10], [3, 7, 40], 6, 1.0)
    X, y = np.concatenate([X, X]), np.concatenate([y, y])        # every point twice: zero curvature between twins
    perm = rng.permutation(len(y))
    return X[perm], y[perm], Xt


def wide(rng):
    return blobs(rng, [300, 213], [0, 1], 8, 1.2)                # n_p = 513 = 2 * 256 + 1


PROBLEMS = dict(uneven=uneven, equal=equal, tiny_classes=tiny_classes, two=two, dup=dup, wide=wide)


def solve(X, y, Xt, C):
    from sklearn.svm import SVC
    clf = SVC(C=C, kernel="linear", decision_function_shape="ovo", tol=1e-9).fit(X.astype(np.float64), y)
    dec = clf.decision_function(Xt.astype(np.float64))
    if dec.ndim == 1:
        dec = -dec[:, None]                                       # scikit-learn flips the binary case
    pred = clf.predict(Xt.astype(np.float64))
    model = svm_ref.fit(X, y, C, tol=1e-7)
    assert model["converged"].all()
    mine = svm_ref.decision_function(model, Xt)
    gap = float(np.abs(mine - dec).max())
    assert (svm_ref.predict(model, Xt) == pred).all()
    return dec, pred.astype(np.int64), gap


def main():
    import sklearn
    print("scikit-learn", sklearn.__version__)
    for name, make in PROBLEMS.items():
        for seed in range(100):
            rng = np.random.default_rng([seed, sum(map(ord, name))])
            X, y, Xt = make(rng)
            X, Xt = X.astype(np.float32), Xt.astype(np.float32)
            got = {tag: solve(X, y, Xt, C) for tag, C in C_VALUES.items()}
            if all(np.abs(dec).min() > 40.0 * max(gap, 1e-7) for dec, _, gap in got.values()):
                break
        else:
            raise SystemExit(f"{name}: no seed passed the margin rule")
        for tag, (dec, pred, gap) in got.items():
            assert np.abs(dec).min() > 40.0 * max(gap, 1e-7)
            np.savez(os.path.join(OUT, f"svm_{name}_{tag}.npz"), X=X, y=y.astype(np.int64), Xt=Xt,
                     C=np.float64(C_VALUES[tag]), dec=dec, pred=pred, cpu_gap=np.float64(gap))
            print(f"{name:13s} {tag:5s} seed {seed:2d}  N {len(y):4d}  min|dec| {np.abs(dec).min():.2e}  "
                  f"cpu_gap {gap:.2e}")


if __name__ == "__main__":
    main()
