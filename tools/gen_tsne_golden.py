#!/usr/bin/env python
"""Writes the t-SNE fixtures of tests/test_oracle_tsne.py and tests/test_gpu_tsne.py.  Run once, commit the files.

tests/golden/tsne_<case>.npz (needs scikit-learn; N <= 128): scikit-learn's own functions on a small blob problem --
d2 (N, N) float32 squared distances, perplexity, P (N, N) float64 from ``_joint_probabilities``, Y0 (N, 2) float64,
alpha, kl and grad from ``_kl_divergence`` of alpha P at Y0, lr (N / 48), momentum, and Y60: Y0 after 60 iterations of
``_gradient_descent`` on alpha P (n_iter_check = 50).

tests/golden/tsne_fit_<n>.npz (tests/tsne_ref.py alone): the float64 reference's whole fit of the blob problems the GPU
test fits -- kl_final after max_iter = 400, kl_250 (the KL of P at the embedding after the 250 exaggerated iterations),
acc64 / acc32 (1-NN label accuracy of the float64 and the float32 run), and margin: 1.1 times the relative spread
(max - min) / kl_final of the final KL over five runs whose initial Y is perturbed by 1e-7 relative.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tsne_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
# case -> (n, d, k, seed, perplexity, alpha, kind of Y0)
CASES = {"init_n96": (96, 8, 3, 0, 10.0, 12.0, "init"), "spread_n128": (128, 16, 4, 1, 30.0, 1.0, "spread"),
         "dup_n65": (65, 6, 3, 2, 12.0, 4.0, "init")}
FITS = [(96, 8, 3, 10.0), (200, 16, 4, 30.0), (333, 16, 5, 30.0)]       # (n, d, k, perplexity), seed 0
FIT_ITER = 400


def sklearn_case(n, d, k, seed, perplexity, alpha, kind):
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne
    X, _ = tsne_ref.blobs(n, d, k, seed)
    if kind == "init" and n == 65:
        # duplicated rows, d2 = 0 off the diagonal: nine copies of one point, fewer than the perplexity of 12 -- with
        # more copies than that no beta reaches the entropy, and scikit-learn's unshifted exp underflows whole rows to
        # zero where the kernel and tests/tsne_ref.py keep the nearest neighbours
        X[1::8] = X[0]
    d2 = tsne_ref.squared_distances(X)
    P = _t_sne._joint_probabilities(d2, perplexity, 0)
    rng = np.random.default_rng(seed + 100)
    Y0 = rng.standard_normal((n, 2)) * (1e-4 if kind == "init" else 3.0)
    args = [P * alpha, 1.0, n, 2]
    kl, grad = _t_sne._kl_divergence(Y0.ravel(), *args)
    # scikit-learn's 'auto' rate without its floor of 50: at N ~ 100 the floor makes the first steps chaotic (two float64
    # runs that differ in summation order alone are 1e-10 apart after 20 steps and O(1) apart after 60), and no bound
    # on a trajectory could be stated; at N / 48 the 60 steps amplify nothing
    lr = n / 12.0 / 4.0
    Y60, _, _ = _t_sne._gradient_descent(_t_sne._kl_divergence, Y0.ravel().copy(), 0, 60, n_iter_check=50,
                                         momentum=0.5, learning_rate=lr, args=args)
    return dict(d2=d2, perplexity=np.float64(perplexity), P=squareform(P), Y0=Y0, alpha=np.float64(alpha),
                kl=np.float64(kl), grad=grad.reshape(n, 2), lr=np.float64(lr), momentum=np.float64(0.5),
                Y60=Y60.reshape(n, 2))


def fit_case(n, d, k, perplexity):
    X, y = tsne_ref.blobs(n, d, k, 0)
    rows, _ = tsne_ref.calibrate(tsne_ref.squared_distances(X), perplexity)
    P = tsne_ref.joint(rows)
    Y0 = tsne_ref.pca_init(X)
    ref = tsne_ref.fit(P, Y0, FIT_ITER, keep=(tsne_ref.EXPLORATION_ITER,))
    kl_250 = float(tsne_ref.grad_kl(P, ref["kept"][tsne_ref.EXPLORATION_ITER])[0])
    low = tsne_ref.fit(P.astype(np.float32), Y0, FIT_ITER, dtype=np.float32)
    rng = np.random.default_rng(n)
    kls = [tsne_ref.fit(P, Y0 * (1.0 + 1e-7 * rng.standard_normal(Y0.shape)), FIT_ITER)["kl"] for _ in range(5)]
    margin = 1.1 * (max(kls) - min(kls)) / ref["kl"]
    return dict(kl_final=np.float64(ref["kl"]), kl_250=np.float64(kl_250), margin=np.float64(margin),
                acc64=np.float64(tsne_ref.knn1_accuracy(ref["Y"], y)),
                acc32=np.float64(tsne_ref.knn1_accuracy(low["Y"], y)), kl32=np.float64(low["kl"]),
                perturbed=np.asarray(kls))


def main():
    for n, d, k, perplexity in FITS:
        out = fit_case(n, d, k, perplexity)
        np.savez(os.path.join(OUT, f"tsne_fit_{n}.npz"), **out)
        print(f"fit n {n:4d}: kl {out['kl_final']:.6f}  kl_250 {out['kl_250']:.6f}  kl32 {out['kl32']:.6f}  "
              f"margin {out['margin']:.3e}  acc {out['acc64']:.3f} / {out['acc32']:.3f}")
    import sklearn
    print("scikit-learn", sklearn.__version__)
    for name, case in CASES.items():
        out = sklearn_case(*case)
        np.savez(os.path.join(OUT, f"tsne_{name}.npz"), **out)
        print(f"{name}: kl {out['kl']:.6f}  |grad| {np.abs(out['grad']).max():.3e}")


if __name__ == "__main__":
    main()
