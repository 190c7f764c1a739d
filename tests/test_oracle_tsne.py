"""CPU: tests/tsne_ref.py, the float64 restatement the GPU tests measure against, is scikit-learn's exact t-SNE -- against
scikit-learn itself where it is installed, and against tests/golden/tsne_*.npz (written from scikit-learn by
tools/gen_tsne_golden.py) everywhere.

Bounds.  P: scikit-learn keeps the conditional rows in float32 (a relative 6e-8 per entry) and divides by their measured
sum where the restatement divides by 2 N (the rows sum to 1 within float32 rounding): a relative 2e-6 covers a sum of
two entries and the normaliser several times over.  The beta sequences themselves are the same: the same start, the
same doubling, halving and bisection.  Gradient, KL and the 60 steps run on scikit-learn's own P in float64 on both
sides and differ by summation order alone, 1e-16 a term.  The 60 steps run at the learning rate N / 48 (scikit-learn's
'auto' without its floor of 50): with the floor, at N ~ 100, the first steps are chaotic -- two float64 runs were 3e-10
apart after 20 steps and O(1) apart after 60 -- and no trajectory bound could be stated; at N / 48 the runs stay within
2e-12 of each other, so 1e-9 of the largest magnitude leaves three digits."""
import numpy as np
import pytest

import tsne_ref
from conftest import load_golden

CASES = ["init_n96", "spread_n128", "dup_n65"]
FITS = [(96, 8, 3, 10.0), (200, 16, 4, 30.0), (333, 16, 5, 30.0)]


def _close(got, want, rel):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - want).max()
    assert err <= rel * max(np.abs(want).max(), 1e-300), (err, np.abs(want).max())


def _check_case(g):
    n = g["d2"].shape[0]
    rows, beta = tsne_ref.calibrate(g["d2"], float(g["perplexity"]))
    assert np.isfinite(rows).all() and np.isfinite(beta).all() and (np.diag(rows) == 0).all()
    P = tsne_ref.joint(rows)
    off = ~np.eye(n, dtype=bool)
    np.testing.assert_allclose(P[off], g["P"][off], rtol=2e-6, atol=2 * tsne_ref.MACHINE_EPSILON)
    # the restatement on scikit-learn's own P
    alpha = float(g["alpha"])
    kl, grad = tsne_ref.grad_kl(g["P"], g["Y0"], alpha)
    assert abs(kl - float(g["kl"])) <= 1e-9 * abs(float(g["kl"]))
    _close(grad, g["grad"], 1e-9)
    out = tsne_ref.gradient_descent(g["P"], g["Y0"], 0, 60, alpha, float(g["momentum"]), float(g["lr"]), 300)
    assert out["done"] == 60 and not out["stopped"]
    _close(out["Y"], g["Y60"], 1e-9)


@pytest.mark.parametrize("case", CASES)
def test_restatement_against_the_golden_files(case):
    _check_case(load_golden("tsne_" + case))


def test_restatement_against_scikit_learn():
    pytest.importorskip("sklearn")
    pytest.importorskip("scipy")
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("gen_tsne_golden", os.path.join(ROOT, "tools", "gen_tsne_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for case in gen.CASES.values():
        _check_case(gen.sklearn_case(*case))
    # one more draw than the files hold
    _check_case(gen.sklearn_case(77, 5, 4, 9, 7.0, 12.0, "init"))


def test_entropy_of_the_calibrated_rows():
    for case in CASES:
        g = load_golden("tsne_" + case)
        _, beta = tsne_ref.calibrate(g["d2"], float(g["perplexity"]))
        _, H = tsne_ref.rows_from_beta(g["d2"], beta)
        assert np.abs(H - np.log(float(g["perplexity"]))).max() <= tsne_ref.PERPLEXITY_TOL


def test_stop_rule_and_schedule():
    X, y = tsne_ref.blobs(60, 6, 3, 0)
    rows, _ = tsne_ref.calibrate(tsne_ref.squared_distances(X), 8.0)
    P = tsne_ref.joint(rows)
    Y0 = tsne_ref.pca_init(X)
    assert abs(Y0[:, 0].std() - 1e-4) < 1e-12
    out = tsne_ref.fit(P, Y0, 300, min_grad_norm=1e9)
    assert out["n_iter"] == 50                                  # the first check
    out = tsne_ref.fit(P, Y0, 300)
    assert out["n_iter"] == 300 and tsne_ref.knn1_accuracy(out["Y"], y) == 1.0
    # a rate of 0 moves nothing: the check at 350 sets the best error, the one at 400 equals it and is 50 > window later
    still = tsne_ref.gradient_descent(P, out["Y"], 300, 1000, 1.0, 0.8, 0.0, 49)
    assert still["stopped"] and still["done"] == 400
    still = tsne_ref.gradient_descent(P, out["Y"], 300, 1000, 1.0, 0.8, 0.0, 50)
    assert still["stopped"] and still["done"] == 450


def test_whole_fit_fixtures_say_what_the_issue_checked():
    """The float64 reference and its float32 run reach 1-NN accuracy 1.0 on the three blob problems, and the KL after
    400 iterations is below the KL after the exaggerated stage."""
    for n, _, _, _ in FITS:
        g = load_golden(f"tsne_fit_{n}")
        assert g["acc64"] == 1.0 and g["acc32"] == 1.0
        assert 0 < g["kl_final"] < g["kl_250"]
        assert 0 <= g["margin"] < 0.2
