"""CPU: the float64 restatement of the one-vs-one linear SVC (svm_ref.py) against the scikit-learn fixtures of
tools/gen_svm_golden.py, its vote rules on hand-built decision values, and -- where scikit-learn is installed -- a live
comparison."""
import numpy as np
import pytest

import svm_ref
from conftest import load_golden

PROBLEMS = ["uneven", "equal", "tiny_classes", "two", "dup", "wide"]
FIXTURES = [f"svm_{p}_{c}" for p in PROBLEMS for c in ("c001", "c1")]


@pytest.fixture(scope="module")
def solved():
    """Every fixture with the restatement's model at tol = 1e-7, computed once."""
    out = {}
    for name in FIXTURES:
        g = load_golden(name)
        out[name] = (g, svm_ref.fit(g["X"], g["y"], float(g["C"]), tol=1e-7))
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_against_fixture(solved, name):
    """dec within 2 * max(cpu_gap, 1e-7): cpu_gap is this solver's own distance on the generating machine, and another
    BLAS build rounds the Gram matrix differently.  pred exact; the generator kept only draws whose smallest |dec| is 40
    times that distance."""
    g, model = solved[name]
    assert model["converged"].all()
    dec = svm_ref.decision_function(model, g["Xt"])
    assert dec.shape == g["dec"].shape
    bound = 2.0 * max(float(g["cpu_gap"]), 1e-7)
    assert np.abs(dec - g["dec"]).max() <= bound
    assert np.abs(g["dec"]).min() > 40.0 * max(float(g["cpu_gap"]), 1e-7)
    np.testing.assert_array_equal(svm_ref.predict(model, g["Xt"]), g["pred"])
    for _, _, rows, alpha in model["pairs"]:
        assert alpha.min() >= 0.0 and alpha.max() <= float(g["C"])


def test_two_has_no_free_alpha_at_small_c(solved):
    """The fixture that reaches the midpoint branch of the rho rule: both alpha sit at C."""
    g, model = solved["svm_two_c001"]
    (a, b, rows, alpha), = model["pairs"]
    assert (a, b) == (0, 1) and list(model["classes"]) == [2, 5]
    assert rows.tolist() == [1, 0]                       # class 2 is the second row given
    assert (alpha == float(g["C"])).all()


def test_dup_reaches_zero_curvature():
    g = load_golden("svm_dup_c1")
    X = g["X"].astype(np.float64)
    K = X @ X.T
    twins = [(i, j) for i in range(len(X)) for j in range(i + 1, len(X)) if (X[i] == X[j]).all()]
    assert len(twins) == 30
    # zero up to the rounding of three GEMM entries (a BLAS sums a diagonal and an off-diagonal entry in different
    # orders): of either sign, so the curvature floor is reached whenever it comes out <= 0
    d = X.shape[1]
    assert all(abs(K[i, i] + K[j, j] - 2.0 * K[i, j]) <= 4.0 * d * 2.0 ** -53 * K[i, i] for i, j in twins)
    assert sorted(set(g["y"].tolist())) == [3, 7, 40]


def test_vote_rules():
    nan = float("nan")
    # three classes, pairs (0,1) (0,2) (1,2)
    dec = np.array([
        [1.0, 1.0, 1.0],      # 0 beats 1 and 2: class 0
        [0.0, 0.0, 0.0],      # exactly 0 votes b: 1, 2, 2 -> class 2
        [nan, nan, nan],      # NaN votes b: class 2
        [1.0, -1.0, 1.0],     # 0 over 1, 2 over 0, 1 over 2: one vote each -> the lowest, class 0
        [-1.0, 1.0, -1.0],    # the other cycle: a three-way tie again -> class 0
        [-1.0, -1.0, 1.0],    # 1, 2, 1 -> class 1
        [-0.0, 5.0, nan],     # -0.0 is not > 0: 1, 0, 2 -> a tie -> class 0
    ])
    assert svm_ref.vote(dec, 3).tolist() == [0, 2, 2, 0, 0, 1, 0]
    assert svm_ref.vote(np.array([[0.0], [1e-300], [nan], [-1.0]]), 2).tolist() == [1, 0, 1, 1]


def test_pooling():
    f = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    np.testing.assert_array_equal(svm_ref.pool(f), f.mean(1) + f.max(1))
    assert svm_ref.pool(f[:, 0]) is not None and svm_ref.pool(f[:, 0]).shape == (2, 4)


def test_rho_midpoint_rule():
    y = np.array([1.0, -1.0])
    # both at the upper bound: ub comes from y = -1, lb from y = +1
    assert svm_ref.rho_of(np.array([0.5, 0.5]), np.array([-0.2, -0.6]), y, 0.5) == (0.6 + -0.2) / 2.0
    # one free alpha: its yG alone
    assert svm_ref.rho_of(np.array([0.25, 0.5]), np.array([-0.2, -0.6]), y, 0.5) == -0.2


def test_iteration_cap_leaves_a_feasible_alpha():
    g = load_golden("svm_equal_c1")
    model = svm_ref.fit(g["X"], g["y"], 1.0, tol=1e-7, max_iter=3)
    assert not model["converged"].any() and (model["n_iter"] == 3).all()
    for _, _, rows, alpha in model["pairs"]:
        yy = np.where(np.arange(len(rows)) < 30, 1.0, -1.0)
        assert alpha.min() >= 0.0 and alpha.max() <= 1.0 and abs(alpha @ yy) <= len(rows) * 2.0 ** -50


def test_live_against_scikit_learn():
    svm = pytest.importorskip("sklearn.svm")
    rng = np.random.default_rng(7)
    means = rng.standard_normal((4, 10))
    sizes = [20, 13, 8, 3]
    X = np.concatenate([m + 0.9 * rng.standard_normal((n, 10)) for m, n in zip(means, sizes)]).astype(np.float32)
    y = np.concatenate([np.full(n, l) for l, n in zip([11, -4, 6, 0], sizes)])
    Xt = rng.standard_normal((16, 10)).astype(np.float32)
    for C in (0.01, 1.0):
        clf = svm.SVC(C=C, kernel="linear", decision_function_shape="ovo", tol=1e-9).fit(X.astype(np.float64), y)
        model = svm_ref.fit(X, y, C, tol=1e-7)
        want = clf.decision_function(Xt.astype(np.float64))
        got = svm_ref.decision_function(model, Xt)
        assert np.abs(got - want).max() < 1e-4           # both stop inside their KKT bands: 1e-7 and 1e-9 of gradient
        decided = np.abs(want).min(axis=1) > 1e-3
        np.testing.assert_array_equal(svm_ref.predict(model, Xt)[decided], clf.predict(Xt.astype(np.float64))[decided])
