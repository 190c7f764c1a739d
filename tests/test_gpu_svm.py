"""GPU: the linear one-vs-one SVC of csrc/svm.hip (OvOLinearSVC, evaluate_svm, ovo_vote) against the scikit-learn
fixtures of tools/gen_svm_golden.py, the KKT conditions recomputed in float64 on the host, the iteration cap, the vote
rules, determinism and the order of the rows.  Every case is a problem of at most 513 rows."""
import math
import warnings

import numpy as np
import pytest
import torch

import svm_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

PROBLEMS = ["uneven", "equal", "tiny_classes", "two", "dup", "wide"]
FIXTURES = [f"svm_{p}_{c}" for p in PROBLEMS for c in ("c001", "c1")]
U = 2.0 ** -53


@pytest.fixture(scope="module")
def fitted(device):
    """(fixture, tol) -> (golden dict, fitted model); each fit is made once and never changed."""
    from si_mamba_amd import OvOLinearSVC
    cache = {}

    def get(name, tol):
        if (name, tol) not in cache:
            g = load_golden(name)
            X, y = torch.from_numpy(g["X"]).to(device), torch.from_numpy(g["y"]).to(device)
            with warnings.catch_warnings():
                warnings.simplefilter("error", RuntimeWarning)           # an unconverged pair is a failure here
                cache[(name, tol)] = (g, OvOLinearSVC(C=float(g["C"]), tol=tol).fit(X, y))
        return cache[(name, tol)]
    return get


def _parity_bound(g):
    return 10.0 * max(float(g["cpu_gap"]), 1e-7)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_parity(fitted, device, name):
    """decision_function within 10 * max(cpu_gap, 1e-7) of scikit-learn's at tol = 1e-9: cpu_gap is the distance of the
    float64 CPU solver at the same tol = 1e-7; both stop inside the same KKT band, and the distance to the optimum
    scales with that band, not with the path taken.  predict exact (the generator kept min |dec| above 40 times that
    distance), every pair converged."""
    g, clf = fitted(name, 1e-7)
    Xt = torch.from_numpy(g["Xt"]).to(device)
    dec = clf.decision_function(Xt)
    assert dec.dtype == torch.float64 and tuple(dec.shape) == g["dec"].shape
    err = np.abs(dec.cpu().numpy() - g["dec"]).max()
    print(f"{name}: |dec - fixture| {err:.3e}, cpu_gap {float(g['cpu_gap']):.3e}, "
          f"ratio to max(cpu_gap, 1e-7) {err / max(float(g['cpu_gap']), 1e-7):.3f}, "
          f"n_iter max {int(clf.n_iter_.max())}")
    assert err <= _parity_bound(g)
    assert clf.predict(Xt).cpu().numpy().tolist() == g["pred"].tolist()
    assert clf.classes_.cpu().numpy().tolist() == sorted(set(g["y"].tolist()))
    assert bool((clf.converged_ == 1).all())
    assert clf.score(Xt, torch.from_numpy(g["pred"]).to(device)) == 1.0


@pytest.mark.parametrize("tol", [1e-3, 1e-7])
@pytest.mark.parametrize("name", FIXTURES)
def test_kkt_in_float64(fitted, device, name, tol):
    """The conditions libsvm stops on, recomputed on the host in float64 from dual_coef_pairs() and the inputs.

    0 <= alpha <= C exactly (the update clips); |y'alpha| <= n_p C 2^-50 (summed exactly with fsum).

    m - M <= tol + 2 (e_drift + e_gram + e_host), u = 2^-53, S = 1 + n_p C Kmax >= |G_t| and every partial sum of it,
    Kmax the largest diagonal entry (>= |K_st| by Cauchy-Schwarz):
      e_drift = n_iter 6 u S: an update G_t += y_t (c_i K_it + c_j K_jt) is two products, a sum, and the addition to
          G_t, each rounded once, on terms bounded by C Kmax <= S and by S;
      e_gram = 2 (d + 2) u Kmax n_p C: an entry of either Gram matrix (the device's and the host's) is a d-term dot
          product, (d + 2) u Kmax off, times sum |alpha| <= n_p C;
      e_host = (n_p + 2) u S: the host's own sum of n_p terms.
    The kernel stopped with m - M < tol on its G; the host's G differs from it by at most the sum of the three at each
    of the two positions that make m and M.

    coef_ = sum alpha y x and decision_function = X coef_' + intercept_, each to the rounding of a float64 sum:
    (terms + 2) u times the sum of the absolute values of the terms."""
    g, clf = fitted(name, tol)
    C = float(g["C"])
    X = g["X"].astype(np.float64)
    d = X.shape[1]
    pairs = clf.dual_coef_pairs()
    coef = clf.coef_.cpu().numpy()
    n_iter = clf.n_iter_.cpu().numpy()
    assert len(pairs) == coef.shape[0] == len(clf.classes_) * (len(clf.classes_) - 1) // 2
    classes = clf.classes_.cpu().numpy()
    for p, (a, b, rows, alpha) in enumerate(pairs):
        rows, alpha = rows.cpu().numpy(), alpha.cpu().numpy()
        want_rows = np.concatenate([np.flatnonzero(g["y"] == classes[a]), np.flatnonzero(g["y"] == classes[b])])
        assert rows.tolist() == want_rows.tolist()
        na = int((g["y"] == classes[a]).sum())
        n_p = len(rows)
        y = np.where(np.arange(n_p) < na, 1.0, -1.0)
        assert alpha.min() >= 0.0 and alpha.max() <= C
        assert abs(math.fsum(alpha * y)) <= n_p * C * 2.0 ** -50
        K = X[rows] @ X[rows].T
        G = y * (K @ (alpha * y)) - 1.0
        up = np.where(y > 0, alpha < C, alpha > 0)
        low = np.where(y > 0, alpha > 0, alpha < C)
        m, M = (-y * G)[up].max(), (-y * G)[low].min()
        kmax = np.diag(K).max()
        S = 1.0 + n_p * C * kmax
        e = n_iter[p] * 6 * U * S + 2 * (d + 2) * U * kmax * n_p * C + (n_p + 2) * U * S
        assert m - M <= tol + 2.0 * e, (p, m - M, e)
        w = (alpha * y) @ X[rows]
        wb = (n_p + 2) * U * (np.abs(alpha)[:, None] * np.abs(X[rows])).sum(0)
        assert (np.abs(coef[p] - w) <= wb).all(), p
    Xt = torch.from_numpy(g["Xt"]).to(device)
    dec = clf.decision_function(Xt).cpu().numpy()
    icpt = clf.intercept_.cpu().numpy()
    Xt64 = g["Xt"].astype(np.float64)
    want = Xt64 @ coef.T + icpt
    db = (d + 3) * U * (np.abs(Xt64) @ np.abs(coef).T + np.abs(icpt))
    assert (np.abs(dec - want) <= db).all()


def test_iteration_cap(fitted, device):
    """max_iter = 3 returns at once, says which pairs needed more, leaves a feasible alpha and warns.  With a loop exit
    that is not uniform over the workgroup this test does not fail: it runs until it is killed."""
    from si_mamba_amd import OvOLinearSVC
    g, full = fitted("svm_equal_c1", 1e-7)
    X, y = torch.from_numpy(g["X"]).to(device), torch.from_numpy(g["y"]).to(device)
    with pytest.warns(RuntimeWarning, match="3 of 3 class pairs"):
        clf = OvOLinearSVC(C=1.0, tol=1e-7, max_iter=3).fit(X, y)
    assert (full.n_iter_ > 3).all()
    assert clf.n_iter_.tolist() == [3, 3, 3] and clf.converged_.tolist() == [0, 0, 0]
    for a, b, rows, alpha in clf.dual_coef_pairs():
        alpha = alpha.cpu().numpy()
        yy = np.where(np.arange(len(alpha)) < 30, 1.0, -1.0)
        assert alpha.min() >= 0.0 and alpha.max() <= 1.0 and alpha.max() > 0.0
        assert abs(math.fsum(alpha * yy)) <= len(alpha) * 2.0 ** -50
    # a cap that is enough says so
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        ok =OvOLinearSVC(C=1.0, tol=1e-7, max_iter=int(full.n_iter_.max()) + 1).fit(X, y)
    assert ok.converged_.tolist() == [1, 1, 1] and torch.equal(ok.coef_, full.coef_)


def test_votes(device):
    from si_mamba_amd.svm import ovo_vote
    nan = float("nan")
    dec = torch.tensor([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [nan, nan, nan], [1.0, -1.0, 1.0], [-1.0, 1.0, -1.0],
                        [-1.0, -1.0, 1.0], [-0.0, 5.0, nan]], dtype=torch.float64, device=device)
    want = [0, 2, 2, 0, 0, 1, 0]
    assert svm_ref.vote(dec.cpu().numpy(), 3).tolist() == want
    pred, matches = ovo_vote(dec, 3)
    assert pred.dtype == torch.int32 and pred.tolist() == want and matches is None
    labels = torch.tensor([0, 2, 1, 0, 7, 1, -1], device=device)
    pred, matches = ovo_vote(dec, 3, labels)
    assert pred.tolist() == want and matches.dtype == torch.int64 and matches.tolist() == [4]
    two = torch.tensor([[0.0], [1e-300], [nan], [-1.0]], dtype=torch.float64, device=device)
    assert ovo_vote(two, 2)[0].tolist() == [1, 0, 1, 1]
    # 64 classes, more rows than one workgroup, against the restatement
    gen = torch.Generator().manual_seed(0)
    big = torch.randn(261, 2016, generator=gen, dtype=torch.float64)
    big[big.abs() < 0.3] = 0.0
    big[5, ::7] = nan
    want = svm_ref.vote(big.numpy(), 64)
    pred, matches = ovo_vote(big.to(device), 64, torch.from_numpy(want.astype(np.int64)).to(device))
    assert pred.tolist() == want.tolist() and matches.item() == 261


def test_determinism(fitted, device):
    """Two fits: the same bits.  bfloat16 rows are widened, so they fit as their float32 values do."""
    from si_mamba_amd import OvOLinearSVC
    g, first = fitted("svm_uneven_c1", 1e-3)
    X, y = torch.from_numpy(g["X"]).to(device), torch.from_numpy(g["y"]).to(device)
    again = OvOLinearSVC(C=1.0).fit(X, y)
    assert torch.equal(first.coef_, again.coef_) and torch.equal(first.intercept_, again.intercept_)
    assert torch.equal(first.n_iter_, again.n_iter_)
    for (_, _, r1, a1), (_, _, r2, a2) in zip(first.dual_coef_pairs(), again.dual_coef_pairs()):
        assert torch.equal(r1, r2) and torch.equal(a1, a2)
    half = OvOLinearSVC(C=1.0).fit(X.bfloat16(), y)
    wide = OvOLinearSVC(C=1.0).fit(X.bfloat16().float(), y)
    assert torch.equal(half.coef_, wide.coef_) and torch.equal(half.intercept_, wide.intercept_)


@pytest.mark.parametrize("name", ["svm_dup_c001", "svm_dup_c1"])
def test_labels_and_order(device, name):
    """The rows in another order (labels 3, 7, 40; every point twice): the same decision values within the parity
    bound, the same predictions."""
    from si_mamba_amd import OvOLinearSVC
    g = load_golden(name)
    perm = np.random.default_rng(5).permutation(len(g["y"]))
    X, y = torch.from_numpy(g["X"][perm]).to(device), torch.from_numpy(g["y"][perm]).to(device)
    clf = OvOLinearSVC(C=float(g["C"]), tol=1e-7).fit(X, y.int())
    Xt = torch.from_numpy(g["Xt"]).to(device)
    err = np.abs(clf.decision_function(Xt).cpu().numpy() - g["dec"]).max()
    print(f"{name} reshuffled: |dec - fixture| {err:.3e}")
    assert err <= _parity_bound(g)
    assert clf.classes_.tolist() == [3, 7, 40] and clf.predict(Xt).tolist() == g["pred"].tolist()


def test_evaluate_svm_on_tokens(device):
    """(N, 1, d) tokens X / 2: mean + max gives X back exactly in fp32, so the accuracy is the fixture's own."""
    from si_mamba_amd import evaluate_svm
    g = load_golden("svm_uneven_c001")
    X, y = torch.from_numpy(g["X"]).to(device), torch.from_numpy(g["y"]).to(device)
    Xt = torch.from_numpy(g["Xt"]).to(device)
    rng = np.random.default_rng(1)
    yt = np.where(rng.random(len(g["pred"])) < 0.25, (g["pred"] + 1) % 5, g["pred"])     # some wrong on purpose
    want = float((g["pred"] == yt).mean())
    assert 0.0 < want < 1.0
    yt = torch.from_numpy(yt).to(device)
    got = evaluate_svm((X / 2)[:, None, :], y, (Xt / 2)[:, None, :], yt, C=0.01)
    assert isinstance(got, float) and got == want
    assert evaluate_svm(X, y, Xt, yt, C=0.01) == want
    # several tokens: the pooling is the reference's mean(1) + max(1)
    tok, tok_t = torch.stack([X / 2, X / 2 - 1.0, X / 2 - 2.0], 1), torch.stack([Xt / 2, Xt / 2 - 1.0, Xt / 2 - 2.0], 1)
    assert evaluate_svm(tok, y, tok_t, yt) == evaluate_svm(tok.mean(1) + tok.max(1)[0], y,
                                                           tok_t.mean(1) + tok_t.max(1)[0], yt)


def test_evaluate_svm_on_model_features(device):
    from si_mamba_amd import evaluate_svm
    from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
    torch.manual_seed(0)
    model = Point_MAE_Mamba(default_mae_config(trans_dim=64, encoder_dims=64, depth=2, decoder_depth=1)).to(device).eval()
    gen = torch.Generator().manual_seed(2)
    labels = torch.arange(24) % 3
    pts = torch.randn(24, 1024, 3, generator=gen) * (1.0 + labels.float())[:, None, None] * 0.3
    with torch.no_grad():
        feats = model(pts.to(device), noaug=True)
    assert feats.dim() == 3 and feats.shape[0] == 24 and feats.shape[2] == 64
    acc = evaluate_svm(feats[:18], labels[:18].to(device), feats[18:], labels[18:].to(device))
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0
