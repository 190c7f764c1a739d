"""GPU: exact t-SNE on the device (csrc/tsne.hip, si_mamba_amd/manifold) against the float64 restatement of
tests/tsne_ref.py.

Tolerances of the calibration, gradient / KL and trajectory groups are not fixed numbers: the yardstick is the float32
run of tsne_ref against its float64 run on the very inputs of the case, so it scales with N and with the cancellation in
P - Q, and the device gets 8 times that deviation (summation order; v_rcp_f32 and v_exp_f32 in place of correctly
rounded operations), with a floor of 1e-6 of the largest magnitude (``tsne_ref.bound``).  Every case prints its measured
error and its bound before it asserts (``-s`` shows them; profiles/tsne.json records them).
"""
import functools

import numpy as np
import pytest
import torch

import tsne_ref
from conftest import load_golden
from guarded_alloc import SENTINEL, ZERO, guarded, place, same_bits
from helpers import clouds

pytestmark = pytest.mark.gpu

F64 = np.float64
F32 = np.float32


def _dev(a, device, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(dtype).to(device)


def _np(t):
    return t.detach().cpu().numpy()


def _report(what, err, bound):
    print(f"tsne-err {what}: err {err:.3e} bound {bound:.3e}")


# ---- calibration -----------------------------------------------------------------------------------------------------
def _cal_cases():
    out = []
    for n in (2, 65, 96, 333, 1025):
        for perp in (5.0, 30.0):
            if perp < n:
                out.append((f"n{n}-p{perp:g}", n, perp, "plain"))
    out.append(("n2-p1.5", 2, 1.5, "plain"))            # one neighbour: no beta reaches log 1.5; the search halves 100 times
    out.append(("n96-p5-dup8", 96, 5.0, "dup"))          # more copies than the perplexity: beta doubles 100 times
    out.append(("n96-p30-dup8", 96, 30.0, "dup"))
    out.append(("n333-p30-x1e4", 333, 30.0, "scaled"))   # exp(-d2) underflows the whole unshifted row at beta = 1
    return out


@functools.lru_cache(maxsize=None)
def _cal_d2(n, kind):
    X, _ = tsne_ref.blobs(n, 8, 4, n)
    if kind == "dup":
        X[1:9] = X[0]                                    # 8 more rows equal to row 0
    d2 = tsne_ref.squared_distances(X)
    if kind == "scaled":
        d2 = (d2 * F32(1e4)).astype(F32)
    d2.setflags(write=False)
    return d2


@pytest.mark.parametrize("name,n,perp,kind", _cal_cases(), ids=[c[0] for c in _cal_cases()])
def test_calibrate(name, n, perp, kind, device):
    from si_mamba_amd.manifold import tsne
    d2 = _cal_d2(n, kind)
    cond, beta = tsne.calibrate(_dev(d2, device), perp)
    cond, beta = _np(cond), _np(beta)
    assert np.isfinite(cond).all() and np.isfinite(beta).all() and (beta > 0).all()
    assert (np.diag(cond) == 0).all() and (cond >= 0).all()
    with np.errstate(over="ignore", invalid="ignore"):
        rows64, H64 = tsne_ref.rows_from_beta(d2, beta, F64)
        rows32, H32 = tsne_ref.rows_from_beta(d2, beta.astype(F32), F32)
        _, beta_ref = tsne_ref.calibrate(d2, perp, F64)
        _, Href = tsne_ref.rows_from_beta(d2, beta_ref, F64)
    # the rows at the beta returned, to fp32 rounding
    err, bound = tsne_ref.deviation(cond, rows64), tsne_ref.bound(rows32, rows64)
    _report(f"calibrate {name} rows", err, bound)
    assert err <= bound
    np.testing.assert_allclose(cond.sum(1, dtype=F64), 1.0, rtol=0, atol=1e-5)
    # the entropy, on every row whose target can be reached at all (the float64 search reaches it)
    target = np.log(perp)
    reach = np.abs(Href - target) <= tsne_ref.PERPLEXITY_TOL
    assert reach.all() or kind == "dup" or n == 2
    if reach.any():
        slack = tsne_ref.bound(H32[reach], H64[reach])
        herr = float(np.abs(H64[reach] - target).max())
        _report(f"calibrate {name} entropy", herr, tsne_ref.PERPLEXITY_TOL + slack)
        assert herr <= tsne_ref.PERPLEXITY_TOL + slack


# ---- gradient and KL -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(n, d=8, k=4, perp=30.0, seed=None):
    """(X, labels, P float32) of a blob problem; P from the float64 restatement, rounded to the device's storage."""
    X, y = tsne_ref.blobs(n, d, k, n if seed is None else seed)
    rows, _ = tsne_ref.calibrate(tsne_ref.squared_distances(X), perp)
    P = tsne_ref.joint(rows).astype(F32)
    P.setflags(write=False)
    return X, y, P


@pytest.mark.parametrize("kind", ["spread", "init"])
@pytest.mark.parametrize("n", [65, 96, 257, 333, 1025])
def test_gradient_and_kl(n, kind, device):
    from si_mamba_amd.manifold import tsne
    _, _, P = _problem(n)
    rng = np.random.default_rng(n + 7)
    Y = (rng.standard_normal((n, 2)) * (5.0 if kind == "spread" else 1e-4)).astype(F32)
    alpha = 1.0 if kind == "spread" else 12.0
    grad, kl = tsne.gradient(_dev(P, device), _dev(Y, device), alpha)
    grad, kl = _np(grad), float(kl.item())
    _, g64 = tsne_ref.grad_kl(P, Y, alpha, F64)
    _, g32 = tsne_ref.grad_kl(P, Y, alpha, F32)
    kl64 = float(tsne_ref.grad_kl(P, Y, 1.0, F64)[0])
    kl32 = float(tsne_ref.grad_kl(P, Y, 1.0, F32)[0])
    err, bound = tsne_ref.deviation(grad, g64), tsne_ref.bound(g32, g64)
    _report(f"gradient n{n} {kind}", err, bound)
    kerr, kbound = abs(kl - kl64), tsne_ref.bound(kl32, kl64)
    _report(f"kl n{n} {kind}", kerr, kbound)
    assert err <= bound
    assert kerr <= kbound


# ---- trajectory ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _settled(n):
    """The float64 reference's state after 300 iterations, rounded to the device's storage."""
    X, _, P = _problem(n)
    lr = max(n / 12.0 / 4.0, 50.0)
    a = tsne_ref.gradient_descent(P, tsne_ref.pca_init(X), 0, 250, 12.0, 0.5, lr, 250)
    b = tsne_ref.gradient_descent(P, a["Y"], 250, 300, 1.0, 0.8, lr, 300)
    return P, lr, tuple(b[k].astype(F32) for k in ("Y", "update", "gains"))


@pytest.mark.parametrize("n", [96, 333])
def test_trajectory_of_five_steps(n, device):
    from si_mamba_amd.manifold import tsne
    P, lr, (Y, update, gains) = _settled(n)
    ref = {}
    for dt in (F64, F32):
        ref[dt] = tsne_ref.gradient_descent(P, Y, 300, 305, 1.0, 0.8, lr, 300, dtype=dt, update=update, gains=gains)
    Pd = _dev(P, device)
    Yd, ud, gd = _dev(Y, device), _dev(update, device), _dev(gains, device)
    status = tsne.new_status(device, 300)
    sum_plogp = torch.tensor([tsne_ref.sum_plogp(P)], dtype=torch.float64, device=device)
    tsne.run(Pd, Yd, ud, gd, status, sum_plogp, 300, 5, exaggeration=1.0, momentum=0.8, learning_rate=lr)
    err, bound = tsne_ref.deviation(_np(Yd), ref[F64]["Y"]), tsne_ref.bound(ref[F32]["Y"], ref[F64]["Y"])
    _report(f"trajectory n{n}", err, bound)
    st = status.tolist()
    assert err <= bound
    # the last iteration of a call computes the error: the KL at the Y the fifth step started from
    assert st[tsne.ST_ITERS] == 305 and st[tsne.ST_STOPPED] == 0
    assert abs(st[tsne.ST_KL] - ref[F64]["error"]) <= tsne_ref.bound(ref[F32]["error"], ref[F64]["error"])


# ---- whole fits ------------------------------------------------------------------------------------------------------
FITS = [(96, 8, 3, 10.0), (200, 16, 4, 30.0), (333, 16, 5, 30.0)]


@pytest.mark.parametrize("n,d,k,perp", FITS)
def test_whole_fit(n, d, k, perp, device):
    """kl_divergence_ against the reference's final KL times (1 + margin) and against its KL after the exaggerated
    stage; margin, kl_final and kl_250 are stored with tests/golden/tsne_fit_<n>.npz (tools/gen_tsne_golden.py)."""
    from si_mamba_amd import TSNE
    from si_mamba_amd.manifold import tsne
    X, y = tsne_ref.blobs(n, d, k, 0)
    g = load_golden(f"tsne_fit_{n}")
    Xd = _dev(X, device)
    model = TSNE(perplexity=perp, max_iter=400)
    Y = _np(model.fit_transform(Xd))
    assert Y.shape == (n, 2) and Y.dtype == F32 and np.isfinite(Y).all()
    assert model.n_iter_ == 400 and model.learning_rate_ == 50.0
    acc = tsne_ref.knn1_accuracy(Y, y)
    # the KL of the returned embedding, recomputed in float64 from the very P the fit used
    cond, _ = tsne.calibrate(tsne.squared_distances(Xd), perp)
    P = _np(tsne.joint_probabilities(cond)[0])
    kl64, kl32 = float(tsne_ref.grad_kl(P, Y, 1.0, F64)[0]), float(tsne_ref.grad_kl(P, Y, 1.0, F32)[0])
    print(f"tsne-fit n{n}: kl {model.kl_divergence_:.6f} host {kl64:.6f} reference {float(g['kl_final']):.6f} "
          f"margin {float(g['margin']):.3e} kl_250 {float(g['kl_250']):.6f} accuracy {acc:.4f}")
    assert acc == 1.0
    assert abs(model.kl_divergence_ - kl64) <= tsne_ref.bound(kl32, kl64)
    assert model.kl_divergence_ <= float(g["kl_final"]) * (1.0 + float(g["margin"]))
    assert model.kl_divergence_ < float(g["kl_250"])


# ---- stop rule, repeatability ----------------------------------------------------------------------------------------
def test_min_grad_norm_stops_at_the_first_check(device):
    from si_mamba_amd import TSNE
    from si_mamba_amd.manifold import tsne
    X, _ = tsne_ref.blobs(96, 8, 3, 0)
    model = TSNE(perplexity=10.0, max_iter=400, min_grad_norm=1e9).fit(_dev(X, device))
    assert model.n_iter_ == 50
    assert model.status_[tsne.ST_STOPPED] == 1.0 and model.status_[tsne.ST_ITERS] == 50.0
    assert model.status_[tsne.ST_GRAD_NORM] > 0.0
    assert np.isfinite(model.kl_divergence_) and bool(torch.isfinite(model.embedding_).all())


def test_two_fits_give_the_same_bits(device):
    from si_mamba_amd import TSNE
    X, _ = tsne_ref.blobs(333, 16, 5, 0)
    Xd = _dev(X, device)
    a = TSNE(max_iter=300).fit(Xd)
    b = TSNE(max_iter=300).fit(Xd.clone())
    assert same_bits(a.embedding_, b.embedding_)
    assert a.kl_divergence_ == b.kl_divergence_ and a.status_ == b.status_ and a.n_iter_ == 300
    c = TSNE(max_iter=300, init="random", random_state=3).fit(Xd)
    d = TSNE(max_iter=300, init="random", random_state=3).fit(Xd)
    assert same_bits(c.embedding_, d.embedding_) and not same_bits(a.embedding_, c.embedding_)
    e = TSNE(max_iter=300, init=a.embedding_.clone()).fit(Xd.bfloat16())
    assert bool(torch.isfinite(e.embedding_).all())


# ---- memory contract -------------------------------------------------------------------------------------------------
def _contract(run, inputs, device):
    """tests/test_gpu_memory_contract.py's rule for one op: guard bands intact, and the plain run and the runs under two
    poisons agree bit for bit."""
    plain = run(*[t.to(device) for t in inputs])
    torch.cuda.synchronize()
    got = []
    for poison in (ZERO, SENTINEL):
        with guarded(poison) as g:
            ins = [place(t.to(device)) for t in inputs]
            out = run(*ins)
            torch.cuda.synchronize()
            g.verify()
            assert len(g.records) > len(ins), "the op allocated nothing through the harness"
            assert "tsne.py" in g.modules
        got.append(out)
    for i, (a, b, p) in enumerate(zip(got[0], got[1], plain)):
        assert bool(torch.isfinite(p).all()), i
        assert same_bits(a, b), f"returned tensor {i} differs between the two poisons"
        assert same_bits(a, p), f"returned tensor {i} differs between the poisoned and the plain run"


def test_memory_contract_calibrate(device):
    from si_mamba_amd.manifold import tsne
    d2 = torch.from_numpy(_cal_d2(333, "plain").copy())
    _contract(lambda d: tsne.calibrate(d, 30.0), [d2], device)


def test_memory_contract_gradient(device):
    from si_mamba_amd.manifold import tsne
    _, _, P = _problem(333)
    Y = torch.randn(333, 2, generator=torch.Generator().manual_seed(1)) * 3
    _contract(lambda p, y: tsne.gradient(p, y, 12.0), [torch.from_numpy(P.copy()), Y], device)


def test_memory_contract_run(device):
    from si_mamba_amd.manifold import tsne
    P, lr, (Y, update, gains) = _settled(333)
    s = torch.tensor([tsne_ref.sum_plogp(P)], dtype=torch.float64)

    def run(p, y, u, g, s):
        # the state is updated in place: every run starts from the same, in buffers of the harness
        y, u, g = (torch.empty_like(t).copy_(t) for t in (y, u, g))
        status = tsne.new_status(p.device, 40)
        tsne.run(p, y, u, g, status, s, 40, 65, exaggeration=1.0, momentum=0.8, learning_rate=lr)   # checks at 50, 100
        return y, u, g, status
    ins = [torch.from_numpy(P.copy())] + [torch.from_numpy(a.copy()) for a in (Y, update, gains)] + [s]
    _contract(run, ins, device)


def test_memory_contract_whole_fit(device):
    from si_mamba_amd import TSNE
    X, _ = tsne_ref.blobs(257, 8, 4, 0)

    def run(x):
        m = TSNE(max_iter=250).fit(x)
        return (m.embedding_,)
    _contract(run, [torch.from_numpy(X)], device)


# ---- PointMamba(return_features=True) --------------------------------------------------------------------------------
def test_return_features(device):
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    cfg = default_config(trans_dim=64, encoder_dims=64, depth=2, num_group=32, group_size=16, cls_dim=5, drop_path=0.,
                         knn_graph=8)
    m = PointMamba(cfg).to(device).eval()
    pts = clouds(4, 256, 20).to(device)
    seen = []
    hook = m.cls_head_finetune.register_forward_hook(lambda mod, args, out: seen.append(args[0].detach().clone()))
    with torch.no_grad():
        plain = m(pts)
        logits, feats = m(pts, return_features=True)
        gt = torch.zeros(4, dtype=torch.long, device=device)
        plain_l, plain_p = m(pts, gt)
        l3, p3, f3 = m(pts, gt, return_features=True)
    hook.remove()
    assert isinstance(plain, torch.Tensor) and plain.shape == (4, 5)
    assert feats.shape == (4, 64) and same_bits(feats, seen[1]) and same_bits(f3, seen[3])
    assert same_bits(logits, plain) and same_bits(l3, plain_l) and same_bits(p3, plain_p) and same_bits(l3, plain)
