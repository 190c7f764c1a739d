"""GPU: the Chamfer kernels on ragged batches and with pytorch3d's other arguments (simamba_chamfer_ragged_*,
mae.chamfer_distance's keywords, the pytorch3d stand-in), against a float64 brute force written here and against the
project's own fixed-length call.

The yardstick is the one of tests/test_gpu_chamfer_large.py with a norm switch and lengths: the fp32 inputs cast to
double, every distance from direct differences on the host, only the real points of every pair, the arg-min the lowest
index among exact minima.  Bounds (derived, not fitted):
  * distances, relative 2e-6.  L2: three fp32 differences, three products and two adds, below 6 * 2^-24 = 3.6e-7; L1:
    three differences and two adds, below 5 * 2^-24 = 3e-7; the minimum of perturbed values inherits it, the fixed-order
    fp64 sum and its rounding to fp32 add < 1e-7, a weight one more rounding (2^-24);
  * indices: equal to the float64 arg-min wherever best and second best differ by more than relative 1e-5 (at most 1 %
    of the real queries may be left out, asserted and printed);
  * gradients, max|got - want| / max|want| <= 1e-5: each term is a difference of fp32 coordinates (L2) or a sign (L1)
    times a coefficient of a few roundings, and a point's K reverse matches are added in fp32 in ascending order, each
    add rounding by at most 2^-24 of a partial sum no larger than the result's scale: K * 2^-24 in all.  So the bound
    can be derived only where K stays small: the gradient cases (GRAD_LENGTHS) use the padded shapes with lengths that
    keep the two sets of a pair within a factor of 8 of each other, and grad_case asserts K <= 100 (6e-6, which leaves
    4e-6 for the other roundings).  A single point against thousands -- pair (2050, 1) of the fourth case, where one
    point sums 2050 equal L1 terms -- measures 1.9e-5 and is outside that derivation, like the (2, 1, 257) that
    tests/test_gpu_chamfer_large.py leaves out of its gradients; such pairs stay in every other test here, the
    bit-for-bit ones included.  The gradient seeds are ones the brute force shows free of near-ties for both norms
    and both directions (asserted), since float64 autograd follows its own arg-min;
  * integer lattice {0..15}^3: every distance (L2 <= 675, L1 <= 45), every sum (< 2^24) and every gradient with
    power-of-two coefficients is exact in fp32, and a mean over a power-of-two length divides exactly: equality.
Everywhere: rows behind a length are 0 (index 0, gradient 0), whatever the buffers or the padding held.
"""
import functools
import sys

import pytest
import torch

from helpers import clouds_from, max_scaled, relerr
from si_mamba_amd import _lib

pytestmark = pytest.mark.gpu

# Padded shapes (P, n, m): the boundaries are 64 (the small route), 256 * Q queries per workgroup, 1024 targets per tile.
CASES = [(8, 70, 33), (8, 300, 1030), (8, 1025, 2049), (4, 2050, 1100), (8, 1, 257)]
# Lengths from 1 to the padded size, both ends included, through 256 / 257 / 1024 / 1025 where they fit; x ascending and
# y mostly descending, so that long sets meet short ones, with one pair of full length on both sides in the third case.
LENGTHS = [([1, 11, 20, 31, 40, 49, 61, 70], [33, 28, 24, 19, 15, 10, 6, 1]),
           ([1, 44, 86, 129, 256, 257, 299, 300], [1030, 1025, 1024, 736, 257, 256, 148, 1]),
           ([1, 256, 257, 439, 586, 731, 1024, 1025], [1, 1025, 1024, 1463, 257, 256, 586, 2049]),
           ([1, 1024, 1025, 2050], [1100, 257, 256, 1]),
           ([1] * 8, [257, 256, 221, 147, 110, 74, 37, 1])]
# The gradient cases: the same padded shapes ((8, 257, 1) in place of (8, 1, 257)), lengths through the same boundaries
# but within a factor of 8 inside a pair, so that no point collects more than a handful of reverse matches (docstring).
GRAD_SHAPES = [(8, 70, 33), (8, 300, 1030), (8, 1025, 2049), (4, 2050, 1100), (8, 257, 1)]
GRAD_LENGTHS = [([1, 4, 20, 31, 40, 49, 61, 70], [1, 28, 24, 19, 15, 10, 33, 32]),
                ([20, 44, 86, 129, 256, 257, 299, 300], [60, 148, 256, 257, 736, 1024, 1025, 1030]),
                ([256, 257, 439, 586, 731, 1024, 1025, 1025], [586, 256, 1024, 1463, 257, 1025, 2049, 2048]),
                ([1024, 1025, 2050, 513], [1100, 257, 256, 1024]),
                ([1, 2, 5, 9, 17, 33, 65, 96], [1] * 8)]
GRAD_SEED = [100, 101, 101, 101, 100]                         # free of near-ties at these lengths (grad_case asserts it)
MAX_REVERSE_MATCHES = 100
BIG = 1 << 30
REDUCTIONS = {"mean": 0, "sum": 1, None: 2}


@functools.lru_cache(maxsize=None)
def case(k):
    """(x (P,n,3), y (P,m,3), nx (P,), ny (P,)) of CASES[k]: generator seeds 11 .. 15."""
    P, n, m = CASES[k]
    gen = torch.Generator().manual_seed(11 + k)
    x, y = clouds_from(P, n, gen), clouds_from(P, m, gen)
    nx, ny = torch.tensor(LENGTHS[k][0]), torch.tensor(LENGTHS[k][1])
    assert nx.shape == ny.shape == (P,) and 1 <= int(nx.min()) and int(nx.max()) <= n and int(ny.max()) <= m
    return x, y, nx, ny


# ---- the float64 brute force ---------------------------------------------------------------------------------------
def rho64(q, t, norm):
    """q (a,3), t (b,3) float64 -> (a,b): direct differences."""
    dx, dy, dz = (q[:, None, c] - t[None, :, c] for c in range(3))
    return dx * dx + dy * dy + dz * dz if norm == 2 else dx.abs() + dy.abs() + dz.abs()


def nearest64(q, t, norm, chunk=512):
    """One pair, real points only: (best (a,), lowest index among exact minima (a,), second best (a,))."""
    q, t = q.double(), t.double()
    a, ar = q.shape[0], torch.arange(t.shape[0])
    best, idx, second = torch.empty(a, dtype=torch.float64), torch.empty(a, dtype=torch.int64), \
        torch.empty(a, dtype=torch.float64)
    for r0 in range(0, a, chunk):
        d = rho64(q[r0:r0 + chunk], t, norm)
        mn = d.min(-1)[0]
        am = torch.where(d == mn[:, None], ar, BIG).min(-1)[0]
        d[torch.arange(d.shape[0]), am] = float("inf")
        best[r0:r0 + chunk], idx[r0:r0 + chunk], second[r0:r0 + chunk] = mn, am, d.min(-1)[0]
    return best, idx, second


def reference(x, y, nx, ny, norm):
    """Per-point distances and indices of every pair at its lengths; zeros (second best: inf) behind them."""
    P, n, m = x.shape[0], x.shape[1], y.shape[1]
    r = dict(d1=torch.zeros(P, n, dtype=torch.float64), d2=torch.zeros(P, m, dtype=torch.float64),
             idx1=torch.zeros(P, n, dtype=torch.int64), idx2=torch.zeros(P, m, dtype=torch.int64),
             second1=torch.full((P, n), float("inf"), dtype=torch.float64),
             second2=torch.full((P, m), float("inf"), dtype=torch.float64))
    for p in range(P):
        a, b = int(nx[p]), int(ny[p])
        r["d1"][p, :a], r["idx1"][p, :a], r["second1"][p, :a] = nearest64(x[p, :a], y[p, :b], norm)
        r["d2"][p, :b], r["idx2"][p, :b], r["second2"][p, :b] = nearest64(y[p, :b], x[p, :a], norm)
    r["real1"] = torch.arange(n)[None] < nx[:, None]
    r["real2"] = torch.arange(m)[None] < ny[:, None]
    return r


@functools.lru_cache(maxsize=None)
def case_reference(k, norm):
    return reference(*case(k), norm)


def want_dist(ref, nx, ny, reduction, one_way, w=None):
    """float64 (P,) for mean / sum, (cham_x, cham_y or None) for None."""
    w = torch.ones(len(nx), dtype=torch.float64) if w is None else w.double()
    cx, cy = ref["d1"] * w[:, None], ref["d2"] * w[:, None]
    if reduction is None:
        return cx, (None if one_way else cy)
    sx, sy = cx.sum(1), cy.sum(1)
    if reduction == "mean":
        sx, sy = sx / nx, sy / ny
    return sx if one_way else sx + sy


def undecided(ref, k):
    """Real queries whose best and second-best float64 distances are within relative 1e-5 (one target: inf)."""
    best, second = ref[f"d{k}"], ref[f"second{k}"]
    return torch.isfinite(second) & ~((second - best) > 1e-5 * second)


# ---- the entry points ----------------------------------------------------------------------------------------------
def lens32(t, device):
    return None if t is None else t.to(device=device, dtype=torch.int32)


def run_raw(x, y, nx, ny, device, norm=2, reduction="mean", one_way=False, queries=0, up=None):
    """simamba_chamfer_ragged_fwd and, with ``up`` (ddist (P,), or (dd1, dd2) without a reduction), _bwd.  Every output
    starts from NaN / -1, so what a call leaves unwritten shows.  Everything comes back on the host."""
    lib = _lib.load()
    xd, yd = x.to(device).contiguous(), y.to(device).contiguous()
    P, n, m = x.shape[0], x.shape[1], y.shape[1]
    lx, ly = lens32(nx, device), lens32(ny, device)
    nan = float("nan")
    o = dict(dist=torch.full((P,), nan, device=device), d1=torch.full((P, n), nan, device=device),
             d2=torch.full((P, m), nan, device=device),
             idx1=torch.full((P, n), -1, device=device, dtype=torch.int32),
             idx2=torch.full((P, m), -1, device=device, dtype=torch.int32))
    red = REDUCTIONS[reduction]
    dist = None if reduction is None else o["dist"]
    i2, d2 = (None, None) if one_way else (o["idx2"], o["d2"])
    rc = lib.simamba_chamfer_ragged_fwd(xd.data_ptr(), yd.data_ptr(), _lib.ptr(lx), _lib.ptr(ly), _lib.ptr(dist),
                                        o["idx1"].data_ptr(), _lib.ptr(i2), o["d1"].data_ptr(), _lib.ptr(d2), P, n, m,
                                        norm, red, int(one_way), queries, _lib.stream_ptr(device))
    assert rc == 0, rc
    if up is not None:
        o["dx"], o["dy"] = torch.full_like(xd, nan), torch.full_like(yd, nan)
        if reduction is None:
            dd, dd1, dd2 = None, up[0].to(device).contiguous(), (None if one_way else up[1].to(device).contiguous())
        else:
            dd, dd1, dd2 = up.to(device).contiguous(), None, None
        rc = lib.simamba_chamfer_ragged_bwd(xd.data_ptr(), yd.data_ptr(), _lib.ptr(lx), _lib.ptr(ly), _lib.ptr(dd),
                                            _lib.ptr(dd1), _lib.ptr(dd2), o["idx1"].data_ptr(), _lib.ptr(i2),
                                            o["dx"].data_ptr(), o["dy"].data_ptr(), P, n, m, norm, red, int(one_way),
                                            queries, _lib.stream_ptr(device))
        assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def run_plain(x, y, device, up=None):
    """The fixed-length entry points simamba_chamfer_large_fwd / _bwd on whole sets."""
    lib = _lib.load()
    xd, yd = x.to(device).contiguous(), y.to(device).contiguous()
    P, n, m = x.shape[0], x.shape[1], y.shape[1]
    o = dict(dist=torch.empty(P, device=device), d1=torch.empty(P, n, device=device),
             d2=torch.empty(P, m, device=device), idx1=torch.empty(P, n, device=device, dtype=torch.int32),
             idx2=torch.empty(P, m, device=device, dtype=torch.int32))
    rc = lib.simamba_chamfer_large_fwd(xd.data_ptr(), yd.data_ptr(), o["dist"].data_ptr(), o["idx1"].data_ptr(),
                                       o["idx2"].data_ptr(), o["d1"].data_ptr(), o["d2"].data_ptr(), P, n, m,
                                       _lib.stream_ptr(device))
    assert rc == 0, rc
    if up is not None:
        o["dx"], o["dy"] = torch.empty_like(xd), torch.empty_like(yd)
        rc = lib.simamba_chamfer_large_bwd(xd.data_ptr(), yd.data_ptr(), up.to(device).data_ptr(),
                                           o["idx1"].data_ptr(), o["idx2"].data_ptr(), o["dx"].data_ptr(),
                                           o["dy"].data_ptr(), P, n, m, _lib.stream_ptr(device))
        assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def upstream(P, seed):
    return torch.rand(P, generator=torch.Generator().manual_seed(seed)) + 0.5


PER_POINT = dict(d1="real1", idx1="real1", dx="real1", d2="real2", idx2="real2", dy="real2")


def assert_zero_behind(got, nx, ny, keys):
    n, m = got["d1"].shape[1], got["d2"].shape[1]
    behind = dict(real1=torch.arange(n)[None] >= nx[:, None], real2=torch.arange(m)[None] >= ny[:, None])
    for k in keys:
        rows = got[k][behind[PER_POINT[k]]]
        assert bool((rows == 0).all()), k                    # NaN or -1: never written; anything else: a wrong value


def python_call(x, y, nx, ny, device, w=None, grad=False, **kw):
    from si_mamba_amd.mae import chamfer_distance
    xd, yd = x.to(device).requires_grad_(grad), y.to(device).requires_grad_(grad)
    wd = None if w is None else w.to(device).requires_grad_(grad)
    out = chamfer_distance(xd, yd, x_lengths=None if nx is None else nx.to(device),
                           y_lengths=None if ny is None else ny.to(device), weights=wd, **kw)
    return out, xd, yd, wd


# ---- 1: every pair alone -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def alone(k, device):
    """The plain fixed-length call on every pair at its true lengths: a list of per-pair results."""
    x, y, nx, ny = case(k)
    g = upstream(x.shape[0], 200 + k)
    return [run_plain(x[p:p + 1, :int(nx[p])], y[p:p + 1, :int(ny[p])], device, up=g[p:p + 1])
            for p in range(x.shape[0])]


@pytest.mark.parametrize("queries", [1, 2, 4])
@pytest.mark.parametrize("k", range(len(CASES)))
def test_every_pair_is_what_it_returns_alone(k, queries, device):
    x, y, nx, ny = case(k)
    got = run_raw(x, y, nx, ny, device, queries=queries, up=upstream(x.shape[0], 200 + k))
    for p, want in enumerate(alone(k, device)):
        a, b = int(nx[p]), int(ny[p])
        assert torch.equal(got["dist"][p:p + 1], want["dist"]), p
        for key, ln in (("d1", a), ("idx1", a), ("dx", a), ("d2", b), ("idx2", b), ("dy", b)):
            assert torch.equal(got[key][p, :ln], want[key][0]), (p, key)
    assert_zero_behind(got, nx, ny, PER_POINT)


# ---- 2: full lengths and no lengths are the plain call -------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CASES)))
def test_full_and_absent_lengths_equal_the_plain_entry_points(k, device):
    x, y, _, _ = case(k)
    P, n, m = CASES[k]
    g = upstream(P, 300 + k)
    want = run_plain(x, y, device, up=g)
    full_x, full_y = torch.full((P,), n), torch.full((P,), m)
    for nx, ny in ((None, None), (full_x, full_y), (full_x, None), (None, full_y)):
        got = run_raw(x, y, nx, ny, device, up=g)
        for key in want:
            assert torch.equal(got[key], want[key]), (key, nx is None, ny is None)


def test_default_python_call_keeps_its_routes(device):
    from si_mamba_amd.mae import chamfer_distance
    gen = torch.Generator().manual_seed(7)
    x, y = clouds_from(5, 32, gen).to(device), clouds_from(5, 32, gen).to(device)
    _lib.counters.clear()
    small = chamfer_distance(x.clone().requires_grad_(), y)
    assert _lib.counters == {"chamfer_small": 1}
    _lib.counters.clear()
    same = chamfer_distance(x, y, x_lengths=None, y_lengths=None, weights=None, norm=2, point_reduction="mean",
                            single_directional=False)
    assert _lib.counters == {"chamfer_small": 1} and torch.equal(same, small.detach())
    _lib.counters.clear()
    chamfer_distance(x, y.clone().requires_grad_())
    assert _lib.counters == {"chamfer_large": 1}
    _lib.counters.clear()
    tiled = chamfer_distance(x, y, x_lengths=torch.full((5,), 32, device=device))       # any new argument: tiled
    assert _lib.counters == {"chamfer_ragged": 1}
    assert relerr(tiled.cpu(), small.detach().cpu().double()) <= 2e-6


# ---- 3: float64 brute force ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_way", [False, True], ids=["both", "one_way"])
@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("k", range(len(CASES)))
def test_distances_and_indices_against_float64(k, norm, one_way, device):
    x, y, nx, ny = case(k)
    ref = case_reference(k, norm)
    dirs = (1,) if one_way else (1, 2)
    got = run_raw(x, y, nx, ny, device, norm=norm, reduction=None, one_way=one_way)
    assert torch.isnan(got["dist"]).all()                    # no reduction: dist is not written
    if one_way:
        assert torch.isnan(got["d2"]).all() and bool((got["idx2"] == -1).all())
    for d in dirs:
        real = ref[f"real{d}"]
        e = relerr(got[f"d{d}"][real], ref[f"d{d}"][real])
        skip = undecided(ref, d)[real]
        share = float(skip.double().mean())
        print(CASES[k], f"norm {norm} d{d}: {e:.2e}; idx{d}: undecided share {share:.2e}")
        assert e <= 2e-6, e
        assert share <= 0.01, share
        assert torch.equal(got[f"idx{d}"].long()[real][~skip], ref[f"idx{d}"][real][~skip])
        limit = (ny if d == 1 else nx)[:, None].expand_as(real)
        assert bool((got[f"idx{d}"][real] >= 0).all()) and bool((got[f"idx{d}"].long()[real] < limit[real]).all())
    assert_zero_behind(got, nx, ny, [f"{a}{d}" for d in dirs for a in ("d", "idx")])

    w = upstream(len(nx), 400 + k)
    for reduction in ("mean", "sum", None):
        for wt in (None, w):
            out, *_ = python_call(x, y, nx, ny, device, w=wt, norm=norm, point_reduction=reduction,
                                  single_directional=one_way)
            want = want_dist(ref, nx, ny, reduction, one_way, wt)
            if reduction is not None:
                e = relerr(out.cpu(), want)
                print(CASES[k], f"norm {norm} {reduction} weights {wt is not None}: {e:.2e}")
                assert out.shape == (len(nx),) and e <= 2e-6, (reduction, e)
                continue
            assert isinstance(out, tuple) and len(out) == 2 and (out[1] is None) == one_way
            for d in dirs:
                real, o = ref[f"real{d}"], out[d - 1].cpu()
                assert relerr(o[real], want[d - 1][real]) <= 2e-6
                assert bool((o[~real] == 0).all())


def autograd64(x, y, nx, ny, norm, reduction, one_way, w, up, device):
    """float64 autograd of the composed form, pair by pair on its real points, on the device: (dx, dy, dw)."""
    xd, yd = x.double().to(device).requires_grad_(), y.double().to(device).requires_grad_()
    wd = w.double().to(device).requires_grad_()
    up = [u.double().to(device) for u in up]
    total = 0.0
    for p in range(x.shape[0]):
        a, b = int(nx[p]), int(ny[p])
        diff = xd[p, :a, None] - yd[p, None, :b]
        d = (diff * diff).sum(-1) if norm == 2 else diff.abs().sum(-1)
        cx, cy = d.min(1)[0] * wd[p], d.min(0)[0] * wd[p]
        if reduction is None:
            total = total + (cx * up[0][p, :a]).sum() + (0.0 if one_way else (cy * up[1][p, :b]).sum())
            continue
        sx, sy = cx.sum(), cy.sum()
        if reduction == "mean":
            sx, sy = sx / a, sy / b
        total = total + up[0][p] * (sx if one_way else sx + sy)
    return tuple(t.cpu() for t in torch.autograd.grad(total, (xd, yd, wd)))


@functools.lru_cache(maxsize=None)
def grad_case(k):
    """Clouds of a seed without near-ties, GRAD_SHAPES[k] at GRAD_LENGTHS[k]."""
    P, n, m = GRAD_SHAPES[k]
    gen = torch.Generator().manual_seed(GRAD_SEED[k])
    x, y = clouds_from(P, n, gen), clouds_from(P, m, gen)
    nx, ny = torch.tensor(GRAD_LENGTHS[k][0]), torch.tensor(GRAD_LENGTHS[k][1])
    for norm in (1, 2):
        ref = reference(x, y, nx, ny, norm)
        assert not undecided(ref, 1).any() and not undecided(ref, 2).any(), "seed has a near-tie: pick another"
        for d, size in ((1, m), (2, n)):
            real = ref[f"real{d}"]
            most = max(int(torch.bincount(ref[f"idx{d}"][p][real[p]], minlength=size).max()) for p in range(P))
            assert most <= MAX_REVERSE_MATCHES, (k, norm, d, most)
    return x, y, nx, ny


@pytest.mark.parametrize("one_way", [False, True], ids=["both", "one_way"])
@pytest.mark.parametrize("reduction", ["mean", "sum", None])
@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("k", range(len(GRAD_SHAPES)))
def test_gradients_against_float64_autograd(k, norm, reduction, one_way, device):
    x, y, nx, ny = grad_case(k)
    P, n, m = x.shape[0], x.shape[1], y.shape[1]
    gen = torch.Generator().manual_seed(500 + k)
    w = torch.rand(P, generator=gen) + 0.5
    up = [torch.rand(P, n, generator=gen) + 0.5, torch.rand(P, m, generator=gen) + 0.5] if reduction is None \
        else [torch.rand(P, generator=gen) + 0.5]
    want = autograd64(x, y, nx, ny, norm, reduction, one_way, w, up, device)
    out, xd, yd, wd = python_call(x, y, nx, ny, device, w=w, grad=True, norm=norm, point_reduction=reduction,
                                  single_directional=one_way)
    if reduction is None:
        loss = (out[0] * up[0].to(device)).sum() + (0.0 if one_way else (out[1] * up[1].to(device)).sum())
    else:
        loss = (out * up[0].to(device)).sum()
    loss.backward()
    errs = {name: max_scaled(t.grad, wt) for name, t, wt in zip(("dx", "dy", "dw"), (xd, yd, wd), want)}
    print((P, n, m), f"norm {norm} {reduction} one_way {one_way}:", {a: f"{b:.2e}" for a, b in errs.items()})
    assert all(e <= 1e-5 for e in errs.values()), errs
    got = dict(d1=xd.grad.abs().sum(-1).cpu(), d2=yd.grad.abs().sum(-1).cpu())
    assert_zero_behind(got, nx, ny, ("d1", "d2"))
    assert torch.isfinite(xd.grad).all() and torch.isfinite(yd.grad).all()


# ---- 4: exact arithmetic -------------------------------------------------------------------------------------------
def fixed_match_grad64(x, y, nx, ny, ref, norm, k1, k2, one_way):
    """The chain rule through the reference's matches, float64: k1 (P,n), k2 (P,m) are the per-point coefficients."""
    x, y = x.double(), y.double()
    dx, dy = torch.zeros_like(x), torch.zeros_like(y)

    def term(a, b):
        return 2 * (a - b) if norm == 2 else torch.sign(a - b)

    for p in range(x.shape[0]):
        a, b = int(nx[p]), int(ny[p])
        i1, i2 = ref["idx1"][p, :a], ref["idx2"][p, :b]
        t1 = k1[p, :a, None] * term(x[p, :a], y[p, i1])          # d1[i] against x_i and y[idx1[i]]
        dx[p, :a] += t1
        dy[p].index_add_(0, i1, -t1)
        if not one_way:
            t2 = k2[p, :b, None] * term(y[p, :b], x[p, i2])
            dy[p, :b] += t2
            dx[p].index_add_(0, i2, -t2)
    return dx, dy


LATTICE = (4, 2100, 2050)
# powers of two for the exact mean; the duplicates below (y[1030], x[1029]) are real in pairs 0, 3 (y) and 1 (x) only
LATTICE_LENGTHS = ([256, 2048, 512, 64], [2048, 1024, 256, 2048])


@functools.lru_cache(maxsize=None)
def lattice():
    """Integer points with duplicated targets on both sides of the tile boundary (y[1030] = y[5], x[1029] = x[3]), a
    query on top of each (x[0] = y[5], y[0] = x[3]: both copies at distance 0) and, behind every length, copies of the
    other set's points: a kernel that read them would report distance 0 there."""
    P, n, m = LATTICE
    gen = torch.Generator().manual_seed(40)
    x = torch.randint(0, 16, (P, n, 3), generator=gen).float()
    y = torch.randint(0, 16, (P, m, 3), generator=gen).float()
    y[:, 1030] = y[:, 5]
    x[:, 1029] = x[:, 3]
    x[:, 0] = y[:, 5]
    y[:, 0] = x[:, 3]
    nx, ny = torch.tensor(LATTICE_LENGTHS[0]), torch.tensor(LATTICE_LENGTHS[1])
    for p in range(P):
        a, b = int(nx[p]), int(ny[p])
        x[p, a:] = y[p, torch.arange(n - a) % b]
        y[p, b:] = x[p, torch.arange(m - b) % a]
    return x, y, nx, ny


@pytest.mark.parametrize("one_way", [False, True], ids=["both", "one_way"])
@pytest.mark.parametrize("norm", [1, 2])
def test_integer_lattice_is_exact(norm, one_way, device):
    x, y, nx, ny = lattice()
    P, n, m = LATTICE
    ref = reference(x, y, nx, ny, norm)
    g = torch.tensor([1.0, 2.0, 0.5, 4.0])
    dirs = (1,) if one_way else (1, 2)
    for reduction in ("sum", "mean"):
        got = run_raw(x, y, nx, ny, device, norm=norm, reduction=reduction, one_way=one_way, up=g)
        for d in dirs:
            assert torch.equal(got[f"d{d}"], ref[f"d{d}"].float()), (reduction, d)
            assert torch.equal(got[f"idx{d}"].long(), ref[f"idx{d}"]), (reduction, d)
        assert torch.equal(got["dist"], want_dist(ref, nx, ny, reduction, one_way).float()), reduction
        k1, k2 = g[:, None].double().expand(P, n), g[:, None].double().expand(P, m)
        if reduction == "mean":
            k1, k2 = k1 / nx[:, None], k2 / ny[:, None]
        wdx, wdy = fixed_match_grad64(x, y, nx, ny, ref, norm, k1, k2, one_way)
        assert torch.equal(got["dx"], wdx.float()) and torch.equal(got["dy"], wdy.float()), reduction
    # per-point coefficients, powers of two
    u1 = torch.tensor([0.5, 1.0, 2.0])[torch.arange(n) % 3].expand(P, n).contiguous()
    u2 = torch.tensor([4.0, 0.25])[torch.arange(m) % 2].expand(P, m).contiguous()
    got = run_raw(x, y, nx, ny, device, norm=norm, reduction=None, one_way=one_way, up=(u1, u2))
    wdx, wdy = fixed_match_grad64(x, y, nx, ny, ref, norm, u1.double(), u2.double(), one_way)
    assert torch.equal(got["dx"], wdx.float()) and torch.equal(got["dy"], wdy.float())
    # the duplicates: the lower index, and never one behind a length
    for p in range(P):
        if ny[p] > 1030:                                     # both copies are real and at distance 0 from x[p, 0]
            assert ref["d1"][p, 0] == 0 and int(got["idx1"][p, 0]) == int(ref["idx1"][p, 0]) <= 5
        if nx[p] > 1029 and not one_way:
            assert ref["d2"][p, 0] == 0 and int(got["idx2"][p, 0]) == int(ref["idx2"][p, 0]) <= 3
    assert int((ny > 1030).sum()) > 0 and int((nx > 1029).sum()) > 0
    assert not bool((got["idx1"] == 1030).any()) and bool((got["idx1"].long() < ny[:, None]).all())
    if not one_way:
        assert not bool((got["idx2"] == 1029).any()) and bool((got["idx2"].long() < nx[:, None]).all())


# ---- 5: the padding is never read ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [float("nan"), float("inf"), 1e30])
@pytest.mark.parametrize("k", [1, 3])
def test_padding_is_never_read(k, fill, device):
    x, y, nx, ny = case(k)
    P, n, m = CASES[k]
    real1, real2 = torch.arange(n)[None] < nx[:, None], torch.arange(m)[None] < ny[:, None]
    zx, zy = x * real1[..., None], y * real2[..., None]
    fx, fy = torch.where(real1[..., None], x, torch.tensor(fill)), torch.where(real2[..., None], y, torch.tensor(fill))
    g = upstream(P, 600 + k)
    gen = torch.Generator().manual_seed(601 + k)
    pp = (torch.rand(P, n, generator=gen) + 0.5, torch.rand(P, m, generator=gen) + 0.5)
    for norm in (1, 2):
        for reduction, up in (("mean", g), ("sum", g), (None, pp)):
            for one_way in (False, True):
                want = run_raw(zx, zy, nx, ny, device, norm=norm, reduction=reduction, one_way=one_way, up=up)
                got = run_raw(fx, fy, nx, ny, device, norm=norm, reduction=reduction, one_way=one_way, up=up)
                keys = ["d1", "idx1", "dx", "dy"] + ([] if one_way else ["d2", "idx2"]) \
                    + ([] if reduction is None else ["dist"])
                for key in keys:
                    assert torch.equal(got[key], want[key]), (norm, reduction, one_way, key)
                    assert torch.isfinite(got[key].float()).all(), (norm, reduction, one_way, key)


# ---- 6: lengths of any integer dtype, clamped ----------------------------------------------------------------------
def test_length_dtypes_and_clamping(device):
    from si_mamba_amd.mae import chamfer_distance
    x, y, nx, ny = case(1)
    P, n, m = CASES[1]
    xd, yd = x.to(device), y.to(device)

    def run(lx, ly):
        a, b = xd.clone().requires_grad_(), yd.clone().requires_grad_()
        cx, cy = chamfer_distance(a, b, x_lengths=lx.to(device), y_lengths=ly.to(device), point_reduction=None)
        (cx.sum() + 2 * cy.sum()).backward()
        return cx.detach(), cy.detach(), a.grad, b.grad

    want = run(nx.to(torch.int32), ny.to(torch.int32))
    for dt in (torch.int16, torch.int64):
        for g, w in zip(run(nx.to(dt), ny.to(dt)), want):
            assert torch.equal(g, w), dt
    # out of range: as if clamped into [1, n] and [1, m]
    wild_x = torch.tensor([0, -5, n + 7, 1 << 40, -(1 << 40), n, 1, (1 << 32) + 5])
    wild_y = torch.tensor([m + 1, 0, -1, 3, 1 << 31, -(1 << 31), (1 << 33) + 2, m])
    want = run(wild_x.clamp(1, n), wild_y.clamp(1, m))
    for g, w in zip(run(wild_x, wild_y), want):
        assert torch.equal(g, w)
    for g, w in zip(run(wild_x.clamp(-30000, 30000).to(torch.int16), wild_y.clamp(-30000, 30000).to(torch.int16)),
                    want):
        assert torch.equal(g, w)


# ---- 7: the pytorch3d stand-in -------------------------------------------------------------------------------------
def test_stand_in_takes_pytorch3d_argument_forms(device):
    from si_mamba_amd.shim import install_shim
    names = ("mamba_ssm", "causal_conv1d", "pytorch3d")
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in names}
    try:
        install_shim(force=True, pytorch3d=True)
        from pytorch3d.loss import chamfer_distance
        k = 1
        x, y, nx, ny = case(k)
        P = len(nx)
        xd, yd, lx, ly = x.to(device), y.to(device), nx.to(device), ny.to(device)
        w = upstream(P, 700)
        for norm in (1, 2):
            ref = case_reference(k, norm)
            for one_way in (False, True):
                for point in ("mean", "sum"):
                    for wt in (None, w, torch.zeros(P)):
                        per = want_dist(ref, nx, ny, point, one_way, wt)
                        wants = {None: per, "sum": per.sum(),
                                 "mean": per.sum() / (P if wt is None else wt.double().sum().clamp_min(1e-300))}
                        for batch, want in wants.items():
                            loss, normals = chamfer_distance(xd, yd, x_lengths=lx, y_lengths=ly, norm=norm,
                                                             weights=None if wt is None else wt.to(device),
                                                             batch_reduction=batch, point_reduction=point,
                                                             single_directional=one_way)
                            assert normals is None and loss.shape == (() if batch else (P,))
                            if wt is not None and not wt.any():
                                assert bool((loss == 0).all()), (batch, point)          # all-zero weights: 0
                            else:
                                assert relerr(loss.cpu(), want) <= 2e-6, (norm, one_way, point, batch)
                out, normals = chamfer_distance(xd, yd, x_lengths=lx, y_lengths=ly, norm=norm, batch_reduction=None,
                                                point_reduction=None, single_directional=one_way)
                if one_way:
                    assert torch.is_tensor(out)                                          # (cham_x, None)
                    cx, cy = out, None
                else:
                    assert isinstance(out, tuple) and len(out) == 2                      # ((cham_x, cham_y), None)
                    cx, cy = out
                assert normals is None and cx.shape == x.shape[:2]
                assert relerr(cx.cpu()[ref["real1"]], ref["d1"][ref["real1"]]) <= 2e-6
                if not one_way:
                    assert cy.shape == y.shape[:2]
                    assert relerr(cy.cpu()[ref["real2"]], ref["d2"][ref["real2"]]) <= 2e-6
        # the mean over the batch with weights is differentiable through the weights and never reads them on the host
        wd = w.to(device).requires_grad_()
        loss, _ = chamfer_distance(xd, yd, x_lengths=lx, y_lengths=ly, weights=wd)
        loss.backward()
        assert torch.isfinite(wd.grad).all() and bool((wd.grad != 0).any())
        with pytest.raises(ValueError):
            chamfer_distance(xd, yd, point_reduction=None)                               # batch_reduction="mean"
        with pytest.raises(NotImplementedError, match="normals"):
            chamfer_distance(xd, yd, x_normals=xd)
    finally:
        for key in [key for key in sys.modules if key.split(".")[0] in names]:
            del sys.modules[key]
        sys.modules.update(saved)


# ---- 8: one capture ------------------------------------------------------------------------------------------------
def test_forward_and_backward_in_one_captured_graph(device):
    from si_mamba_amd.mae import chamfer_distance
    x, y, nx, ny = case(1)
    P = len(nx)
    g = upstream(P, 800).to(device)
    others = (nx.flip(0).contiguous(), ny.flip(0).contiguous())

    def step(a, b, lx, ly):
        d = chamfer_distance(a, b, x_lengths=lx, y_lengths=ly)
        return (d,) + torch.autograd.grad(d, (a, b), g)

    xd, yd = x.to(device).requires_grad_(), y.to(device).requires_grad_()
    eager = [[t.clone() for t in step(xd, yd, lx.to(device), ly.to(device))] for lx, ly in ((nx, ny), others)]
    static_x, static_y = x.to(device).requires_grad_(), y.to(device).requires_grad_()
    static_lx, static_ly = nx.to(device), ny.to(device)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        step(static_x, static_y, static_lx, static_ly)                   # warm-up off the default stream
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(static_x, static_y, static_lx, static_ly)
    for (lx, ly), want in zip(((nx, ny), others), eager):
        static_lx.copy_(lx.to(device))
        static_ly.copy_(ly.to(device))
        graph.replay()
        torch.cuda.synchronize(device)
        for o, w in zip(out, want):
            assert torch.equal(o, w)
    assert not torch.equal(eager[0][0], eager[1][0])                     # the two length sets do differ
