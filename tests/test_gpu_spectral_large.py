"""GPU parity of the large-G spectral kernels (128 < G <= 512, csrc/spectral_large.hip): k-NN graph, top-k Laplacian
eigenpairs and orders against the oracle and against the reference's own function bodies.

The fixtures (tools/pin_large_groups.py) carry no adjacency arrays: at G = 512 they would not fit the size limit of a
committed file.  The adjacency is recomputed from the fixture's centres with oracle.spectral_ref, which
tests/test_oracle_pinned.py holds to the reference's own graph at G <= 128.  Both fixture families share their
centres, so the adjacency tests run on the oracle family only; every eigenpair / order test runs on both.

Tolerances: the eigensolver works in fp32 on the G x G matrix, and the rounding error of the Householder reduction
grows with G (each entry is touched by G reflectors).  The bounds the G <= 128 tests state at 2e-5
(tests/test_gpu_spectral.py) are scaled by G / 128 here.

Order parity uses the mask of tests/test_gpu_spectral.py (exact wherever both neighbouring sorted entries are further
apart than 4x the measured eigenvector error, at least 4e-6) with its non-vacuity guard: 90 % of the positions must
pass the mask up to G = 256.  A unit 512-vector has neighbour gaps about 8x smaller than a 128-vector while the
solver error stays ~1e-6, so on the G = 512 surface fixture only 87-94 % of the positions clear even the 4e-6 floor,
whatever the solver (a property of the fixture, computed from the oracle's vectors alone); the one-sided knn = 8 graph
("asym") has the smallest spectral gaps and so the largest measured error, and 81 % of its positions pass the mask.
The guard is 0.8 at G = 512.
The bar on the exact fraction over ALL positions (> 97 %) is the same at every G.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import spectral_ref as sr
from oracle.gen_golden import SPECTRAL_COMBOS, unit_ball_centers
from test_gpu_spectral import align_sign

pytestmark = pytest.mark.gpu

OWN = ["spectral_g256", "spectral_g512_surface"]
FIXTURES = OWN + ["ref_" + n for n in OWN]


def _tol(G):
    return 2e-5 * G / 128


def assert_order_matches_oracle(order, sgn, wvecs, worder, err, tag):
    """tests/test_gpu_spectral.py's check of the kernel's order against the oracle's (see there), with the
    non-vacuity guard of the module docstring; returns (hits, total) over all positions."""
    G = order.shape[-1]
    wk = wvecs * sgn
    want = torch.sort(wk.transpose(1, 2), dim=2, stable=True)[1]
    same = (sgn.squeeze(1) > 0)
    assert torch.equal(want[same], worder[same]), tag
    wsorted = torch.gather(wk.transpose(1, 2), 2, want)
    d = wsorted[..., 1:] - wsorted[..., :-1]
    one = torch.full_like(wsorted[..., :1], 1.0)
    gapl, gapr = torch.cat([one, d], -1), torch.cat([d, one], -1)
    tau = 4.0 * err[:, :, None].clamp_min(1e-6)
    safe = (gapl > tau) & (gapr > tau)
    assert safe.float().mean() > (0.9 if G <= 256 else 0.8), (tag, safe.float().mean().item())
    assert torch.equal(order[safe], want[safe]), tag
    return (order == want).sum().item(), order.numel()


def _adj(centers, cb):
    return sr.create_graph_from_feature_space(centers, cb["knn"], cb["alpha"], cb["symmetric"], cb["self_loop"],
                                              cb["binary"])


def _lam_gap(all_vals, k=4):
    """distance of each of the k smallest eigenvalues to its nearest neighbour in the spectrum"""
    d = (all_vals[:, 1:k + 1] - all_vals[:, 0:k]).abs()
    left = torch.cat([torch.full((all_vals.shape[0], 1), 1.0), (all_vals[:, 1:k] - all_vals[:, 0:k - 1]).abs()], 1)
    return torch.minimum(d, left)


def _residual(adj_cpu, vals, vecs, msym=False):
    """max |S v - lambda v| against the float64 mirrored lower triangle the kernel decomposes"""
    A = adj_cpu.double()
    L = sr.sym_laplacian(A) if msym else sr.rw_laplacian(A)
    S = sr.eigh_lower(L)
    v = vecs.double().cpu()
    return (S @ v - v * vals.double().cpu()[:, None, :]).abs().max().item()


@pytest.mark.parametrize("name", OWN)
def test_graph_adjacency_large(name, device):
    from si_mamba_amd import spectral
    g = load_golden(name)
    c = torch.from_numpy(g["centers"])
    assert c.shape[1] > 128
    for cb in SPECTRAL_COMBOS:
        got = spectral.create_graph_from_feature_space_gpu_weighted_adjacency(
            c.to(device), cb["knn"], cb["alpha"], cb["symmetric"], cb["self_loop"], cb["binary"]).cpu().numpy()
        want = _adj(c, cb).numpy()
        np.testing.assert_array_equal(got != 0, want != 0)                  # same edges, exactly
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=0)            # device expf vs libm (<= 2 ulp apart)
    # create_graph_from_centers: the sigma = mean-distance branch (alpha == 0) and the weighted form
    got = spectral.create_graph_from_centers(c.to(device), 10, 0.0, True, True, False).cpu().numpy()
    want = sr.create_graph_from_centers(c, 10, 0.0, True, True, False).numpy()
    np.testing.assert_array_equal(got != 0, want != 0)
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=0)
    got = spectral.create_graph_from_centers(c.to(device), 10, 10.0, True, True, False).cpu().numpy()
    want = sr.create_graph_from_centers(c, 10, 10.0, True, True, False, self_alpha=10.0).numpy()
    np.testing.assert_array_equal(got != 0, want != 0)
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=0)


@pytest.mark.parametrize("name", FIXTURES)
def test_eigenpairs_and_orders_large(name, device):
    from si_mamba_amd import _lib, spectral
    g = load_golden(name)
    c = torch.from_numpy(g["centers"])
    G = c.shape[1]
    tol = _tol(G)
    hit = tot = 0
    before = _lib.counters.get("spectral_large_g", 0)
    for cb in SPECTRAL_COMBOS:
        t = cb["tag"]
        adj = _adj(c, cb)
        vals, vecs, _, _, order = spectral._eig(adj.to(device), 4, True, False, want_all=False, want_order=True)
        np.testing.assert_allclose(vals.cpu().numpy(), g[f"{t}.vals"], atol=tol)
        wvecs = torch.from_numpy(g[f"{t}.vecs"])
        gv, sgn = align_sign(vecs.cpu(), wvecs)
        err = (gv - wvecs).abs().amax(dim=1)
        assert (err * _lam_gap(torch.from_numpy(g[f"{t}.all_vals"]))).max() < tol, (t, err.max().item())
        assert (vecs.transpose(1, 2) @ vecs - torch.eye(4, device=device)).abs().max() < tol
        assert _residual(adj, vals, vecs) < tol, t
        # (1) the order IS the stable argsort of the kernel's own eigenvectors; (2) the oracle's order away from ties
        for i in range(4):
            assert torch.equal(order[:, i], spectral.argsort_rows(vecs[:, :, i].contiguous())), t
        h, n = assert_order_matches_oracle(order.cpu(), sgn, wvecs, torch.from_numpy(g[f"{t}.order"]), err, t)
        hit += h
        tot += n
    assert _lib.counters.get("spectral_large_g", 0) == before + len(SPECTRAL_COMBOS)
    print(f"{name}: exact order positions {hit}/{tot}")
    assert hit / tot > 0.97, (hit, tot)


@pytest.mark.parametrize("name", FIXTURES)
def test_symmetric_and_largest_modes_large(name, device):
    from si_mamba_amd import spectral
    g = load_golden(name)
    c = torch.from_numpy(g["centers"])
    tol = _tol(c.shape[1])
    adj = _adj(c, SPECTRAL_COMBOS[0])
    v, e, _, _, _ = spectral._eig(adj.to(device), 4, True, True, want_all=False)       # MATRIX_SYM: first pair dropped
    np.testing.assert_allclose(v.cpu().numpy(), g["hardest.sym.vals"], atol=tol)
    assert _residual(adj, v, e, msym=True) < tol
    v, e, _, _, _ = spectral._eig(adj.to(device), 4, False, False, want_all=False)     # largest
    np.testing.assert_allclose(v.cpu().numpy(), g["hardest.largest.vals"], atol=tol)
    assert _residual(adj, v, e) < tol
    assert (v[:, 1:] <= v[:, :-1]).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_spectral_order_from_centres_large(name, device):
    """The fused call the models make (centres -> graph -> large-G top-k -> argsort) against the golden orders."""
    from si_mamba_amd import spectral
    g = load_golden(name)
    c = torch.from_numpy(g["centers"]).to(device)
    tol = _tol(c.shape[1])
    hit = tot = 0
    for cb in SPECTRAL_COMBOS:
        t = cb["tag"]
        vals, vecs, order = spectral.spectral_order(c, cb["knn"], cb["alpha"], 4, smallest=True,
                                                    symmetric=cb["symmetric"], self_loop=cb["self_loop"],
                                                    binary=cb["binary"])
        np.testing.assert_allclose(vals.cpu().numpy(), g[f"{t}.vals"], atol=tol)
        wvecs = torch.from_numpy(g[f"{t}.vecs"])
        gv, sgn = align_sign(vecs.cpu(), wvecs)
        err = (gv - wvecs).abs().amax(dim=1)
        h, n = assert_order_matches_oracle(order.cpu(), sgn, wvecs, torch.from_numpy(g[f"{t}.order"]), err, t)
        hit += h
        tot += n
    assert hit / tot > 0.97, (hit, tot)


@pytest.mark.parametrize("name", ["spectral_g64", "spectral_g128", "spectral_g128_surface"])
def test_forced_large_kernel_agrees_with_tridiagonal_kernel(name, device):
    """The large-G kernel forced at G <= 128 (_lib.spectral_large_g) against the LDS-resident tridiagonal kernel the
    library runs there, on the existing fixtures: same spectrum, same vectors within solver error, same orders away
    from near-ties."""
    from si_mamba_amd import _lib, spectral
    g = load_golden(name)
    for cb in SPECTRAL_COMBOS:
        t = cb["tag"]
        adj = torch.from_numpy(g[f"{t}.adj"]).to(device)
        v0, e0, _, _, o0 = spectral._eig(adj, 4, True, False, want_all=False, want_order=True)
        before = _lib.counters.get("spectral_large_g", 0)
        with _lib.spectral_large_g():
            v1, e1, _, _, o1 = spectral._eig(adj, 4, True, False, want_all=False, want_order=True)
        assert _lib.counters.get("spectral_large_g", 0) == before + 1
        assert (v1 - v0).abs().max() < 2e-5, t
        lam_gap = _lam_gap(torch.from_numpy(g[f"{t}.all_vals"])).to(device)
        assert ((e1 - e0).abs().amax(dim=1) * lam_gap).max() < 2e-5, t
        wvecs = torch.from_numpy(g[f"{t}.vecs"])
        gv, sgn = align_sign(e1.cpu(), wvecs)
        err = (gv - wvecs).abs().amax(dim=1)
        assert_order_matches_oracle(o1.cpu(), sgn, wvecs, torch.from_numpy(g[f"{t}.order"]), err, t)
        # the two kernels use the same sign convention: their orders agree wherever the vectors are not near-tied
        sv = torch.gather(e0.transpose(1, 2), 2, o0)
        d = sv[..., 1:] - sv[..., :-1]
        one = torch.ones_like(sv[..., :1])
        safe = (torch.cat([one, d], -1) > 1e-4) & (torch.cat([d, one], -1) > 1e-4)
        assert torch.equal(o1[safe], o0[safe]), t
    adj = torch.from_numpy(g["hardest.adj"]).to(device)
    with _lib.spectral_large_g():
        v, _, _, _, _ = spectral._eig(adj, 4, True, True, want_all=False)
    np.testing.assert_allclose(v.cpu().numpy(), g["hardest.sym.vals"], atol=2e-5)


# (G, forced large kernel): a single reflector, an odd G, a Gershgorin reduction that crosses one wave and the full
# pitch on both kernels; the first size above the LDS limit and a G that is no multiple of 64 on the large kernel.
SHARED_STEP_CASES = [(3, False), (5, False), (65, False), (128, False), (3, True), (5, True), (65, True), (128, True),
                     (129, True), (200, True)]
SHARED_STEP_SEED = 0     # float64 spectra of these clouds: selected eigenvalues at least 2.4e-3 apart (checked on CPU)


@pytest.mark.parametrize("G,large", SHARED_STEP_CASES)
def test_shared_solver_steps_small_and_full_width(G, large, device):
    """The solver steps both eigen kernels share are parametrised by pitch, thread count and the number of extracted
    pairs; every other test runs k = 4.  Here: k = min(8, G) smallest (all eight waves, both inverse-iteration batches
    of the large kernel) and k = min(7, G - 1) MATRIX_SYM (eight extracted, first dropped), on a weighted symmetric
    graph, at the module's bound.  No eigenvector parity with the oracle: at k = 8 the gaps of a random cloud are not
    controlled, and residual and orthogonality do not depend on them."""
    import contextlib
    from si_mamba_amd import _lib, spectral
    tol = 2e-5 * max(1, G / 128)
    c = unit_ball_centers(2, G, SHARED_STEP_SEED)
    adj = sr.create_graph_from_feature_space(c, min(8, G - 1), 10.0, True, False, False)
    for k, msym in [(min(8, G), False), (min(7, G - 1), True)]:
        skip = 1 if msym else 0
        S = sr.eigh_lower(sr.sym_laplacian(adj.double()) if msym else sr.rw_laplacian(adj.double()))
        want = torch.linalg.eigh(S)[0][:, skip:skip + k]
        before = _lib.counters.get("spectral_large_g", 0)
        with (_lib.spectral_large_g() if large and G <= 128 else contextlib.nullcontext()):
            vals, vecs, _, _, order = spectral._eig(adj.to(device), k, True, msym, want_all=False, want_order=True)
        assert _lib.counters.get("spectral_large_g", 0) == before + (1 if large else 0)
        err = (vals.double().cpu() - want).abs().max().item()
        res = _residual(adj, vals, vecs, msym=msym)
        orth = (vecs.transpose(1, 2) @ vecs - torch.eye(k, device=device)).abs().max().item()
        print(f"G={G} large={large} k={k} msym={msym}: eigenvalue err {err:.2e} residual {res:.2e} orth {orth:.2e}")
        assert err < tol and res < tol and orth < tol, (k, msym, err, res, orth)
        for i in range(k):
            assert torch.equal(order[:, i], spectral.argsort_rows(vecs[:, :, i].contiguous())), (k, msym, i)


def test_full_batch_large(device):
    """(B = 64, G = 512): solver invariants of the k pairs without an oracle (no full spectrum at this size)."""
    from si_mamba_amd import spectral
    B, G, k = 64, 512, 4
    c = unit_ball_centers(B, G, 11).to(device)
    vals, vecs, order = spectral.spectral_order(c, 20, 10.0, k, smallest=True, symmetric=True, self_loop=False,
                                                binary=True)
    assert torch.isfinite(vals).all() and torch.isfinite(vecs).all()
    assert (vals[:, 1:] >= vals[:, :-1]).all()
    assert (vecs.transpose(1, 2) @ vecs - torch.eye(k, device=device)).abs().max() < _tol(G)
    adj = spectral.create_graph_from_feature_space_gpu_weighted_adjacency(c, 20, 10.0, True, False, True)
    assert torch.equal(adj, adj.transpose(1, 2)) and (adj.sum(-1) >= 20).all()
    assert _residual(adj.cpu(), vals, vecs) < _tol(G)
    # each order is a permutation that sorts its eigenvector
    assert torch.equal(order.sort(dim=2)[0], torch.arange(G, device=device).expand(B, k, G))
    sv = torch.gather(vecs.transpose(1, 2), 2, order)
    assert (sv[..., 1:] >= sv[..., :-1]).all()


def test_full_spectrum_refused_above_128(device):
    from si_mamba_amd import spectral
    adj = torch.zeros(1, 256, 256, device=device)
    with pytest.raises(NotImplementedError, match="spectral_order"):
        spectral.calc_top_k_eigenvalues_eigenvectors(adj, 4, True)
    with pytest.raises(NotImplementedError, match="top-k route"):
        spectral.calc_top_k_eigenvalues_eigenvectors_symmetric(adj, 4, True)
    with pytest.raises(RuntimeError, match="simamba_laplacian_topk_ex"):
        spectral._eig(torch.zeros(1, 513, 513, device=device), 4, True, False, want_all=False)
