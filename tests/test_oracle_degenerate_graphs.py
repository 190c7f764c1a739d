"""CPU: the table of tests/degenerate_graphs.py against float64, and its checker end to end without a device.

  * every literal of ROWS (gap, cluster size, parity columns) and of INADMISSIBLE is re-derived from the float64 spectrum;
  * the structure each case is there for is present: multiplicities, component counts, tau == 0 runs, lambda_min < -2;
  * ``check_eigenpairs`` passes every row for a stand-in solver -- LAPACK's float32 eigh of the same fp32 matrix, its k
    selected pairs, signs flipped to the convention, orders from a stable argsort.  So every bound holds for a plain fp32
    solve: the bounds rest on the reference, not on the kernels;
  * three planted defects are each caught.
"""
import numpy as np
import pytest
import torch

import degenerate_graphs as dg
from oracle.gen_golden import SPECTRAL_COMBOS


def _float64(case, G, msym):
    S64, w, V = dg.reference(dg.laplacian32(dg.adjacency(case, G)[None], msym))
    return S64[0], w[0].numpy(), V[0]


def _multiplicity(w, tol=1e-9):
    """per eigenvalue, how many eigenvalues (itself included) lie within tol"""
    return (np.abs(w[:, None] - w[None, :]) <= tol).sum(1)


def standin(S32, G, mode):
    """float32 LAPACK on the fp32 matrix -> (vals (B,k), vecs (B,G,k), order (B,k,G)) in the kernels' conventions"""
    w, V = torch.linalg.eigh(S32)
    sel = dg.selected_indices(G, mode)
    vals, vecs = w[:, sel].contiguous(), V[:, :, sel].contiguous()
    vecs = vecs * dg.convention_sign(vecs)
    order = torch.sort(vecs.transpose(1, 2), dim=2, stable=True)[1]
    return vals, vecs, order


# ---- the table --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", dg.SIZES)
def test_rows_match_float64(G):
    for mname, mode in dg.MODES.items():
        listed = dg.ROWS.get((G, mname), {})
        bad = dg.INADMISSIBLE.get((G, mname), {})
        if mode.k == 4:                                     # the k = 4 modes walk every case at every size
            assert set(listed) | set(bad) == set(dg.CASES) and not set(listed) & set(bad), (G, mname)
        for case in list(listed) + list(bad):
            _, w, _ = _float64(case, G, mode.msym)
            sel = dg.selected_indices(G, mode)
            idx, gap = dg.cluster_of(w, sel)
            if case in bad:
                assert gap < dg.MIN_GAP and gap == pytest.approx(bad[case], rel=1e-2), (G, mname, case, gap)
                continue
            rgap, rsize, parity = listed[case]
            assert gap >= dg.MIN_GAP, (G, mname, case, gap)
            assert idx.size == rsize, (G, mname, case, idx.size)
            assert (np.isinf(gap) and np.isinf(rgap)) or gap == pytest.approx(rgap, rel=1e-3), (G, mname, case, gap)
            if parity:
                assert gap >= dg.PARITY_GAP and all(dg.alone(w, sel[i]) for i in parity), (G, mname, case)


def test_path_rows_carry_order_parity():
    for G in (64, 128):
        assert dg.ROWS[(G, "rw_small")]["path"][2] == (1, 2, 3)


def test_k7_rows():
    k7 = [(G, c) for (G, m), d in dg.ROWS.items() if m == "rw_small_k7" for c in d]
    assert len(k7) == 2
    assert any(G <= 128 for G, _ in k7) and any(G > 128 for G, _ in k7)      # forced and native large kernel


def test_every_route_has_a_cluster_larger_than_k():
    for sizes in (dg.SIZES_SMALL, dg.SIZES_LARGE):                           # Jacobi / tridiagonal / forced; native
        assert any(size > dg.MODES[m].k for (G, m), d in dg.ROWS.items() if G in sizes for _, size, _ in d.values())


# ---- what each case is there for -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", dg.SIZES)
def test_structures_present(G):
    # ring: a circulant's eigenvalues come in pairs (j, G - j); alone are j = 0 and, G even, j = G / 2
    _, w, _ = _float64("ring", G, False)
    assert (_multiplicity(w) >= 2).sum() >= G - 2
    # path: already tridiagonal -- every reflector is skipped -- and every eigenvalue simple
    S64, w, _ = _float64("path", G, False)
    zt = dg.zero_taus(S64)
    assert len(zt) == G - 2 and all(zt)
    assert np.diff(w).min() > dg.CLUSTER_TOL
    # complete: one (G-1)-fold eigenvalue
    _, w, _ = _float64("complete", G, False)
    assert w[-1] - w[1] < 1e-6 and w[1] - w[0] > 1.0
    # two_rings: two components; equal rings (G even) make every eigenvalue but 0 and the two at j = n / 2 four-fold
    _, w, _ = _float64("two_rings", G, False)
    assert (np.abs(w) < 1e-6).sum() == 2
    if G % 2 == 0:
        assert (_multiplicity(w) >= 4).sum() >= G - 4
    # ring_path_ring: three components (counted on the symmetric Laplacian: the mirrored rw matrix of a chain is not
    # semi-definite and has no zero of its own), and every (tau_{k-1}, tau_k) zero / non-zero transition
    _, w, _ = _float64("ring_path_ring", G, True)
    assert (np.abs(w) < 1e-6).sum() == 3
    S64, w, _ = _float64("ring_path_ring", G, False)
    assert (np.abs(w) < 1e-6).sum() >= 2
    zt = dg.zero_taus(S64)
    assert dg.tau_transitions(zt) == {(False, False), (False, True), (True, False), (True, True)}
    first_zero = zt.index(True)
    assert not any(zt[:first_zero]) and not all(zt[first_zero:])              # tau != 0, then == 0, then != 0 again
    # lattice: what a regular cloud produces -- the tie rule picks the edges (6th and 7th neighbour equally far), the
    # Laplacian is dense (no reflector skipped)
    p = dg.grid_points(G)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1).sort(dim=1)[0]
    assert (d2[:, 6] == d2[:, 7]).sum() > G // 2
    S64, w, _ = _float64("lattice", G, False)
    assert not any(dg.zero_taus(S64))
    # stars: spectrum of the mirrored lower triangle far outside [-1, 3]
    for case in ("star", "double_star"):
        _, w, _ = _float64(case, G, False)
        assert w[0] < -2.0 and w[-1] > 3.0, (case, w[0], w[-1])
    _, w, _ = _float64("star", G, False)
    assert w[0] == pytest.approx(1 - np.sqrt(G - 1), abs=1e-4)


# ---- the checker, end to end ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,mname", sorted(dg.ROWS))
def test_standin_solver_passes_every_row(G, mname):
    mode = dg.MODES[mname]
    names, adj = dg.batch(G, mname)
    S32 = dg.laplacian32(adj, mode.msym)
    vals, vecs, order = standin(S32, G, mode)
    parity = [dg.ROWS[(G, mname)][n][2] for n in names]
    got = dg.check_eigenpairs(S32.double(), vals, vecs, order, G, mode, parity=parity, tag=f"standin G={G} {mname}")
    for n, m in zip(names, got):
        print(f"G={G} {mname} {n}: " + " ".join(f"{k}={v:.2e}" if isinstance(v, float) else f"{k}={v}"
                                                 for k, v in m.items()))
        assert m["cluster"] == dg.ROWS[(G, mname)][n][1]
        if dg.ROWS[(G, mname)][n][2]:
            assert "parity_hits" in m


def _row(G, mname, case):
    mode = dg.MODES[mname]
    S32 = dg.laplacian32(dg.adjacency(case, G)[None], mode.msym)
    return mode, S32, standin(S32, G, mode)


def test_planted_vector_outside_the_cluster_is_caught():
    """one eigenvector replaced by ANOTHER vector of the same cluster plus 1e-3 of a vector outside it: still unit
    length and orthogonal to the other three within 1e-6, still inside every eigenvalue bound"""
    G, mname, case = 64, "sym_small", "complete"            # 63-fold cluster, gap 1.016
    mode, S32, (vals, vecs, order) = _row(G, mname, case)
    S64, w, V = dg.reference(S32)
    dg.check_eigenpairs(S64, vals, vecs, order, G, mode)    # passes as it stands
    idx, gap = dg.cluster_of(w[0].numpy(), dg.selected_indices(G, mode))
    P = V[0][:, idx]
    inside = P[:, 10] - vecs[0].double() @ (vecs[0].double().T @ P[:, 10])   # in the cluster, orthogonal to the returned
    inside = inside / inside.norm()
    outside = V[0][:, 0]
    planted = inside + 1e-3 * outside
    bad = vecs.clone()
    bad[0, :, 2] = (planted / planted.norm()).float()
    bad = bad * dg.convention_sign(bad)
    bad_order = torch.sort(bad.transpose(1, 2), dim=2, stable=True)[1]
    assert (bad[0].T @ bad[0] - torch.eye(4)).abs().max() < 5e-6
    with pytest.raises(AssertionError, match="residual|subspace"):
        dg.check_eigenpairs(S64, vals, bad, bad_order, G, mode)
    # the subspace bound alone sees it too: leakage 1e-3 x gap 1.016 against 2e-5
    v = bad[0, :, 2].double()
    assert (v - P @ (P.T @ v)).norm() * gap > 40 * dg.LEAK_TOL


def test_swapped_eigenvalues_are_caught():
    G, mname, case = 64, "rw_small", "path"
    mode, S32, (vals, vecs, order) = _row(G, mname, case)
    dg.check_eigenpairs(S32.double(), vals, vecs, order, G, mode)
    bad = vals.clone()
    bad[0, 1], bad[0, 2] = vals[0, 2], vals[0, 1]
    with pytest.raises(AssertionError, match="eigenvalue error"):
        dg.check_eigenpairs(S32.double(), bad, vecs, order, G, mode)


def test_repeated_index_in_an_order_is_caught():
    G, mname, case = 63, "rw_small", "ring"
    mode, S32, (vals, vecs, order) = _row(G, mname, case)
    dg.check_eigenpairs(S32.double(), vals, vecs, order, G, mode)
    bad = order.clone()
    bad[0, 3, 17] = bad[0, 3, 16]
    with pytest.raises(AssertionError, match="not a permutation"):
        dg.check_eigenpairs(S32.double(), vals, vecs, bad, G, mode)


# ---- the clouds of the route from centres -----------------------------------------------------------------------------------
def test_dyadic_clouds_are_distinct_tied_and_admissible():
    mode = dg.MODES["rw_small"]
    for name, c in dg.dyadic_clouds().items():
        G = c.shape[1]
        assert torch.equal(c * 8, (c * 8).round()) and len({tuple(q) for q in c[0].tolist()}) == G, name
        d2 = ((c.double().unsqueeze(2) - c.double().unsqueeze(1)) ** 2).sum(-1)[0].sort(dim=1)[0]
        for cb in SPECTRAL_COMBOS:
            # the tie rule decides edges: rows whose knn-th and (knn+1)-th neighbours are equally far
            assert (d2[:, cb["knn"]] == d2[:, cb["knn"] + 1]).sum() > 0, (name, cb["tag"])
            adj = dg.knn_adjacency_ref(c, cb["knn"], cb["alpha"], cb["symmetric"], cb["self_loop"], cb["binary"])
            S32 = dg.laplacian32(adj, False)
            vals, vecs, order = standin(S32, G, mode)
            dg.check_eigenpairs(S32.double(), vals, vecs, order, G, mode, tag=f"{name} {cb['tag']}")
