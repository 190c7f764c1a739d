"""Graphs with degenerate spectra, and the one checker of an eigen-ordering result on them.

TEST INFRASTRUCTURE (shared by test_oracle_degenerate_graphs.py, CPU, and test_gpu_spectral_degenerate.py).  Every other
spectral test runs on k-NN graphs of random or FPS-sampled clouds, whose spectra are simple and whose Laplacians are
dense: every Householder reflector of the top-k kernels has tau != 0, no eigenvalue repeats, and the spectrum of the
mirrored lower triangle stays far inside [-1, 3].  The adjacencies here are built from integers and have, by
construction, repeated eigenvalues (ring, complete, two_rings, lattice), Laplacians that are tridiagonal already or
block-diagonal (path, two_rings, ring_path_ring: tau == 0) and spectra far outside [-1, 3] (star, double_star).

Inside a repeated eigenvalue the individual eigenvectors are not defined, only their span is.  So nothing here compares
vector with vector.  ``check_eigenpairs`` holds a result to the float64 decomposition of THE SAME fp32 matrix by what is
defined: eigenvalues, residuals, orthonormality, the distance of every returned vector from the float64 invariant
subspace of its cluster (times the cluster's gap: the Davis-Kahan form of the suite's ``err * gap`` bar), the sign
convention, and the orders.

  cluster   the selected eigenvalues, extended to the transitive closure of "within CLUSTER_TOL of a member"
  gap       distance of the cluster to the rest of the float64 spectrum; a row is admissible iff gap >= MIN_GAP
  ROWS      {(G, mode): {case: (gap, cluster size, parity columns)}} -- literals; test_oracle_degenerate_graphs.py
            re-derives every one of them.  A case missing from a (G, mode) entry is inadmissible there (see INADMISSIBLE).
  parity    the columns i of a row on which the order is also held against the float64 vector's own order
            (test_gpu_spectral.assert_order_matches_oracle): eigenvalue i alone in its CLUSTER_TOL-component and the
            row's gap >= PARITY_GAP, and the 90 % guard of that function holds, with room, for the float64 vector
            at three times the error of a float32 LAPACK solve (so the flags rest on the reference, not the kernels).

No GPU code runs here.
"""
import collections

import numpy as np
import torch

from oracle import spectral_ref as sr

CLUSTER_TOL = 1e-4
MIN_GAP = 3e-4
PARITY_GAP = 1e-3
SIZES_SMALL = (63, 64, 127, 128)          # the three G <= 128 routes; odd: the Jacobi tournament's dummy, `tid < G` tails
SIZES_LARGE = (160, 255)                  # the large kernel, natively
SIZES = SIZES_SMALL + SIZES_LARGE

Mode = collections.namedtuple("Mode", "smallest msym k")
MODES = {"rw_small": Mode(True, False, 4), "sym_small": Mode(True, True, 4), "rw_large": Mode(False, False, 4),
         "rw_small_k7": Mode(True, False, 7)}     # k = 7: the second inverse-iteration batch of the large kernel


# ---- adjacencies (integers only) -----------------------------------------------------------------------------------
def ring(n, reach):
    a = torch.zeros(n, n)
    i = torch.arange(n)
    for d in range(1, reach + 1):
        a[i, (i + d) % n] = 1.0
        a[i, (i - d) % n] = 1.0
    return a


def path(n, first=40):
    """Chain with the integer edge weights first, first + 1, ...  Any chain has a tridiagonal Laplacian (tau == 0 at
    every reflector) and simple eigenvalues.  With EQUAL weights the mirrored lower triangle is the same up to its last
    row read forwards and backwards, so the entries of every low eigenvector pair up within 1e-6 (sin x = sin(pi - x))
    and the order-parity guard, which wants 90 % of a vector's sorted neighbours apart, cannot hold (2 % for vector 1
    at G = 128).  Rising weights break the mirror and spread the low eigenvalues (1.8e-3 apart at G = 128 against
    3e-4): an fp32 solver's vector error, which goes with one over that distance and widens the guard's mask, then
    leaves the guard room for vectors 1..3 at every G <= 128.  A steeper rise localises the vectors (entries near
    zero tie again), a flatter one closes the eigenvalues up."""
    a = torch.zeros(n, n)
    i = torch.arange(n - 1)
    a[i, i + 1] = a[i + 1, i] = (first + i).float()
    return a


def complete(n):
    return torch.ones(n, n) - torch.eye(n)


def two_rings(n):
    return torch.block_diag(ring(n // 2, 2), ring(n - n // 2, 2))


def ring_path_ring(n):
    a = n // 3
    return torch.block_diag(ring(a, 2), path(a), ring(n - 2 * a, 2))


def grid_points(n):
    """the first n sites of the 4 x 4 x ceil(n / 16) integer grid (z fastest varying last: index = 16 z + 4 y + x)"""
    nz = -(-n // 16)
    z, y, x = torch.meshgrid(torch.arange(nz), torch.arange(4), torch.arange(4), indexing="ij")
    return torch.stack([x.flatten(), y.flatten(), z.flatten()], 1)[:n]


def lattice(n, knn=6):
    """symmetric 6-NN graph of the grid: every node's 6 nearest others by (squared distance, index), both directions"""
    p = grid_points(n)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)                      # int64, exact
    nn = torch.sort(d2, dim=1, stable=True)[1][:, 1:knn + 1]                 # ties to the lower index; [0] is the node
    a = torch.zeros(n, n)
    rows = torch.arange(n)[:, None].expand(-1, knn)
    a[rows, nn] = 1.0
    a[nn, rows] = 1.0
    return a


def star(n, hubs=1):
    a = torch.zeros(n, n)
    a[:hubs, :] = 1.0
    a[:, :hubs] = 1.0
    a.fill_diagonal_(0.0)
    return a


def double_star(n):
    return star(n, 2)


CASES = {"ring": lambda n: ring(n, 3), "path": path, "complete": complete, "two_rings": two_rings,
         "ring_path_ring": ring_path_ring, "lattice": lattice, "star": star, "double_star": double_star}


def adjacency(case, G):
    return CASES[case](G)


# ---- the float64 reference --------------------------------------------------------------------------------------------
def laplacian32(adj, msym):
    """(B,G,G) fp32 adjacency -> the fp32 matrix eigh(UPLO='L') decomposes, formed with the oracle's ops"""
    return sr.eigh_lower(sr.sym_laplacian(adj) if msym else sr.rw_laplacian(adj))


def selected_indices(G, mode):
    """ascending-spectrum indices of the k selected eigenvalues, in output order (MATRIX_SYM drops the first)"""
    skip = 1 if mode.msym else 0
    if mode.smallest:
        return list(range(skip, skip + mode.k))
    return [G - 1 - skip - i for i in range(mode.k)]


def cluster_of(w, sel):
    """w (G,) ascending float64, sel: indices -> (sorted member indices of the closure, gap to the rest)"""
    G = w.shape[0]
    member = np.zeros(G, bool)
    member[list(sel)] = True
    grown = True
    while grown:                                        # the spectrum is sorted: the closure grows over neighbours
        grown = False
        for i in range(G - 1):
            if member[i] != member[i + 1] and abs(w[i + 1] - w[i]) <= CLUSTER_TOL:
                member[i] = member[i + 1] = True
                grown = True
    idx = np.nonzero(member)[0]
    rest = w[~member]
    gap = float("inf") if rest.size == 0 else float(np.abs(w[idx][:, None] - rest[None, :]).min())
    return idx, gap


def alone(w, i):
    """eigenvalue i has no other eigenvalue within CLUSTER_TOL"""
    d = np.abs(w - w[i])
    d[i] = np.inf
    return bool(d.min() > CLUSTER_TOL)


def reference(S32):
    """(B,G,G) fp32 -> (S64, w64 (B,G), V64 (B,G,G)): float64 eigh of the widened fp32 matrix"""
    S64 = S32.double()
    w, V = torch.linalg.eigh(S64)
    return S64, w, V


def zero_taus(S64):
    """The reflectors the top-k kernels skip: Householder tridiagonalisation of one (G,G) float64 matrix with the
    kernels' rule (csrc/spectral_device.h, householder_params) -> list of G - 2 booleans, True where tau == 0."""
    S = torch.as_tensor(S64, dtype=torch.float64).clone().numpy()
    G = S.shape[0]
    out = []
    for k in range(G - 2):
        x = S[k + 1:, k].copy()
        nrm2, x0 = float(x @ x), float(x[0])
        rest = nrm2 - x0 * x0
        if not (rest > 1e-30 and rest > 1e-12 * nrm2):
            out.append(True)
            continue
        out.append(False)
        beta = -np.copysign(np.sqrt(nrm2), x0)
        tau = (beta - x0) / beta
        v = x / (x0 - beta)
        v[0] = 1.0
        S22 = S[k + 1:, k + 1:]
        p = tau * (S22 @ v)
        w = p - 0.5 * tau * (p @ v) * v
        S22 -= np.outer(v, w) + np.outer(w, v)
        S[k + 1, k] = S[k, k + 1] = beta
        S[k + 2:, k] = S[k, k + 2:] = 0.0
    return out


def tau_transitions(zt):
    """the set of (tau_{k-1} == 0, tau_k == 0) pairs the pipelined large kernel meets"""
    return {(a, b) for a, b in zip(zt[:-1], zt[1:])}


# ---- the cases of one (G, mode), batched -------------------------------------------------------------------------------
def rows_of(G, mode_name):
    """the admissible cases of (G, mode), in table order"""
    return list(ROWS.get((G, mode_name), {}))


def batch(G, mode_name):
    """(names, adj (B,G,G) fp32): the admissible cases of one size and mode as ONE batch"""
    names = rows_of(G, mode_name)
    return names, torch.stack([adjacency(n, G) for n in names])


# ---- bounds ---------------------------------------------------------------------------------------------------------
def scale(G):
    """the suite's bars are stated at G <= 128 and grow with G / 128 above (tests/test_gpu_spectral_large.py)"""
    return max(1.0, G / 128)


VAL_TOL = 2e-5          # |lambda - lambda64|                                  (test_gpu_spectral.py)
RES_TOL = 2e-5          # max |S v - lambda v|, top-k routes                   (test_gpu_spectral_large.py)
RES_TOL_JACOBI = 3e-5   # ... Jacobi route                                     (test_full_batch_properties)
ORTH_TOL = 1e-5         # |V^T V - I|, top-k routes                            (test_topk_only_path_...)
ORTH_TOL_JACOBI = 3e-5  # ... Jacobi route                                     (test_full_batch_properties)
LEAK_TOL = 2e-5         # max_i |v_i - P P^T v_i|_2 * gap                      (the err * gap bar)


def cpu_argsort_rows(v):
    """(rows, n) fp32 -> ascending argsort, ties by index: what spectral.argsort_rows computes"""
    return torch.sort(v, dim=1, stable=True)[1]


def convention_sign(vecs):
    """(B,G,k) fp32 -> (B,1,k) +-1: the sign of the entry of largest fp32 magnitude, first index on ties"""
    first = vecs.abs().argmax(dim=1, keepdim=True)              # torch: the first of equal maxima
    s = torch.sign(torch.gather(vecs, 1, first))
    s[s == 0] = 1
    return s


def check_eigenpairs(S64, vals, vecs, order, G, mode, *, jacobi=False, parity=None, argsort=cpu_argsort_rows, tag="",
                     ref=None, measure_only=False):
    """Hold one batched result to the float64 decomposition of S64 (B,G,G).

    vals (B,k) fp32, vecs (B,G,k) fp32, order (B,k,G) int64 or None, all on the CPU.  ``parity``: per sample the tuple
    of columns that also get order parity with the float64 vector (ROWS), or None.  ``argsort``: (rows, n) fp32 ->
    int64, the argsort the orders are compared with bit for bit (the device's on the GPU).  ``ref``: (w64, V64) if the
    caller has them already.  Returns one dict of measured figures per sample; asserts every bound -- with
    ``measure_only`` only what the measuring itself relies on (finite values, orders that are permutations), so that a
    caller can record the figures of a failing row before it asserts."""
    from test_gpu_spectral import align_sign, assert_order_matches_oracle
    B, k = vals.shape
    assert vecs.shape == (B, G, k) and S64.shape == (B, G, G), tag
    assert vals.dtype == torch.float32 and vecs.dtype == torch.float32, tag
    s = scale(G)
    # 1. finite
    assert torch.isfinite(vals).all() and torch.isfinite(vecs).all(), f"{tag}: non-finite eigenpairs"
    # 2. the orders are permutations -- before anything gathers with them
    if order is not None:
        assert order.shape == (B, k, G) and order.dtype == torch.int64, tag
        want_perm = torch.arange(G).expand(B, k, G)
        assert torch.equal(order.sort(dim=2)[0], want_perm), f"{tag}: order is not a permutation of 0..G-1"
    w64, V64 = ref if ref is not None else torch.linalg.eigh(S64)
    sel = selected_indices(G, mode)
    v64 = vecs.double()
    out = []
    for b in range(B):
        t = f"{tag}[{b}]"
        w = w64[b].numpy()
        idx, gap = cluster_of(w, sel)
        assert gap >= MIN_GAP, f"{t}: inadmissible row, gap {gap:.3e}"
        # 3. eigenvalues
        val_err = (vals[b].double() - w64[b, sel]).abs().max().item()
        # 4. residual with the device's own lambda
        res = (S64[b] @ v64[b] - v64[b] * vals[b].double()[None, :]).abs().max().item()
        # 5. orthonormality
        orth = (v64[b].T @ v64[b] - torch.eye(k, dtype=torch.float64)).abs().max().item()
        # 6. distance from the cluster's invariant subspace
        P = V64[b][:, idx]
        leak = (v64[b] - P @ (P.T @ v64[b])).norm(dim=0).max().item()
        out.append(dict(val_err=val_err, residual=res, orth=orth, leak=leak, gap=gap, cluster=int(idx.size)))
        if measure_only:
            continue
        assert val_err <= VAL_TOL * s, f"{t}: eigenvalue error {val_err:.3e} > {VAL_TOL * s:.1e}"
        rtol = (RES_TOL_JACOBI if jacobi else RES_TOL) * s
        assert res <= rtol, f"{t}: residual {res:.3e} > {rtol:.1e}"
        otol = (ORTH_TOL_JACOBI if jacobi else ORTH_TOL) * s
        assert orth <= otol, f"{t}: orthonormality {orth:.3e} > {otol:.1e}"
        assert leak * (gap if np.isfinite(gap) else 0.0) <= LEAK_TOL * s, \
            f"{t}: subspace leakage {leak:.3e} x gap {gap:.3e} > {LEAK_TOL * s:.1e}"
    if measure_only:
        return out
    # 7. sign convention
    big = torch.gather(vecs, 1, vecs.abs().argmax(dim=1, keepdim=True))
    assert (big > 0).all(), f"{tag}: sign convention (largest-magnitude entry positive)"
    if order is not None:
        # 8. the order IS the argsort of the kernel's own vectors
        rows = vecs.transpose(1, 2).reshape(B * k, G).contiguous()
        assert torch.equal(order.reshape(B * k, G), argsort(rows).reshape(B * k, G)), \
            f"{tag}: order differs from the argsort of the returned vectors"
        # 9. order parity with the float64 vectors where they are defined
        for b in range(B):
            cols = list(parity[b]) if parity is not None and parity[b] else []
            if not cols:
                continue
            w = w64[b].numpy()
            _, gap = cluster_of(w, sel)
            assert gap >= PARITY_GAP and all(alone(w, sel[i]) for i in cols), f"{tag}[{b}]: parity flag on a cluster"
            wv = V64[b][:, [sel[i] for i in cols]][None]                        # (1,G,n)
            gv, sgn = align_sign(v64[b][:, cols][None], wv)
            err = (gv - wv).abs().amax(dim=1)
            worder = torch.sort(wv.transpose(1, 2), dim=2, stable=True)[1]
            hit, tot = assert_order_matches_oracle(order[b:b + 1, cols], sgn, wv, worder, err, f"{tag}[{b}] parity")
            out[b]["parity_hits"] = [hit, tot]
    return out


# ---- clouds with exact ties, for the route from centres ---------------------------------------------------------------
def dyadic_clouds():
    """{name: (1,G,3) fp32} DISTINCT points with dyadic coordinates: squared distances are exact in fp32 and equal exactly
    when they are equal in float64.  The full 4 x 4 x 4 and 4 x 4 x 8 grids over 8, and a random lattice draw
    (tests/lattice_clouds.py) with its repeated points removed (first occurrence kept), cut to 100 points."""
    import lattice_clouds
    draw = lattice_clouds.lattice(1, 160, 4, 77)[0]
    seen, keep = set(), []
    for i, q in enumerate(draw.tolist()):
        if tuple(q) not in seen:
            seen.add(tuple(q))
            keep.append(i)
    return {"grid64": (grid_points(64).float() / 8)[None], "grid128": (grid_points(128).float() / 8)[None],
            "draw100": draw[keep[:100]][None].clone()}


def knn_adjacency_ref(points, knn, alpha, symmetric, self_loop, binary):
    """oracle.spectral_ref.create_graph_from_feature_space with its ``topk`` replaced by the rule the kernels document:
    the knn + 1 smallest by (float64 distance, index), the first dropped unless self_loop.  Weights with the oracle's
    fp32 ops."""
    B, N, _ = points.shape
    p = points.double()
    d2 = ((p.unsqueeze(2) - p.unsqueeze(1)) ** 2).sum(-1)
    idx = torch.sort(d2, dim=-1, stable=True)[1][:, :, :knn + 1]
    diff = points.unsqueeze(2) - points.unsqueeze(1)
    d = torch.gather(torch.sqrt(torch.sum(diff ** 2, dim=-1)), 2, idx)
    if not self_loop:
        idx, d = idx[:, :, 1:], d[..., 1:]
    w = torch.exp((-1) * alpha * d ** 2)
    return sr._scatter_adjacency(B, N, idx, w, symmetric, binary, points.dtype)


# ---- the table ---------------------------------------------------------------------------------------------------------
# {(G, mode): {case: (gap, cluster size, parity columns)}}, written by hand from the float64 reference and re-derived by
# test_oracle_degenerate_graphs.py (gap to 4 significant digits).  Gap INF: the cluster is the whole spectrum (complete,
# rw, smallest: 0 and the (G-1)-fold eigenvalue), so there is nothing to leak into and the subspace bound holds trivially.
INF = float("inf")
ROWS = {
    (63, 'rw_small'): {
        'ring': (0.1075, 5, ()),
        'path': (0.009119, 4, (1, 2, 3)),
        'complete': (INF, 63, ()),
        'two_rings': (0.003089, 4, ()),
        'ring_path_ring': (0.03918, 4, ()),
        'lattice': (0.1056, 4, (0, 1, 2, 3)),
        'star': (7.874, 62, ()),
        'double_star': (0.01613, 61, ()),
    },
    (63, 'sym_small'): {
        'ring': (0.02307, 4, ()),
        'path': (0.001365, 4, (0, 1, 2, 3)),
        'complete': (1.016, 62, ()),
        'two_rings': (0.1338, 6, ()),
        'ring_path_ring': (0.06, 5, ()),
        'lattice': (0.0303, 4, (0, 1, 2, 3)),
        'star': (1, 61, ()),
        'double_star': (0.01613, 60, ()),
    },
    (63, 'rw_large'): {
        'ring': (0.0008784, 4, ()),
        'path': (0.009119, 4, (1, 2, 3)),
        'complete': (1.016, 62, ()),
        'two_rings': (0.01459, 4, ()),
        'ring_path_ring': (0.0836, 4, ()),
        'lattice': (0.006622, 4, (0, 1, 2, 3)),
        'star': (7.874, 62, ()),
        'double_star': (5.531, 62, ()),
    },
    (64, 'rw_small'): {
        'ring': (0.1044, 5, ()),
        'path': (0.008831, 4, (1, 2, 3)),
        'complete': (INF, 64, ()),
        'two_rings': (0.1368, 6, ()),
        'ring_path_ring': (0.03918, 4, ()),
        'lattice': (0.1017, 4, (0, 1, 2, 3)),
        'star': (7.937, 63, ()),
        'double_star': (0.01587, 62, ()),
    },
    (64, 'sym_small'): {
        'ring': (0.02236, 4, ()),
        'path': (0.001324, 4, (0, 1, 2, 3)),
        'complete': (1.016, 63, ()),
        'two_rings': (0.1368, 6, ()),
        'ring_path_ring': (0.05053, 5, ()),
        'lattice': (0.03547, 4, (0, 1, 2, 3)),
        'star': (1, 62, ()),
        'double_star': (0.01587, 61, ()),
    },
    (64, 'rw_large'): {
        'ring': (0.01202, 4, ()),
        'path': (0.008831, 4, (1, 2, 3)),
        'complete': (1.016, 63, ()),
        'two_rings': (0.01459, 4, ()),
        'ring_path_ring': (0.0836, 4, ()),
        'lattice': (0.02045, 4, (0, 1, 2, 3)),
        'star': (7.937, 63, ()),
        'double_star': (5.576, 63, ()),
    },
    (127, 'rw_small'): {
        'ring': (0.02803, 5, ()),
        'path': (0.00234, 4, (1, 2, 3)),
        'complete': (INF, 127, ()),
        'two_rings': (0.0003834, 4, ()),
        'ring_path_ring': (0.009412, 4, ()),
        'lattice': (0.01505, 4, (0, 1, 2, 3)),
        'star': (11.22, 126, ()),
        'double_star': (0.007937, 125, ()),
    },
    (127, 'sym_small'): {
        'ring': (0.005703, 4, ()),
        'path': (0.0003527, 4, ()),
        'complete': (1.008, 126, ()),
        'two_rings': (0.03527, 6, ()),
        'ring_path_ring': (0.01458, 5, ()),
        'lattice': (0.02961, 4, (0, 1, 2, 3)),
        'star': (1, 125, ()),
        'double_star': (0.007937, 124, ()),
    },
    (127, 'rw_large'): {
        'ring': (0.002314, 4, ()),
        'path': (0.00234, 4, (1, 2, 3)),
        'complete': (1.008, 126, ()),
        'two_rings': (0.001392, 4, ()),
        'ring_path_ring': (0.02085, 4, ()),
        'lattice': (0.03897, 4, (0, 1, 2, 3)),
        'star': (11.22, 126, ()),
        'double_star': (7.91, 126, ()),
    },
    (128, 'rw_small'): {
        'ring': (0.0276, 5, ()),
        'path': (0.00231, 4, (1, 2, 3)),
        'complete': (INF, 128, ()),
        'two_rings': (0.03565, 6, ()),
        'ring_path_ring': (0.009412, 4, ()),
        'lattice': (0.0165, 4, (0, 1, 2, 3)),
        'star': (11.27, 127, ()),
        'double_star': (0.007874, 126, ()),
    },
    (128, 'sym_small'): {
        'ring': (0.005614, 4, ()),
        'path': (0.0003474, 4, ()),
        'complete': (1.008, 127, ()),
        'two_rings': (0.03565, 6, ()),
        'ring_path_ring': (0.01351, 5, ()),
        'lattice': (0.02928, 4, (0, 1, 2, 3)),
        'star': (1, 126, ()),
        'double_star': (0.007874, 125, ()),
    },
    (128, 'rw_large'): {
        'ring': (0.00555, 4, ()),
        'path': (0.00231, 4, (1,)),
        'complete': (1.008, 127, ()),
        'two_rings': (0.001392, 4, ()),
        'ring_path_ring': (0.02085, 4, ()),
        'lattice': (0.02263, 4, (0, 1, 2, 3)),
        'star': (11.27, 127, ()),
        'double_star': (7.941, 127, ()),
    },
    (160, 'rw_small'): {
        'ring': (0.01778, 5, ()),
        'path': (0.001636, 4, (3,)),
        'complete': (INF, 160, ()),
        'two_rings': (0.02293, 6, ()),
        'ring_path_ring': (0.006083, 4, ()),
        'lattice': (0.0267, 4, (0, 1, 2, 3)),
        'star': (12.61, 159, ()),
        'double_star': (0.006289, 158, ()),
    },
    (160, 'sym_small'): {
        'ring': (0.003595, 4, ()),
        'complete': (1.006, 159, ()),
        'two_rings': (0.02293, 6, ()),
        'ring_path_ring': (0.00909, 5, ()),
        'lattice': (0.0152, 4, (0, 1, 2, 3)),
        'star': (1, 158, ()),
        'double_star': (0.006289, 157, ()),
    },
    (160, 'rw_large'): {
        'ring': (0.0006693, 4, ()),
        'path': (0.001636, 4, (1, 2)),
        'complete': (1.006, 159, ()),
        'two_rings': (0.003209, 4, ()),
        'ring_path_ring': (0.01297, 4, ()),
        'lattice': (0.03035, 4, (0, 1, 2, 3)),
        'star': (12.61, 159, ()),
        'double_star': (8.891, 159, ()),
    },
    (255, 'rw_small'): {
        'ring': (0.007051, 5, ()),
        'path': (0.0008467, 4, ()),
        'complete': (INF, 255, ()),
        'two_rings': (0.008958, 6, ()),
        'lattice': (0.03363, 4, (0, 1, 2, 3)),
        'star': (15.94, 254, ()),
        'double_star': (0.003937, 253, ()),
    },
    (255, 'sym_small'): {
        'ring': (0.001416, 4, ()),
        'path': (0.000689, 5, ()),
        'complete': (1.004, 254, ()),
        'two_rings': (0.008958, 6, ()),
        'ring_path_ring': (0.003494, 5, ()),
        'lattice': (0.009433, 4, (0, 1, 2, 3)),
        'star': (1, 253, ()),
        'double_star': (0.003937, 252, ()),
    },
    (255, 'rw_large'): {
        'ring': (0.00191, 4, ()),
        'path': (0.0008467, 4, ()),
        'complete': (1.004, 254, ()),
        'two_rings': (0.001574, 4, ()),
        'ring_path_ring': (0.00497, 4, ()),
        'lattice': (0.02912, 4, (0, 1, 2, 3)),
        'star': (15.94, 254, ()),
        'double_star': (11.25, 254, ()),
    },
    (128, 'rw_small_k7'): {
        'two_rings': (0.05813, 10, ()),
    },
    (255, 'rw_small_k7'): {
        'ring_path_ring': (0.002735, 8, ()),
    },
}

# cases the float64 reference shows inadmissible (gap < MIN_GAP) at a (G, mode): {(G, mode): {case: gap}}
INADMISSIBLE = {
    (160, 'sym_small'): {'path': 0.000227},
    (255, 'rw_small'): {'ring_path_ring': 0.00021},
}
