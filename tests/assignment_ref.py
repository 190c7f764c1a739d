"""Exact minimum-cost assignment in numpy, and the float64 cost of a given matching.

TEST INFRASTRUCTURE (shared by test_emd_abi.py, CPU, and test_gpu_emd.py).  The earth mover's distance kernels
(csrc/emd.hip) return a matching that an auction found; what they are held to is the optimum, which needs an exact
solver.  scipy is not part of what the GPU tests may assume, so the solver is here: the Hungarian method in its
shortest-augmenting-path form (Jonker-Volgenant; O(n^3), the inner loop over columns vectorised), on float64 costs.  On
the lattice clouds of lattice_clouds.py every cost is a multiple of 1/64 far below 2^53, so every sum and difference the
solver forms is exact and so is its optimum.

No GPU code runs here and no expected output is written down.
"""
import functools
import itertools

import numpy as np


def cost_matrix(x, y):
    """(n, 3), (n, 3) -> (n, n) float64 squared Euclidean distances, formed from the differences."""
    d = np.asarray(x, dtype=np.float64)[:, None, :] - np.asarray(y, dtype=np.float64)[None, :, :]
    return (d * d).sum(-1)


def min_cost_assignment(cost):
    """(n, n) float64 -> (assign (n,) int64 with assign[i] the column of row i, total cost)."""
    cost = np.asarray(cost, dtype=np.float64)
    n = cost.shape[0]
    assert cost.shape == (n, n)
    u, v = np.zeros(n + 1), np.zeros(n + 1)             # potentials of rows and columns, 1-based; slot 0 is virtual
    p = np.zeros(n + 1, dtype=np.int64)                 # p[j]: row matched to column j, 0 = none
    way = np.zeros(n + 1, dtype=np.int64)
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv = np.full(n + 1, np.inf)
        used = np.zeros(n + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            better = ~used[1:] & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            masked = np.where(used[1:], np.inf, minv[1:])
            j1 = int(masked.argmin()) + 1
            delta = masked[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    assign = np.empty(n, dtype=np.int64)
    assign[p[1:] - 1] = np.arange(n)
    return assign, float(cost[np.arange(n), assign].sum())


def brute_force(cost):
    """The optimum over all n! permutations (n <= 8 or so)."""
    cost = np.asarray(cost, dtype=np.float64)
    n = cost.shape[0]
    rows = np.arange(n)
    return min(float(cost[rows, list(perm)].sum()) for perm in itertools.permutations(range(n)))


def matched_cost(x, y, assign):
    """sum_i |x_i - y_assign[i]|^2 in float64."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    d = x - y[np.asarray(assign, dtype=np.int64)]
    return float((d * d).sum())


def is_permutation(assign):
    a = np.asarray(assign, dtype=np.int64)
    return a.ndim == 1 and np.array_equal(np.sort(a), np.arange(a.shape[0]))


# ---- the inputs the GPU tests walk, and their optima (solved once per process) ---------------------------------------
# both instantiations (one wave per pair up to 64 points, one workgroup above) and their boundary, lane counts that are
# and are not multiples of the wave; five pairs leave the one-wave kernel's last workgroup (four pairs) partial
EMD_SIZES = (1, 2, 3, 31, 32, 33, 64, 65, 255, 256, 1000, 1024)


def emd_pairs(n):
    return 5 if n <= 64 else 2


def emd_seed(n):
    return 100 + n


def lattice_eps(n):
    """The largest power of two below 1 / (64 n): lattice costs are multiples of 1/64, so an optimality gap below
    n * eps < 1/64 is no gap."""
    k = 0
    while 2.0 ** -k >= 1.0 / (64 * n):
        k += 1
    return 2.0 ** -k


def distinct_lattice(n, seed):
    """(n, 3) fp32, n distinct sites of the lattice {-8 .. 8}^3 / 8 (4913 sites): any two are at least 1/64 apart in
    squared distance."""
    import torch
    g = torch.Generator().manual_seed(seed)
    site = torch.randperm(17 ** 3, generator=g)[:n]
    return torch.stack([site // 289, (site // 17) % 17, site % 17], -1).float().sub(8).div(8)


def gaussian_pairs(pairs, n, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randn(pairs, n, 3, generator=g), torch.randn(pairs, n, 3, generator=g)


def lattice_pairs(pairs, n, seed):
    """The exact-tie clouds of lattice_clouds.lattice with R = 4, scale = 8: every cost a multiple of 1/64, at most 3."""
    import lattice_clouds
    return lattice_clouds.lattice(pairs, n, 4, seed, scale=8), lattice_clouds.lattice(pairs, n, 4, seed + 1, scale=8)


@functools.lru_cache(maxsize=None)
def solved(kind, pairs, n, seed):
    """(x, y, optimum (pairs,) float64, cmax (pairs,) float64) for ``kind`` in ("gaussian", "lattice")."""
    x, y = (gaussian_pairs if kind == "gaussian" else lattice_pairs)(pairs, n, seed)
    costs = [cost_matrix(x[p].numpy(), y[p].numpy()) for p in range(pairs)]
    opt = np.array([min_cost_assignment(c)[1] for c in costs])
    return x, y, opt, np.array([c.max() for c in costs])
