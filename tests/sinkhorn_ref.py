"""The debiased Sinkhorn divergence of include/simamba.h, dense, in torch on the CPU, in a chosen dtype.

TEST INFRASTRUCTURE (shared by test_oracle_sinkhorn.py, CPU, and test_gpu_sinkhorn.py).  It restates the procedure the
kernels of csrc/sinkhorn.hip implement, step for step: masses 1/nx and 1/ny, costs (dx*dx + dy*dy) + dz*dz, diam2 from
the bounding box of the pair's points, S = ceil(log2(1 / eps_rel)) scaling steps at diam2 * 2^-t and ``iters`` steps at
diam2 * eps_rel, an f-update followed by a g-update from g = 0, the value from the final potentials, the row-marginal
error from one further f-update, and the gradient with the potentials held fixed.  The inputs are fp32 tensors (float64
ones only where a test perturbs them for finite differences); ``dtype`` is what everything after them is computed in.
``ref_error`` is the float32 run against the float64 run: the number the GPU tests scale their bars from, measured on
the reference alone.

Cost matrices are formed in row blocks of at most 2^18 entries, so (8192, 8192) fits a test machine.  No GPU code runs
here and no expected output is written down.
"""
import functools
import math

import torch

BLOCK = 1 << 18


def scaling_steps(eps_rel):
    """The first S with 2^-S <= eps_rel (eps_rel as the fp32 value the library is handed)."""
    eps_rel = torch.tensor(float(eps_rel), dtype=torch.float32).item()
    s = 0
    while 2.0 ** -s > eps_rel:
        s += 1
    return s


def diam2_of(x, y):
    """Squared diagonal of the bounding box of the points of x and y, at least 1e-30, in their dtype."""
    pts = torch.cat([x, y], 0)
    e = pts.amax(0) - pts.amin(0)
    d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    return torch.clamp(d2, min=1e-30) if d2 == d2 else d2


def _blocks(nr, nc):
    step = max(1, BLOCK // nc)
    return [(s, min(s + step, nr)) for s in range(0, nr, step)]


def _diff_cost(rows, cols):
    """The three coordinate differences (nr, nc) each, and the cost (dx*dx + dy*dy) + dz*dz."""
    colsT = cols.t().contiguous()
    d = [rows[:, c:c + 1] - colsT[c][None, :] for c in range(3)]
    return d, (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def softmin(eps, rows, cols, pot):
    """out_i = -eps log sum_j (1 / nc) exp((pot_j - C_ij) / eps)"""
    nc = cols.shape[0]
    out = torch.empty(rows.shape[0], dtype=rows.dtype)
    for s, e in _blocks(rows.shape[0], nc):
        _, c = _diff_cost(rows[s:e], cols)
        out[s:e] = -eps * torch.logsumexp((pot[None, :] - c) / eps - math.log(nc), 1)
    return out


def plan_mean(eps, rows, cols, pot):
    """out_i = sum_j softmax_j((pot_j - C_ij) / eps) (rows_i - cols_j), (nr, 3)"""
    out = torch.empty_like(rows)
    for s, e in _blocks(rows.shape[0], cols.shape[0]):
        d, c = _diff_cost(rows[s:e], cols)
        w = torch.softmax((pot[None, :] - c) / eps, 1)
        out[s:e] = torch.stack([(w * dc).sum(1) for dc in d], 1)
    return out


def solve_problem(eps_list, rows, cols):
    """The schedule on one problem: (f over rows, g over cols) after the last step."""
    f = torch.zeros(rows.shape[0], dtype=rows.dtype)
    g = torch.zeros(cols.shape[0], dtype=rows.dtype)
    for eps in eps_list:
        f = softmin(eps, rows, cols, g)
        g = softmin(eps, cols, rows, f)
    return f, g


def sinkhorn_pair(x, y, eps_rel=2.0 ** -6, iters=16, dtype=torch.float64, debias=True, diam2=None):
    """One pair, x (n, 3) and y (m, 3) fp32 -> dict of div, ot_xy, merr, the potentials f_xy, g_xy, g_xx, g_yy, f_yy,
    and the gradients dx, dy of div (potentials held fixed), all in ``dtype``.  ``diam2``: use this value instead of
    the bounding box's (finite differences with the temperature held fixed)."""
    assert x.dtype == y.dtype and (x.dtype == torch.float32 or x.dtype == dtype)     # float64 points: differences only
    x, y = x.to(dtype), y.to(dtype)
    n, m = x.shape[0], y.shape[0]
    d2 = diam2_of(x, y) if diam2 is None else torch.as_tensor(diam2, dtype=dtype)
    rel = torch.tensor(float(eps_rel), dtype=torch.float32).to(dtype)
    S = scaling_steps(eps_rel)
    eps_list = [d2 * 2.0 ** -t for t in range(S)] + [d2 * rel] * iters
    assert eps_list, "at least one step"
    eps = d2 * rel
    f_xy, g_xy = solve_problem(eps_list, x, y)
    ot_xy = f_xy.sum() / n + g_xy.sum() / m
    f_plus = softmin(eps, x, y, g_xy)
    merr = (1.0 - torch.exp((f_xy - f_plus) / eps)).abs().sum() / n
    dx = plan_mean(eps, x, y, g_xy)
    dy = plan_mean(eps, y, x, f_xy)
    out = dict(diam2=d2, ot_xy=ot_xy, merr=merr, f_xy=f_xy, g_xy=g_xy)
    if debias:
        f_xx, g_xx = solve_problem(eps_list, x, x)
        f_yy, g_yy = solve_problem(eps_list, y, y)
        ot_xx = f_xx.sum() / n + g_xx.sum() / n
        ot_yy = f_yy.sum() / m + g_yy.sum() / m
        out.update(div=ot_xy - 0.5 * ot_xx - 0.5 * ot_yy, g_xx=g_xx, g_yy=g_yy, f_yy=f_yy)
        dx = dx - plan_mean(eps, x, x, g_xx)
        dy = dy - plan_mean(eps, y, y, f_yy)
    else:
        out.update(div=ot_xy)
    out.update(dx=dx * (2.0 / n), dy=dy * (2.0 / m))
    return out


def sinkhorn_batch(x, y, **kw):
    """(P, n, 3), (P, m, 3) -> dict of stacked results of sinkhorn_pair."""
    per = [sinkhorn_pair(x[p], y[p], **kw) for p in range(x.shape[0])]
    return {k: torch.stack([r[k] for r in per]) for k in per[0]}


def gaussian_sets(pairs, n, m, seed):
    """x standard normal, y narrower and off centre: a divergence well away from 0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(pairs, n, 3, generator=g)
    y = 0.75 * torch.randn(pairs, m, 3, generator=g) + torch.tensor([0.5, -0.25, 0.125])
    return x, y


# ---- the cases the GPU tests walk (pairs, n, m): one lane, less than one wave, one off the wave multiple, one off the
# row block and tile, several tiles with a remainder in both roles, the reconstruct() shape, and one full tile plus one
# column (1025: the second tile is one point and seven columns of padding, on the first step without a potential)
SIZES = ((5, 1, 1), (3, 2, 3), (4, 63, 65), (2, 256, 257), (2, 300, 1000), (1, 1000, 300), (1, 2048, 1024),
         (2, 9, 1025))
SETTINGS = ((2.0 ** -6, 16), (2.0 ** -9, 4))
LIMIT_CASE = (1, 8192, 8192, 2.0 ** -3, 2)


def case_seed(pairs, n, m):
    return 7000 + 31 * n + m + pairs


@functools.lru_cache(maxsize=None)
def reference(pairs, n, m, eps_rel, iters):
    """(x, y, float32 run, float64 run) of one case; computed once per process and not to be written to."""
    x, y = gaussian_sets(pairs, n, m, case_seed(pairs, n, m))
    r32 = sinkhorn_batch(x, y, eps_rel=eps_rel, iters=iters, dtype=torch.float32)
    r64 = sinkhorn_batch(x, y, eps_rel=eps_rel, iters=iters, dtype=torch.float64)
    return x, y, r32, r64


def ref_error(case):
    """case = (pairs, n, m, eps_rel, iters) -> the largest absolute difference between the float32 and the float64 run
    of this helper on the same fp32 inputs, per quantity: {"div", "ot_xy", "dx", "dy"}."""
    _, _, r32, r64 = reference(*case)
    return {k: (r32[k].double() - r64[k]).abs().max().item() for k in ("div", "ot_xy", "dx", "dy")}


def ulp32(v):
    """The spacing of fp32 at |v| (v a float or a tensor: its largest magnitude)."""
    v = float(torch.as_tensor(v).abs().max())
    return 2.0 ** -149 if v < 2.0 ** -126 else 2.0 ** (math.floor(math.log2(v)) - 23)
