"""Earth mover's distance between equal-sized point sets on the HIP auction kernels (csrc/emd.hip).

The other standard point-set distance next to Chamfer: the mean squared distance under the cheapest one-to-one matching
of the two sets.  In the Point-BERT / Point-MAE lineage it is ``emd()``, a CUDA-only extension; the reference leaves it
commented out (models/point_mamba.py:2947-2956).
"""
from __future__ import annotations

import torch

from . import _lib
from ._pointsets import as_pairs

EMD_MAX_POINTS = 1024


def default_max_rounds(n: int) -> int:
    """The cap on auction rounds per pair: 128 n + 4096.  At least three times the most rounds any pair of the test
    inputs takes ("Earth mover's distance", has the counts: 43 791 of 135 168 at n = 1024 on the exact-tie
    lattice with eps below 1 / (64 n), the slowest of them)."""
    return 128 * int(n) + 4096


class EmdFn(torch.autograd.Function):
    """dist, assign, rounds, converged of simamba_emd_fwd; the gradient holds the matching fixed."""

    @staticmethod
    def forward(ctx, x, y, eps, max_rounds):
        _lib.require_gpu(x, "earth_movers_distance")
        _lib.require_gpu(y, "earth_movers_distance")
        xf = x.float().contiguous()
        yf = y.float().contiguous()
        pairs, n, _ = xf.shape
        dev = xf.device
        dist = torch.empty(pairs, device=dev, dtype=torch.float32)
        assign = torch.empty(pairs, n, device=dev, dtype=torch.int32)
        rounds = torch.empty(pairs, device=dev, dtype=torch.int32)
        converged = torch.empty(pairs, device=dev, dtype=torch.uint8)
        _lib.count("emd")
        _lib.call("simamba_emd_fwd", xf, yf, assign, dist, rounds, converged, pairs, n, eps, max_rounds,
                  device=dev, time_as="emd_fwd")
        ctx.save_for_backward(xf, yf, assign)
        ctx.dtypes = (x.dtype, y.dtype)
        ctx.mark_non_differentiable(assign, rounds, converged)
        return dist, assign, rounds, converged

    @staticmethod
    def backward(ctx, ddist, *unused):
        xf, yf, assign = ctx.saved_tensors
        n = xf.shape[1]
        idx = assign.long().unsqueeze(-1).expand(-1, -1, 3)
        # d/dx_i = 2 (x_i - y_a(i)) / n ; d/dy_a(i) = -that: a gather and a scatter over a permutation
        g = (xf - torch.gather(yf, 1, idx)) * (ddist.float() * (2.0 / n)).view(-1, 1, 1)
        dx = g.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None
        dy = None
        if ctx.needs_input_grad[1]:
            dy = torch.empty_like(g).scatter_(1, idx, -g).to(ctx.dtypes[1])
        return dx, dy, None, None


def earth_movers_distance(x, y, *, eps=None, max_rounds=None, return_assignment=False):
    """(P, n, 3), (P, n, 3) -> dist (P,): ``mean_i |x_i - y_a(i)|^2`` under the cheapest one-to-one matching ``a`` of
    each pair, 1 <= n <= 1024; ``(n, 3)`` inputs are one pair.  Inputs are cast with ``.float()``.

    ``eps``: the auction's final epsilon, absolute, in cost units: the matching's total cost is within ``n * eps`` of
    the optimum (so ``dist`` within ``eps``).  None: ``2^-14`` of each pair's largest cost.
    ``max_rounds``: the cap on bidding rounds per pair, None: ``default_max_rounds(n)``.  A pair that reaches it reports
    ``converged == 0``; its matching is still one-to-one and its ``dist`` that matching's cost, with no promise of
    optimality.  Non-finite coordinates cannot hang the call: such a pair ends at the cap at the latest, ``assign`` is a
    permutation and ``dist`` is inf or NaN.
    ``return_assignment``: also return ``assign`` (P, n) int32 with ``assign[p, i]`` the y point matched to
    ``x[p, i]``, ``rounds`` (P,) int32 and ``converged`` (P,) uint8.

    Differentiable in both arguments with the matching held fixed: ``d/dx_i = 2 (x_i - y_a(i)) / n`` and
    ``d/dy_a(i)`` its negative.  The same bits every call.  Nothing is read on the host, so the call can be captured in
    a hipGraph (which is also why ``converged`` is returned and not raised on)."""
    if x.shape != y.shape or x.dim() not in (2, 3) or x.shape[-1] != 3:
        raise ValueError(f"earth_movers_distance: x and y must both be (P, n, 3) or (n, 3) with the same n, got "
                         f"{tuple(x.shape)} and {tuple(y.shape)}")
    x, y, single = as_pairs(x, y)
    pairs, n, _ = x.shape
    if not 1 <= n <= EMD_MAX_POINTS or pairs < 1:
        raise ValueError(f"earth_movers_distance: 1 <= n <= {EMD_MAX_POINTS} points per set and at least one pair, "
                         f"got n = {n}, {pairs} pairs")
    eps = 0.0 if eps is None else float(eps)
    if not eps >= 0.0:
        raise ValueError(f"earth_movers_distance: eps must be None or a number >= 0, got {eps!r}")
    max_rounds = default_max_rounds(n) if max_rounds is None else int(max_rounds)
    if max_rounds < 1:
        raise ValueError(f"earth_movers_distance: max_rounds must be at least 1, got {max_rounds}")
    dist, assign, rounds, converged = EmdFn.apply(x, y, eps, max_rounds)
    if single:
        dist, assign, rounds, converged = dist[0], assign[0], rounds[0], converged[0]
    return (dist, assign, rounds, converged) if return_assignment else dist
