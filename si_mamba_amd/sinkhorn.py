"""Debiased Sinkhorn divergence between point sets of unequal size on the HIP kernels of csrc/sinkhorn.hip.

The transport distance for the case ``earth_movers_distance`` refuses: n against m points, smooth in both sets (the
``SamplesLoss("sinkhorn")`` of geomloss with uniform weights and squared Euclidean cost, stated in include/simamba.h).
"""
from __future__ import annotations

import torch

from . import _lib
from ._pointsets import as_pairs, lengths_i32

SINKHORN_MAX_POINTS = 8192
SINKHORN_MAX_STEPS = 4096


def scaling_steps(eps_rel: float) -> int:
    """S = ceil(log2(1 / eps_rel)): the first S with 2^-S <= eps_rel, as the library counts it (eps_rel as fp32)."""
    eps_rel = torch.tensor(float(eps_rel), dtype=torch.float32).item()
    s = 0
    while 2.0 ** -s > eps_rel:
        s += 1
    return s


def _lengths(lengths, device):
    return lengths_i32(None if lengths is None else lengths.to(device))


class SinkhornFn(torch.autograd.Function):
    """div, ot_xy, merr and the potentials f_xy, g_xy, g_xx, g_yy, f_yy of simamba_sinkhorn_fwd; the gradient holds
    the potentials fixed."""

    @staticmethod
    def forward(ctx, x, y, xlen, ylen, eps_rel, iters, debias):
        _lib.require_gpu(x, "sinkhorn_divergence")
        _lib.require_gpu(y, "sinkhorn_divergence")
        xf = x.float().contiguous()
        yf = y.float().contiguous()
        pairs, n, _ = xf.shape
        m = yf.shape[1]
        dev = xf.device
        flags = _lib.SINKHORN_DEBIAS if debias else 0
        new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)       # noqa: E731
        div, ot_xy, merr = new(pairs), new(pairs), new(pairs)
        f_xy, g_xy = new(pairs, n), new(pairs, m)
        g_xx, g_yy, f_yy = (new(pairs, n), new(pairs, m), new(pairs, m)) if debias else (None, None, None)
        ws_bytes = _lib.load().simamba_sinkhorn_workspace_bytes(pairs, n, m, flags)
        ws = torch.empty(ws_bytes // 4, device=dev, dtype=torch.float32)
        _lib.count("sinkhorn")
        _lib.call("simamba_sinkhorn_fwd", xf, yf, xlen, ylen, div, ot_xy, merr, f_xy, g_xy, g_xx, g_yy, f_yy, pairs, n,
                  m, eps_rel, iters, flags, ws, ws_bytes, device=dev, time_as="sinkhorn_fwd")
        ctx.save_for_backward(xf, yf, xlen, ylen, f_xy, g_xy, g_xx, f_yy)
        ctx.dtypes = (x.dtype, y.dtype)
        ctx.args = (eps_rel, flags)
        empty = new(0)
        pots = tuple(empty if t is None else t for t in (f_xy, g_xy, g_xx, g_yy, f_yy))
        ctx.mark_non_differentiable(ot_xy, merr, *pots)
        return (div, ot_xy, merr) + pots

    @staticmethod
    def backward(ctx, ddiv, *unused):
        xf, yf, xlen, ylen, f_xy, g_xy, g_xx, f_yy = ctx.saved_tensors
        eps_rel, flags = ctx.args
        pairs, n, _ = xf.shape
        m = yf.shape[1]
        dev = xf.device
        dx = torch.empty_like(xf) if ctx.needs_input_grad[0] else None
        dy = torch.empty_like(yf) if ctx.needs_input_grad[1] else None
        ws = torch.empty(pairs, device=dev, dtype=torch.float32)
        _lib.call("simamba_sinkhorn_bwd", xf, yf, xlen, ylen, ddiv.float().contiguous(), f_xy, g_xy, g_xx, f_yy, dx, dy,
                  pairs, n, m, eps_rel, flags, ws, 4 * pairs, device=dev, time_as="sinkhorn_bwd")
        if dx is not None:
            dx = dx.to(ctx.dtypes[0])
        if dy is not None:
            dy = dy.to(ctx.dtypes[1])
        return dx, dy, None, None, None, None, None


def sinkhorn_divergence(x, y, *, x_lengths=None, y_lengths=None, eps_rel=2.0 ** -6, iters=16, debias=True,
                        return_info=False):
    """(P, n, 3), (P, m, 3) -> div (P,) fp32: ``OT_eps(x, y) - OT_eps(x, x) / 2 - OT_eps(y, y) / 2`` of each pair, with
    uniform masses, cost ``|x_i - y_j|^2`` and 1 <= n, m <= 8192; ``(n, 3)`` against ``(m, 3)`` is one pair.  Inputs are
    cast with ``.float()``.

    ``eps_rel``, ``iters``: the temperature is scaled down from the pair's ``diam2`` (the squared diagonal of the
    bounding box of both sets) by halves, ``ceil(log2(1 / eps_rel))`` steps, then ``iters`` steps run at
    ``diam2 * eps_rel``; 0 < eps_rel <= 1, iters >= 0, 1 to 4096 steps in all.  The defaults (6 + 16 steps) are a
    choice, not a measurement: ``merr`` says whether they suffice.
    ``x_lengths``, ``y_lengths``: (P,) integer tensors for ragged batches: pair p is the first ``x_lengths[p]`` points
    of ``x[p]`` against the first ``y_lengths[p]`` of ``y[p]``.  The kernels clamp them to [1, n] and [1, m]; nothing
    at or behind a length is read, gradients there are 0, and every pair's result is what it returns alone.
    ``debias=False``: ``OT_eps(x, y)`` alone.
    ``return_info``: also return ``ot_xy`` (P,) and ``merr`` (P,), the row-marginal error of the transport plan after
    the last step (the counterpart of the EMD's ``converged``).

    Differentiable in both arguments with the potentials held fixed, which is exact at convergence.  The divergence of
    a set from itself is 0.0 and its gradients are exactly 0.  The same bits every call.  Nothing is read on the host,
    so the call can be captured in a hipGraph."""
    if x.dim() != y.dim() or x.dim() not in (2, 3) or x.shape[-1] != 3 or y.shape[-1] != 3 or \
            (x.dim() == 3 and x.shape[0] != y.shape[0]):
        raise ValueError(f"sinkhorn_divergence: x and y must be (P, n, 3) and (P, m, 3), or (n, 3) and (m, 3), got "
                         f"{tuple(x.shape)} and {tuple(y.shape)}")
    x, y, single = as_pairs(x, y)
    pairs, n, m = x.shape[0], x.shape[1], y.shape[1]
    if not (1 <= n <= SINKHORN_MAX_POINTS and 1 <= m <= SINKHORN_MAX_POINTS) or pairs < 1:
        raise ValueError(f"sinkhorn_divergence: 1 <= n, m <= {SINKHORN_MAX_POINTS} points per set and at least one "
                         f"pair, got n = {n}, m = {m}, {pairs} pairs")
    eps_rel, iters = float(eps_rel), int(iters)
    if not 0.0 < torch.tensor(eps_rel, dtype=torch.float32).item() <= 1.0:
        raise ValueError(f"sinkhorn_divergence: eps_rel must be in (0, 1] as an fp32 number, got {eps_rel!r}")
    if iters < 0 or not 1 <= scaling_steps(eps_rel) + iters <= SINKHORN_MAX_STEPS:
        raise ValueError(f"sinkhorn_divergence: iters >= 0 and 1 to {SINKHORN_MAX_STEPS} steps in all, got "
                         f"{scaling_steps(eps_rel)} scaling steps + iters = {iters}")
    for name, t in (("x_lengths", x_lengths), ("y_lengths", y_lengths)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.shape != (pairs,) or t.is_floating_point()):
            raise ValueError(f"sinkhorn_divergence: {name} must be an integer tensor of shape ({pairs},)")
    _lib.require_gpu(x, "sinkhorn_divergence")
    out = SinkhornFn.apply(x, y, _lengths(x_lengths, x.device), _lengths(y_lengths, x.device), eps_rel,
                           iters, bool(debias))
    div, ot_xy, merr = out[:3]
    if single:
        div, ot_xy, merr = div[0], ot_xy[0], merr[0]
    return (div, ot_xy, merr) if return_info else div
