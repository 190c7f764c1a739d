"""Chamfer distance on the HIP kernels: the one-wave pair kernels of csrc/chamfer.hip (the MAE patch loss) and the tiled
ones of csrc/chamfer_large.hip (whole clouds, ragged batches, pytorch3d's other arguments) behind one entry point,
``chamfer_distance``.  ``si_mamba_amd.mae`` re-exports every name here.
"""
from __future__ import annotations

import torch

from . import _lib, grouping
from ._pointsets import lengths_i32

CHAMFER_SMALL_MAX = 64       # points per set of the one-wave kernels (csrc/chamfer.hip); the tiled ones take 8192


class ChamferFn(torch.autograd.Function):
    """The one-wave kernels (csrc/chamfer.hip): sets of up to 64 points whose ``gt`` needs no gradient (the MAE patch
    loss).  Everything else, up to 8192 points per set, runs the tiled kernels (ChamferRaggedFn)."""

    @staticmethod
    def forward(ctx, pred, gt):
        _lib.require_gpu(pred, "chamfer_distance")
        _lib.count("chamfer_small")
        p = pred.float().contiguous()
        g = gt.detach().float().contiguous()
        pairs, n, _ = p.shape
        m = g.shape[1]
        dev = p.device
        ctx.in_dtype = pred.dtype
        dist = torch.empty(pairs, device=dev, dtype=torch.float32)
        i1 = torch.empty(pairs, n, device=dev, dtype=torch.uint8)
        i2 = torch.empty(pairs, m, device=dev, dtype=torch.uint8)
        _lib.call("simamba_chamfer_fwd", p, g, dist, i1, i2, pairs, n, m, device=dev)
        ctx.save_for_backward(p, g, i1, i2)
        return dist

    @staticmethod
    def backward(ctx, ddist):
        p, g, i1, i2 = ctx.saved_tensors
        pairs, n, _ = p.shape
        dd = ddist.float().contiguous()
        dp = torch.empty_like(p)
        _lib.call("simamba_chamfer_bwd", p, g, dd, i1, i2, dp, pairs, n, g.shape[1], device=p.device)
        return dp.to(ctx.in_dtype), None


_CHAMFER_REDUCTIONS = {"mean": 0, "sum": 1, None: 2}


def _pair_lengths(t, pairs, device, what):
    """A per-pair length argument as the tiled kernels read it: grouping._per_cloud's rules, then lengths_i32."""
    return lengths_i32(grouping._per_cloud(t, pairs, device, what))


class ChamferRaggedFn(torch.autograd.Function):
    """The tiled kernels with per-pair lengths, norm 1 or 2, mean / sum / no point reduction and one-way matching
    (simamba_chamfer_ragged_*; with no lengths, norm 2, mean and both ways exactly simamba_chamfer_large_*).  Returns
    dist (pairs,), or with no reduction d1 (pairs, n) and, unless one-way, d2 (pairs, m)."""

    @staticmethod
    def forward(ctx, pred, gt, xlen, ylen, norm, reduction, one_way):
        _lib.require_gpu(pred, "chamfer_distance")
        p = pred.float().contiguous()
        g = gt.detach().float().contiguous()
        pairs, n, _ = p.shape
        m = g.shape[1]
        dev = p.device
        ctx.in_dtype, ctx.gt_dtype = pred.dtype, gt.dtype
        ctx.mode = (norm, reduction, int(one_way))
        dist = torch.empty(pairs, device=dev, dtype=torch.float32) if reduction != 2 else None
        i1 = torch.empty(pairs, n, device=dev, dtype=torch.int32)
        d1 = torch.empty(pairs, n, device=dev, dtype=torch.float32)
        i2 = None if one_way else torch.empty(pairs, m, device=dev, dtype=torch.int32)
        d2 = None if one_way else torch.empty(pairs, m, device=dev, dtype=torch.float32)
        _lib.call("simamba_chamfer_ragged_fwd", p, g, xlen, ylen, dist, i1, i2, d1, d2, pairs, n, m, norm, reduction,
                  int(one_way), 0, device=dev)
        ctx.save_for_backward(p, g, i1, i2, xlen, ylen)
        if reduction != 2:
            return dist
        return d1 if one_way else (d1, d2)

    @staticmethod
    def backward(ctx, *grads):
        p, g, i1, i2, xlen, ylen = ctx.saved_tensors
        norm, reduction, one_way = ctx.mode
        pairs, n, _ = p.shape
        m = g.shape[1]
        up = [None if t is None else t.float().contiguous() for t in grads]
        if reduction != 2:
            dd, dd1, dd2 = up[0], None, None
        else:
            dd, dd1 = None, up[0]
            dd2 = None if one_way else up[1]
            if dd1 is None:
                dd1 = torch.zeros(pairs, n, device=p.device, dtype=torch.float32)
            if dd2 is None and not one_way:
                dd2 = torch.zeros(pairs, m, device=p.device, dtype=torch.float32)
        dp = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        dg = torch.empty_like(g) if ctx.needs_input_grad[1] else None
        _lib.call("simamba_chamfer_ragged_bwd", p, g, xlen, ylen, dd, dd1, dd2, i1, i2, dp, dg, pairs, n, m, norm,
                  reduction, one_way, 0, device=p.device)
        return (None if dp is None else dp.to(ctx.in_dtype)), (None if dg is None else dg.to(ctx.gt_dtype)), \
            None, None, None, None, None


def chamfer_distance(pred, gt, *, x_lengths=None, y_lengths=None, weights=None, norm=2, point_reduction="mean",
                     single_directional=False):
    """(pairs, n, 3), (pairs, m, 3) -> (pairs,): pytorch3d ``chamfer_distance(..., batch_reduction=None)[0]``, for
    sets of up to 8192 points; both arguments are differentiable.

    The keywords are pytorch3d's.  ``x_lengths`` / ``y_lengths`` (pairs,) integers: pair p is the first
    ``x_lengths[p]`` points of ``pred[p]`` against the first ``y_lengths[p]`` of ``gt[p]`` (values outside [1, n] /
    [1, m] are clamped by the kernel; the padding is never read).  ``norm`` 1 or 2; ``point_reduction`` "mean" (over
    the real points), "sum" or None, which returns the per-point ``(cham_x (pairs, n), cham_y (pairs, m))`` with zeros
    behind the lengths; ``single_directional`` drops the gt-to-pred term (``cham_y`` is None); ``weights`` (pairs,)
    scales every pair and is differentiable.  Any of them takes the tiled kernels whatever the set sizes; without
    them the call is what it always was.  No host read."""
    if norm not in (1, 2):
        raise ValueError(f"chamfer_distance: norm must be 1 or 2, got {norm!r}")
    if point_reduction == "max":
        raise NotImplementedError("chamfer_distance: point_reduction='max' is not built (mean, sum or None)")
    if point_reduction not in _CHAMFER_REDUCTIONS:
        raise ValueError(f"chamfer_distance: point_reduction must be 'mean', 'sum' or None, got {point_reduction!r}")
    one_way = bool(single_directional)
    pairs = pred.shape[0]
    xlen = _pair_lengths(x_lengths, pairs, pred.device, "chamfer_distance: x_lengths")
    ylen = _pair_lengths(y_lengths, pairs, pred.device, "chamfer_distance: y_lengths")
    if weights is not None:
        if not torch.is_tensor(weights) or weights.shape != (pairs,):
            raise ValueError(f"chamfer_distance: weights must be a tensor of shape ({pairs},)")
        if not weights.dtype.is_floating_point:
            raise TypeError(f"chamfer_distance: weights must hold floats, got {weights.dtype}")
    dense = xlen is None and ylen is None and weights is None and norm == 2 and point_reduction == "mean" \
        and not one_way
    if dense and max(pred.shape[1], gt.shape[1]) <= CHAMFER_SMALL_MAX and not gt.requires_grad:
        return ChamferFn.apply(pred, gt)
    _lib.count("chamfer_large" if dense else "chamfer_ragged")
    out = ChamferRaggedFn.apply(pred, gt, xlen, ylen, norm, _CHAMFER_REDUCTIONS[point_reduction], one_way)
    if point_reduction is not None:
        return out if weights is None else out * weights
    cham_x, cham_y = (out, None) if one_way else out
    if weights is not None:
        cham_x = cham_x * weights[:, None]
        cham_y = None if cham_y is None else cham_y * weights[:, None]
    return cham_x, cham_y
