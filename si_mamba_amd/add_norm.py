"""Fused DropPath-scaled residual add + LayerNorm (or RMSNorm) on the MI355X kernel (csrc/add_norm.hip).

Computes exactly what the reference's Block.forward does before the mixer (models/block.py:56-60):

    residual = drop_path(hidden) + residual        (or hidden when residual is None)
    normed   = LayerNorm(residual)                 (rms=True: RMSNorm(residual), no bias)

as one streaming pass forward and one backward.  ``rowscale`` is the per-sample DropPath factor
(keep-mask / keep-prob) or None.

Compact batches (``hidden_slot`` / ``normed_slot``, simamba_add_layer_norm_fwd_slots / _bwd_slots): ``hidden`` may hold
only some samples of the batch, packed -- the others take ``residual`` as it is, which is what a rowscale of 0 gives --
and ``normed`` may be produced only for some.  MixerModel uses both to run a mixer on the samples whose result the next
block's DropPath keeps (block.py).
"""
from __future__ import annotations

import torch

from . import _lib


def add_norm_bwd(dn, dro, res_out, mean, rstd, w, rs, dres, dhid, Bsz, rows, dim, hcode, ocode, flags,
                 hidden_slot=None, hidden_batch=None, normed_slot=None, normed_batch=None):
    """The add + norm backward pass (simamba_add_layer_norm_bwd_slots) into ``dres`` / ``dhid`` (either may be None);
    -> the fp32 (dweight, dbias) rows, summed over the kernel's per-workgroup partials (RMSNorm: dweight only).
    ``hidden_slot`` / ``normed_slot`` (B,) int32: ``dhid`` / ``dn`` hold ``hidden_batch`` / ``normed_batch`` samples."""
    dev = res_out.device
    grid = _lib.load().simamba_add_layer_norm_grid(Bsz, rows)
    part = torch.empty(grid, 2, dim, device=dev, dtype=torch.float32)
    hb = Bsz if hidden_slot is None else hidden_batch
    nb = Bsz if normed_slot is None else normed_batch
    _lib.call("simamba_add_layer_norm_bwd_slots", dn, dro, res_out, mean, rstd, w, rs, dres, dhid, part, hidden_slot, hb,
              normed_slot, nb, Bsz, rows, dim, hcode, ocode, flags, device=dev,
              time_as="add_rms_bwd" if flags else "add_ln_bwd")
    # RMS: only the dweight half of the partials is written
    return part[:, :1].sum(0) if flags else part.sum(0)


class AddLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, residual, weight, bias, eps, rowscale, out_dtype, rms=False, hidden_slot=None,
                hidden_dtype=None, normed_slot=None, normed_batch=None):
        # the full-size operand: hidden, or the residual when hidden is compact (None: no sample has hidden rows)
        full = hidden if hidden_slot is None else residual
        if full is None:
            raise ValueError("add_layer_norm_fn: a compact hidden (hidden_slot) goes with a residual")
        _lib.require_gpu(full, "add_layer_norm_fn")
        h = None if hidden is None else hidden.contiguous()
        Bsz, rows, dim = full.shape[0], full[0].numel() // full.shape[-1], full.shape[-1]
        shape = tuple(full.shape)
        dev = full.device
        hdtype = h.dtype if h is not None else (hidden_dtype or torch.float32)
        hb = Bsz if hidden_slot is None else (0 if h is None else h.shape[0])
        nb = Bsz if normed_slot is None else int(normed_batch)
        if h is not None and tuple(h.shape[1:]) != shape[1:]:
            raise ValueError(f"add_layer_norm_fn: hidden {tuple(h.shape)} against residual {shape}")
        hcode = _lib.dtype_code(hdtype)
        ocode = _lib.dtype_code(out_dtype)
        flags = _lib.NORM_RMS if rms else 0
        res = None if residual is None else residual.float().contiguous()
        w = weight.float().contiguous()
        b = None if bias is None else bias.float().contiguous()
        rs = None if (rowscale is None or res is None) else rowscale.float().contiguous()
        alias = res is None and hdtype == torch.float32        # residual_out is hidden itself
        res_out = h if alias else torch.empty(shape, device=dev, dtype=torch.float32)
        normed = torch.empty((nb,) + shape[1:], device=dev, dtype=out_dtype)
        mean = None if rms else torch.empty(Bsz * rows, device=dev, dtype=torch.float32)   # RMSNorm has no mean
        rstd = torch.empty(Bsz * rows, device=dev, dtype=torch.float32)
        _lib.call("simamba_add_layer_norm_fwd_slots", h, res, rs, w, b, None if alias else res_out, normed, mean, rstd,
                  hidden_slot, hb, normed_slot, nb, Bsz, rows, dim, float(eps), hcode, ocode, flags, device=dev,
                  time_as="add_rms_fwd" if rms else "add_ln_fwd")
        ctx.save_for_backward(res_out, mean, rstd, w, rs, hidden_slot, normed_slot)
        ctx.meta = (Bsz, rows, dim, hcode, ocode, hdtype, residual is not None,
                    None if residual is None else residual.dtype, weight.dtype, bias is not None, flags, hb, nb)
        return normed, res_out

    @staticmethod
    def backward(ctx, dnormed, dres_out):
        res_out, mean, rstd, w, rs, hidden_slot, normed_slot = ctx.saved_tensors
        Bsz, rows, dim, hcode, ocode, hdtype, has_res, res_dtype, wdtype, has_bias, flags, hb, nb = ctx.meta
        dev = res_out.device
        dn = dnormed.contiguous()
        dro = None if dres_out is None else dres_out.float().contiguous()
        # gradient w.r.t. residual (fp32) and w.r.t. hidden; they are the same tensor unless DropPath rescales
        # hidden, hidden is not fp32 or hidden is compact (then dhidden is: the mapped samples, at their slots)
        need_split = (rs is not None) or (hdtype != torch.float32) or not has_res or hidden_slot is not None
        dres = torch.empty(res_out.shape, device=dev, dtype=torch.float32) if has_res else None
        dhid = torch.empty((hb,) + tuple(res_out.shape[1:]), device=dev, dtype=hdtype) if need_split and hb else None
        dwb = add_norm_bwd(dn, dro, res_out, mean, rstd, w, rs, dres, dhid, Bsz, rows, dim, hcode, ocode, flags,
                           hidden_slot, hb, normed_slot, nb)
        if dhid is None and hidden_slot is None:
            dhid = dres
        return (dhid, None if not has_res else dres.to(res_dtype), dwb[0].to(wdtype),
                dwb[1].to(wdtype) if has_bias else None, None, None, None, None, None, None, None, None)


def add_layer_norm_fn(hidden, residual, weight, bias, eps=1e-5, rowscale=None, out_dtype=None, rms=False, *,
                      hidden_slot=None, hidden_dtype=None, normed_slot=None, normed_batch=None):
    """-> (normed, residual_out).  hidden: (B, ..., dim); residual: same shape or None; rowscale: (B,) or None.
    ``rms=True``: RMSNorm (``bias`` must be None) in place of LayerNorm.

    Compact batches.  ``hidden_slot`` (B,) int32 on the device: ``hidden`` is (n, ..., dim) with n <= B and sample b's
    rows are ``hidden[hidden_slot[b]]``; -1: the sample has none and ``residual_out[b] = residual[b]``.  ``hidden`` may
    be None when no sample has any (``hidden_dtype``: the dtype it would have had).  The gradient w.r.t. ``hidden`` is
    compact in the same way.  ``normed_slot`` (B,) int32 with ``normed_batch``: ``normed`` comes out as
    (normed_batch, ..., dim) holding sample b at ``normed_slot[b]``; samples at -1 get none (and no gradient flows into
    the norm through them).  ``residual_out`` always holds the whole batch."""
    if rms and bias is not None:
        raise ValueError("add_layer_norm_fn(rms=True): RMSNorm takes no bias")
    if normed_slot is not None and normed_batch is None:
        raise ValueError("add_layer_norm_fn: normed_slot goes with normed_batch")
    if out_dtype is None:
        out_dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else weight.dtype
    return AddLayerNormFn.apply(hidden, residual, weight, bias, eps, rowscale, out_dtype, bool(rms), hidden_slot,
                                hidden_dtype, normed_slot, normed_batch)


def add_rms_norm_fn(hidden, residual, weight, eps=1e-5, rowscale=None, out_dtype=None):
    """add_layer_norm_fn with RMSNorm: -> (normed, residual_out)."""
    return add_layer_norm_fn(hidden, residual, weight, None, eps, rowscale=rowscale, out_dtype=out_dtype, rms=True)
