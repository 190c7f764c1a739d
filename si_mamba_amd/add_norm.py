"""Fused DropPath-scaled residual add + LayerNorm (or RMSNorm) on the MI355X kernel (csrc/add_norm.hip).

Computes exactly what the reference's Block.forward does before the mixer (models/block.py:56-60):

    residual = drop_path(hidden) + residual        (or hidden when residual is None)
    normed   = LayerNorm(residual)                 (rms=True: RMSNorm(residual), no bias)

as one streaming pass forward and one backward.  ``rowscale`` is the per-sample DropPath factor
(keep-mask / keep-prob) or None.
"""
from __future__ import annotations

import torch

from . import _lib


def add_norm_bwd(dn, dro, res_out, mean, rstd, w, rs, dres, dhid, Bsz, rows, dim, hcode, ocode, flags):
    """The add + norm backward pass (simamba_add_layer_norm_bwd_ex) into ``dres`` / ``dhid`` (either may be None);
    -> the fp32 (dweight, dbias) rows, summed over the kernel's per-workgroup partials (RMSNorm: dweight only)."""
    dev = res_out.device
    grid = _lib.load().simamba_add_layer_norm_grid(Bsz, rows)
    part = torch.empty(grid, 2, dim, device=dev, dtype=torch.float32)
    _lib.call("simamba_add_layer_norm_bwd_ex", dn, dro, res_out, mean, rstd, w, rs, dres, dhid, part, Bsz, rows, dim,
              hcode, ocode, flags, device=dev, time_as="add_rms_bwd" if flags else "add_ln_bwd")
    # RMS: only the dweight half of the partials is written
    return part[:, :1].sum(0) if flags else part.sum(0)


class AddLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, residual, weight, bias, eps, rowscale, out_dtype, rms=False):
        _lib.require_gpu(hidden, "add_layer_norm_fn")
        h = hidden.contiguous()
        Bsz, rows, dim = h.shape[0], h[0].numel() // h.shape[-1], h.shape[-1]
        dev = h.device
        hcode = _lib.dtype_code(h.dtype)
        ocode = _lib.dtype_code(out_dtype)
        flags = _lib.NORM_RMS if rms else 0
        res = None if residual is None else residual.float().contiguous()
        w = weight.float().contiguous()
        b = None if bias is None else bias.float().contiguous()
        rs = None if (rowscale is None or res is None) else rowscale.float().contiguous()
        alias = res is None and h.dtype == torch.float32        # residual_out is hidden itself
        res_out = h if alias else torch.empty(h.shape, device=dev, dtype=torch.float32)
        normed = torch.empty(h.shape, device=dev, dtype=out_dtype)
        mean = None if rms else torch.empty(Bsz * rows, device=dev, dtype=torch.float32)   # RMSNorm has no mean
        rstd = torch.empty(Bsz * rows, device=dev, dtype=torch.float32)
        _lib.call("simamba_add_layer_norm_fwd_ex", h, res, rs, w, b, None if alias else res_out, normed, mean, rstd,
                  Bsz, rows, dim, float(eps), hcode, ocode, flags, device=dev,
                  time_as="add_rms_fwd" if rms else "add_ln_fwd")
        ctx.save_for_backward(res_out, mean, rstd, w, rs)
        ctx.meta = (Bsz, rows, dim, hcode, ocode, h.dtype, residual is not None,
                    None if residual is None else residual.dtype, weight.dtype, bias is not None, flags)
        return normed, res_out

    @staticmethod
    def backward(ctx, dnormed, dres_out):
        res_out, mean, rstd, w, rs = ctx.saved_tensors
        Bsz, rows, dim, hcode, ocode, hdtype, has_res, res_dtype, wdtype, has_bias, flags = ctx.meta
        dev = res_out.device
        dn = dnormed.contiguous()
        dro = None if dres_out is None else dres_out.float().contiguous()
        # gradient w.r.t. residual (fp32) and w.r.t. hidden; they are the same tensor unless DropPath rescales
        # hidden or hidden is not fp32
        need_split = (rs is not None) or (hdtype != torch.float32) or not has_res
        dres = torch.empty(res_out.shape, device=dev, dtype=torch.float32) if has_res else None
        dhid = torch.empty(res_out.shape, device=dev, dtype=hdtype) if need_split else None
        dwb = add_norm_bwd(dn, dro, res_out, mean, rstd, w, rs, dres, dhid, Bsz, rows, dim, hcode, ocode, flags)
        if dhid is None:
            dhid = dres
        return (dhid, None if not has_res else dres.to(res_dtype), dwb[0].to(wdtype),
                dwb[1].to(wdtype) if has_bias else None, None, None, None, None)


def add_layer_norm_fn(hidden, residual, weight, bias, eps=1e-5, rowscale=None, out_dtype=None, rms=False):
    """-> (normed, residual_out).  hidden: (B, ..., dim); residual: same shape or None; rowscale: (B,) or None.
    ``rms=True``: RMSNorm (``bias`` must be None) in place of LayerNorm."""
    if rms and bias is not None:
        raise ValueError("add_layer_norm_fn(rms=True): RMSNorm takes no bias")
    if out_dtype is None:
        out_dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else weight.dtype
    return AddLayerNormFn.apply(hidden, residual, weight, bias, eps, rowscale, out_dtype, bool(rms))


def add_rms_norm_fn(hidden, residual, weight, eps=1e-5, rowscale=None, out_dtype=None):
    """add_layer_norm_fn with RMSNorm: -> (normed, residual_out)."""
    return add_layer_norm_fn(hidden, residual, weight, None, eps, rowscale=rowscale, out_dtype=out_dtype, rms=True)
