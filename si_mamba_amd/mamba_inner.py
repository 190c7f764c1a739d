"""Fused mixer body: conv1d -> x_proj -> dt_proj -> selective scan -> out_proj, one autograd node.

Counterpart of ``mamba_ssm.ops.selective_scan_interface.mamba_inner_fn`` (the fast path the
reference's mixer takes when called from models/block.py:72).  Compared with chaining the separate
ops it never copies an activation-sized tensor:

  * ``x`` and ``z`` are the two halves of the in_proj output ``xz (B, 2D, L)``; the HIP kernels read
    them in place through a batch stride, and the backward writes ``dx`` / ``dz`` straight into the
    halves of ONE ``dxz`` buffer (no ``chunk`` / ``cat`` / ``contiguous``);
  * ``B_t`` / ``C_t`` are read out of the x_proj output ``(B, L, R+2N)`` through strides;
  * every GEMM is issued in the orientation that yields an L-contiguous ``(B, *, L)`` result, so no
    transposition kernel runs.

Hand-written MFMA kernels: conv1d + SiLU -> x_proj (-> dt_proj) (csrc/xdt_proj.hip, xdt_proj_bf16.hip), and under bf16
compute in_proj / out_proj's input gradient (csrc/in_proj_bf16.hip, via tokens_times_weight) and out_proj fused with the
next block's add + LayerNorm (out_norm.py).  The fp32 in_proj / out_proj and the remaining backward products are library
GEMMs (hipBLASLt / rocBLAS through torch.bmm).
"""
from __future__ import annotations

import torch

from . import _lib


def _w(t, dtype):
    return t if t.dtype == dtype else t.to(dtype)


# GEMM helpers.  torch.matmul folds a (2-D weight) x (3-D activation) product into one mm on a
# reshaped view; with L-contiguous (B, D, L) activations that reshape is a 200-800 MB copy per call
# (measured: 12 strided-copy launches, 27 % of a block's GPU time).  torch.bmm with the weight
# expanded over the batch (batch stride 0) keeps every operand in place and yields the L-contiguous /
# token-contiguous result directly.
def _wx(W, X):
    """W (M, K) applied to every X[b] (K, N) -> (B, M, N)."""
    return torch.bmm(W.unsqueeze(0).expand(X.shape[0], -1, -1), X)


def _xw(X, W):
    """every X[b] (M, K) times W (K, N) -> (B, M, N)."""
    return torch.bmm(X, W.unsqueeze(0).expand(X.shape[0], -1, -1))


def _sum_bmm(X, Y):
    """sum_b X[b] (M, K) @ Y[b] (K, N) -> (M, N): a weight gradient.  The batch sum accumulates and RETURNS fp32 (for
    16-bit operands too: the parameters it goes to are fp32 under autocast, so the cast kernel that would follow -- one
    launch per weight, layer and step -- never runs, and the sum of 64 partials is not rounded to bf16 first)."""
    return torch.bmm(X, Y).sum(0, dtype=torch.float32)


class InProjFn(torch.autograd.Function):
    """xz = W_in @ hidden^T as (B, 2D, L), L contiguous (+ optional bias)."""

    @staticmethod
    def forward(ctx, hidden, weight, bias):
        io = hidden.dtype
        if torch.is_autocast_enabled("cuda"):
            io = torch.get_autocast_dtype("cuda")
            hidden = hidden.to(io)
        wc = _w(weight, io)
        xz = tokens_times_weight(hidden, wc) if bias is None else _wx(wc, hidden.transpose(1, 2))
        if bias is not None:
            xz = xz + _w(bias, io)[None, :, None]
        ctx.save_for_backward(hidden, weight)
        ctx.wc = wc                     # the weight in compute dtype: not cast a second time in backward
        ctx.has_bias = bias is not None
        return xz

    @staticmethod
    def backward(ctx, dxz):
        hidden, weight = ctx.saved_tensors
        io = hidden.dtype
        dxz = dxz.to(io)
        dh = _xw(dxz.transpose(1, 2), ctx.wc) if ctx.needs_input_grad[0] else None            # (B, L, d)
        dw = _sum_bmm(dxz, hidden).to(weight.dtype) if ctx.needs_input_grad[1] else None     # (2D, d)
        db = dxz.sum((0, 2)).to(weight.dtype) if ctx.has_bias else None
        return dh, dw, db


def tokens_times_weight(x, w):
    """out[b, j, t] = sum_c w[j, c] x[b, t, c]: token-major (B, L, C) activations against a row-major (M, C) weight, result
    (B, M, L) with L contiguous -- the shape of in_proj's forward and of out_proj's input gradient.  bf16 operands whose
    grid fills the chip go through the hand-written kernels (csrc/in_proj_bf16.hip, csrc/in_proj_f32.hip), anything else
    through the library."""
    if (x.dtype in (torch.bfloat16, torch.float32) and w.dtype == x.dtype and x.is_cuda and x.dim() == 3
            and x.is_contiguous() and in_proj_hand_ok(x, w)):
        Bsz, L, C = x.shape
        wcc = w.contiguous()
        out = torch.empty(Bsz, w.shape[0], L, device=x.device, dtype=x.dtype)
        _lib.call("simamba_in_proj_fwd", x, wcc, out, Bsz, L, C, w.shape[0], _lib.dtype_code(x.dtype),
                  device=x.device, time_as="in_proj_fwd")
        _lib.count("in_proj_hand")
        return out
    return _wx(w, x.transpose(1, 2))


def in_proj_hand_ok(hidden, wc):
    """Shapes the hand-written in_proj kernel takes (include/simamba.h) and grids that fill the chip."""
    Bsz, L, C = hidden.shape
    tile = 128 if hidden.dtype == torch.float32 else 256       # tokens per workgroup
    return (C % 64 == 0 and C <= 384 and wc.shape[0] % 32 == 0 and L % 8 == 0 and hidden.data_ptr() % 16 == 0
            and _lib.in_proj_hand_enabled(Bsz * ((L + tile - 1) // tile), hidden.dtype))


def in_proj_fn(hidden, weight, bias=None):
    return InProjFn.apply(hidden, weight, bias)


def xdt_proj_fused_ok(x, wx, wdt, conv=False):
    """Shapes / dtypes the hand-written MFMA kernels take (include/simamba.h; fp32 and bf16, weights in the
    activations' type); anything else runs the two library GEMMs (and, with ``conv``, the separate conv kernel)."""
    S, D = wx.shape
    R = wdt.shape[1]
    pack = 4 if x.dtype == torch.float32 else 8
    return (x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and wx.dtype == x.dtype and wdt.dtype == x.dtype
            and x.dim() == 3 and x.stride(2) == 1 and x.stride(1) == x.shape[2] and x.stride(0) % pack == 0
            and x.shape[1] == D and D % 64 == 0 and x.shape[2] % pack == 0 and S % 4 == 0 and S <= 64
            and D * x.shape[2] * 4 < 2 ** 32 - 65536 and (not conv or D <= 1024)
            and R % 4 == 0 and 4 <= R <= 24 and S >= R and wdt.shape[0] == D and x.data_ptr() % 16 == 0)


def xdt_proj_fwd(x, wx, wdt, conv=None, want_delta=True):
    """x (B, D, L) fp32 or bf16 (batch-strided views allowed), wx (S, D), wdt (D, R) -> x_dbl (B, L, S) token-major, delta
    (B, D, L) -- or None with ``want_delta=False``: the delta product is then left to the scan kernels
    (simamba_selective_scan_dt_fwd).  ``conv=(w (D, 4) fp32, bias (D) or None, out (B, D, L))``: the causal depthwise
    conv1d + SiLU is applied to x on the way in and its result written to ``out``.  No autograd: called from inside
    MambaInnerFn.forward, whose backward differentiates the products itself."""
    Bsz, D, L = x.shape
    S, R = wx.shape[0], wdt.shape[1]
    wxc, wdc = wx.contiguous(), wdt.contiguous()
    x_dbl = torch.empty(Bsz, L, S, device=x.device, dtype=x.dtype)
    delta = torch.empty(Bsz, D, L, device=x.device, dtype=x.dtype) if want_delta else None
    if conv is None:
        _lib.call("simamba_xdt_proj_fwd", x, wxc, wdc, x_dbl, delta, Bsz, D, L, S, R, _lib.dtype_code(x.dtype),
                  x.stride(0), device=x.device, time_as="xdt_proj_fwd")
    else:
        cw, cb, out = conv
        _lib.call("simamba_conv_xdt_proj_fwd", x, cw, cb, wxc, wdc, out, x_dbl, delta, Bsz, D, L, S, R,
                  _lib.dtype_code(x.dtype), x.stride(0), device=x.device, time_as="xdt_proj_fwd")
    return x_dbl, delta


class MambaInnerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xz, conv_w, conv_b, x_proj_w, dt_proj_w, out_proj_w, out_proj_b, A, D, delta_bias,
                dt_rank, d_state, grad_mode=True):
        _lib.require_gpu(xz, "mamba_inner_fn")
        if xz.stride(2) != 1 or xz.stride(1) != xz.shape[2]:
            xz = xz.contiguous()
        io = xz.dtype
        code = _lib.dtype_code(io)
        Bsz, twoD, L = xz.shape
        Dm = twoD // 2
        R, N = dt_rank, d_state
        S = R + 2 * N
        dev = xz.device
        xbs = xz.stride(0)
        x_in, z = xz[:, :Dm], xz[:, Dm:]

        cw = conv_w.float().contiguous()
        cb = None if conv_b is None else conv_b.float().contiguous()
        Af = A.float().contiguous()
        Df = None if D is None else D.float().contiguous()
        bf = None if delta_bias is None else delta_bias.float().contiguous()
        W = cw.shape[1]

        # out_proj_w None: the caller applies out_proj itself (out_norm.py fuses it with the next block's add +
        # LayerNorm) and this node returns the gated scan output y (B, D, L)
        no_out = out_proj_w is None
        xw_c, dtw_c = _w(x_proj_w, io), _w(dt_proj_w, io)                             # compute-dtype weights,
        ow_c = None if no_out else _w(out_proj_w, io)
        ctx.wcast = (xw_c, dtw_c, ow_c)                                               # reused by backward
        x_conv = torch.empty(Bsz, Dm, L, device=dev, dtype=io)
        # (ctx.needs_input_grad is True under torch.no_grad() too: the caller's grad mode comes in as an argument)
        need_grad = grad_mode and any(ctx.needs_input_grad)
        pack = 4 if io == torch.float32 else 8
        ckpt_step, x_ckpt = _lib.scan_plan(Bsz, Dm, L, N, io, dev, need_grad, **_lib.mixer_scan_operands(
            xz.data_ptr(), Af.data_ptr(), Dm, L, R, N, xz.element_size(), xbs))
        # Where both scan directions run the lanes-per-channel kernels (scan_plan: CKPT_SEQ) those kernels can form
        # delta = dt_proj.weight @ dt themselves on the matrix pipe, and the (B, D, L) delta tensor never exists: one
        # write and two reads of it per layer and step less (csrc/scan_fwd_seq.hip, csrc/scan_bwd_seq.hip).  Taken
        # for bf16 I/O, where it is faster; measured slower in fp32 (_lib.fuse_dt_enabled)
        fuse_dt = (_lib.fuse_dt_enabled(io) and ckpt_step == _lib.CKPT_SEQ and N == 16 and R % pack == 0 and R <= 24
                   and _lib.current_scan_variant() != _lib.SCAN_ROWSCAN)
        if W == 4 and xdt_proj_fused_ok(x_in, xw_c, dtw_c, conv=True):
            # conv1d + SiLU -> x_proj (-> dt_proj) as ONE pass over the x half of xz on the matrix cores
            # (csrc/xdt_proj.hip); x_conv is written as a by-product for the scan and the backward
            x_dbl, delta = xdt_proj_fwd(x_in, xw_c, dtw_c, conv=(cw, cb, x_conv), want_delta=not fuse_dt)
            _lib.count("xdt_conv_fused")
        else:
            fuse_dt = False
            _lib.call("simamba_causal_conv1d_fwd", x_in, cw, cb, x_conv, Bsz, Dm, L, W, 1, code, xbs,
                      device=dev, time_as="conv1d_fwd")
            if xdt_proj_fused_ok(x_conv, xw_c, dtw_c):
                x_dbl, delta = xdt_proj_fwd(x_conv, xw_c, dtw_c)
                _lib.count("xdt_fused")
            else:
                _lib.count("xdt_gemm")
                x_dbl = _xw(x_conv.transpose(1, 2), xw_c.t())                          # (B, L, S)
                delta = _wx(dtw_c, x_dbl[:, :, :R].transpose(1, 2))                    # (B, D, L)
        Bv, Cv = x_dbl[:, :, R:R + N], x_dbl[:, :, R + N:]                            # (B, L, N) views
        if x_dbl.data_ptr() % 16 or not x_dbl.is_contiguous():
            raise RuntimeError("mamba_inner_fn: x_proj output not as planned")         # the allocator never does this

        y = torch.empty(Bsz, Dm, L, device=dev, dtype=io)
        dtw_k = dtw_c.contiguous() if fuse_dt else None
        if fuse_dt:
            _lib.count("scan_dt_fwd")
            _lib.call("simamba_selective_scan_dt_fwd", x_conv, x_dbl, dtw_k, Af, Df, z, bf, y, x_ckpt, None,
                      Bsz, Dm, L, N, R, code, xbs, x_dbl.stride(0), x_dbl.stride(1),
                      ckpt_step, _lib.current_scan_variant(), device=dev, time_as="scan_fwd")
        else:
            _lib.call("simamba_selective_scan_fwd", x_conv, delta, Af, Bv, Cv, Df, z, bf, y, x_ckpt, None,
                      Bsz, Dm, L, N, code, 1, xbs, x_dbl.stride(0), 1, x_dbl.stride(1),
                      ckpt_step, _lib.current_scan_variant(), device=dev, time_as="scan_fwd")

        if no_out:
            out = y
        else:
            out = _xw(y.transpose(1, 2), ow_c.t())                                     # (B, L, d)
            if out_proj_b is not None:
                out = out + _w(out_proj_b, io)
        ctx.no_out = no_out
        ctx.dims = (R, N, W)
        ctx.ckpt_step = ckpt_step
        ctx.dtw_k = dtw_k                                   # not None: delta was formed inside the scan (no tensor)
        ctx.has_out_bias = out_proj_b is not None and not no_out
        ctx.param_dtypes = (conv_w.dtype, None if conv_b is None else conv_b.dtype, x_proj_w.dtype,
                            dt_proj_w.dtype, None if no_out else out_proj_w.dtype, A.dtype,
                            None if D is None else D.dtype, None if delta_bias is None else delta_bias.dtype)
        ctx.save_for_backward(xz, x_conv, x_dbl, delta, None if no_out else y, cw, cb, x_proj_w, dt_proj_w, out_proj_w,
                              Af, Df, bf, x_ckpt)
        return out

    @staticmethod
    def backward(ctx, dout):
        (xz, x_conv, x_dbl, delta, y, cw, cb, x_proj_w, dt_proj_w, out_proj_w, Af, Df, bf, x_ckpt) = ctx.saved_tensors
        lib = _lib.load()
        R, N, W = ctx.dims
        io = xz.dtype
        code = _lib.dtype_code(io)
        Bsz, twoD, L = xz.shape
        Dm = twoD // 2
        S = R + 2 * N
        dev = xz.device
        xbs = xz.stride(0)
        dout = dout.to(io)
        f32 = dict(device=dev, dtype=torch.float32)
        xw_c, dtw_c, ow_c = ctx.wcast
        if ctx.no_out:                                                                # the gradient IS dy (B, D, L)
            dy = dout.contiguous()
            d_out_w = d_out_b = None
        else:
            if dout.stride(2) != 1:
                dout = dout.contiguous()
            # out_proj
            d_out_w = _sum_bmm(dout.transpose(1, 2), y.transpose(1, 2))               # (d, D)
            d_out_b = dout.sum((0, 1)) if ctx.has_out_bias else None
            dy = tokens_times_weight(dout, ow_c.t())                                  # (B, D, L)

        # selective scan
        dxz = torch.empty_like(xz)
        du = torch.empty(Bsz, Dm, L, device=dev, dtype=io)
        ddelta = torch.empty(Bsz, Dm, L, device=dev, dtype=io)
        # the five fp32 accumulators of the scan backward are carved back to back out of one allocation: the
        # library zeroes exactly-adjacent spans with a single memset node
        dA, dB, dC, dD, dbias = _lib.scan_bwd_accumulators(Bsz, Dm, L, N, Df is not None, bf is not None, dev)
        Bv, Cv = x_dbl[:, :, R:R + N], x_dbl[:, :, R + N:]
        z, dz = xz[:, Dm:], dxz[:, Dm:]
        # deterministic: partials + fixed-order sums instead of float atomics
        flags, ws, nws = _lib.det_args(lib.simamba_scan_bwd_workspace_floats, Bsz, Dm, L, N,
                                       _lib.CKPT_SEQ if ctx.dtw_k is not None else ctx.ckpt_step, device=dev)
        _lib.count("scan_bwd_det" if flags else "scan_bwd_atomic")
        if ctx.dtw_k is not None:
            _lib.call("simamba_selective_scan_dt_bwd_ex", x_conv, x_dbl, ctx.dtw_k, Af, Df, z, bf, dy, x_ckpt,
                      du, ddelta, dA, dB, dC, dD, dz, dbias, Bsz, Dm, L, N, R, code,
                      xbs, dxz.stride(0), x_dbl.stride(0), x_dbl.stride(1), flags, ws, nws,
                      device=dev, time_as="scan_bwd")
        else:
            _lib.call("simamba_selective_scan_bwd_ex", x_conv, delta, Af, Bv, Cv, Df, z, bf, dy, x_ckpt,
                      du, ddelta, dA, dB, dC, dD, dz, dbias, Bsz, Dm, L, N, code, 1,
                      xbs, dxz.stride(0), x_dbl.stride(0), 1, x_dbl.stride(1), ctx.ckpt_step, flags, ws, nws,
                      device=dev, time_as="scan_bwd")

        # dt_proj / x_proj
        dx_dbl = torch.empty(Bsz, L, S, device=dev, dtype=io)
        dx_dbl[:, :, :R].copy_(_xw(ddelta.transpose(1, 2), dtw_c))
        # dB | dC (two adjacent (B, N, L) blocks of the accumulator allocation, _lib.scan_bwd_accumulators) into the
        # token-major columns [R, S) in one strided copy
        dBC = torch.as_strided(dB, (2, Bsz, N, L), (Bsz * N * L, N * L, L, 1))
        dx_dbl[:, :, R:].view(Bsz, L, 2, N).copy_(dBC.permute(1, 3, 0, 2))
        d_dt_w = _sum_bmm(ddelta, x_dbl[:, :, :R])                                     # (D, R)
        d_x_w = _sum_bmm(dx_dbl.transpose(1, 2), x_conv.transpose(1, 2))               # (S, D)
        # dx_conv = du + x_proj_w^T @ dx_dbl^T, accumulated in place by the GEMM (beta = 1)
        wxT = xw_c.t().unsqueeze(0).expand(Bsz, -1, -1)
        torch.baddbmm(du, wxT, dx_dbl.transpose(1, 2), out=du)

        # conv1d: dx goes straight into the first half of dxz
        # taps and bias gradients carved from one allocation: the library clears adjacent accumulators with one memset
        dconv = torch.empty(Dm * W + (Dm if cb is not None else 0), **f32)
        dcw = dconv[:Dm * W].view(Dm, W)
        dcb = dconv[Dm * W:] if cb is not None else None
        flags, ws, nws = _lib.det_args(lib.simamba_causal_conv1d_bwd_workspace_floats, Bsz, Dm, L, W, device=dev)
        _lib.count("conv1d_bwd_det" if flags else "conv1d_bwd_atomic")
        _lib.call("simamba_causal_conv1d_bwd_ex", xz, cw, cb, du, dxz, dcw, dcb, Bsz, Dm, L, W, 1, code,
                  xbs, dxz.stride(0), flags, ws, nws, device=dev, time_as="conv1d_bwd")

        t_cw, t_cb, t_xw, t_dtw, t_ow, t_A, t_D, t_b = ctx.param_dtypes
        return (dxz, dcw.to(t_cw), None if dcb is None else dcb.to(t_cb), d_x_w.to(t_xw), d_dt_w.to(t_dtw),
                None if d_out_w is None else d_out_w.to(t_ow),
                None if d_out_b is None else d_out_b.to(out_proj_w.dtype), dA.to(t_A),
                None if dD is None else dD.to(t_D), None if dbias is None else dbias.to(t_b), None, None, None)


def mamba_inner_fn(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight,
                   out_proj_bias, A, D=None, delta_bias=None, dt_rank=None, d_state=None):
    """xz: (B, 2D, L); conv1d_weight: (D, W) or (D, 1, W); returns (B, L, d_model) -- or, with ``out_proj_weight=None``
    (beyond upstream's signature), the gated scan output y (B, D, L) that out_proj would be applied to.

    ``B``/``C`` are always input-dependent (taken from x_proj), delta_softplus is always on: the only
    configuration the reference's mixer uses.
    """
    if conv1d_weight.dim() == 3:
        conv1d_weight = conv1d_weight.squeeze(1)
    if dt_rank is None:
        dt_rank = delta_proj_weight.shape[1]
    if d_state is None:
        d_state = (x_proj_weight.shape[0] - dt_rank) // 2
    return MambaInnerFn.apply(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight,
                              out_proj_bias, A, D, delta_bias, dt_rank, d_state, torch.is_grad_enabled())
