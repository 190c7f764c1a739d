"""selective_scan_fn on the MI355X kernels.

Mirrors the operator the reference's mixer uses
(``mamba_ssm.ops.selective_scan_interface.selective_scan_fn``; reached from
reference models/block.py:72 through the Mamba built at models/point_mamba.py:162):
same argument names, meaning and return values.
"""
from __future__ import annotations

import torch

from . import _lib


def _rows_contiguous(t):
    """(B, D, L) view whose (D, L) planes are dense: only the batch stride may differ."""
    return t.dim() == 3 and t.stride(2) == 1 and t.stride(1) == t.shape[2]


def _bc_bnl(M, name):
    if M.dim() == 4:
        if M.shape[1] != 1:
            raise ValueError(f"{name}: only ngroups == 1 is supported (got {tuple(M.shape)})")
        return M[:, 0], True
    if M.dim() != 3:
        raise ValueError(f"{name} must be (batch, dstate, seqlen) or (batch, 1, dstate, seqlen)")
    return M, False


class SelectiveScanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, delta, A, B, C, D=None, z=None, delta_bias=None,
                delta_softplus=False, return_last_state=False, grad_mode=True):
        _lib.require_gpu(u, "selective_scan_fn")
        io = u.dtype
        code = _lib.dtype_code(io)
        if A.is_complex():
            raise NotImplementedError("complex A is not on the SI-Mamba path")
        B3, ctx.b_grouped = _bc_bnl(B, "B")
        C3, ctx.c_grouped = _bc_bnl(C, "C")
        batch, dim, L = u.shape
        N = A.shape[1]
        if A.shape[0] != dim or B3.shape != (batch, N, L) or C3.shape != (batch, N, L):
            raise ValueError("selective_scan_fn: inconsistent shapes")
        uc = u.contiguous()
        dc = delta.to(io).contiguous()
        Ac = A.float().contiguous()
        # B, C are read through their strides (no transposition copy) when both share them
        Bc, Cc = B3.to(io), C3.to(io)
        if Bc.stride() != Cc.stride() or min(Bc.stride()) < 0:
            Bc, Cc = Bc.contiguous(), Cc.contiguous()
        Dc = None if D is None else D.float().contiguous()
        zc = None if z is None else z.to(io)
        if zc is not None and not _rows_contiguous(zc):
            zc = zc.contiguous()
        bc = None if delta_bias is None else delta_bias.float().contiguous()
        out = torch.empty_like(uc)
        # ctx.needs_input_grad is True under torch.no_grad() too: the caller's grad mode comes in as an argument
        needs_grad = grad_mode and any(ctx.needs_input_grad)
        # out and the backward's dout / du / ddelta / dz are fresh contiguous allocations (16-byte aligned)
        addr_or = uc.data_ptr() | dc.data_ptr() | (0 if zc is None else zc.data_ptr())
        ckpt_step, x_ckpt = _lib.scan_plan(batch, dim, L, N, io, u.device, needs_grad, softplus=delta_softplus,
                                           has_z=zc is not None, act_addr_or=addr_or, a_addr=Ac.data_ptr(),
                                           b_addr=Bc.data_ptr(), c_addr=Cc.data_ptr(),
                                           z_bs=0 if zc is None else zc.stride(0), bc_strides=Bc.stride())
        last = (torch.empty(batch, dim, N, device=u.device, dtype=torch.float32)
                if return_last_state else None)
        _lib.call("simamba_selective_scan_fwd", uc, dc, Ac, Bc, Cc, Dc, zc, bc, out, x_ckpt, last,
                  batch, dim, L, N, code, int(bool(delta_softplus)),
                  0 if zc is None else zc.stride(0), Bc.stride(0), Bc.stride(1), Bc.stride(2),
                  ckpt_step, _lib.current_scan_variant(), device=u.device, time_as="scan_fwd")
        ctx.delta_softplus = bool(delta_softplus)
        ctx.ckpt_step = ckpt_step
        ctx.has = (D is not None, z is not None, delta_bias is not None)
        ctx.in_dtypes = (delta.dtype, B.dtype, C.dtype,
                         None if D is None else D.dtype,
                         None if z is None else z.dtype,
                         None if delta_bias is None else delta_bias.dtype, A.dtype)
        ctx.save_for_backward(uc, dc, Ac, Bc, Cc, Dc, zc, bc, x_ckpt)
        if return_last_state:
            ctx.mark_non_differentiable(last)
            return out, last
        return out

    @staticmethod
    def backward(ctx, dout, *unused):
        uc, dc, Ac, Bc, Cc, Dc, zc, bc, x_ckpt = ctx.saved_tensors
        lib = _lib.load()
        batch, dim, L = uc.shape
        N = Ac.shape[1]
        io = uc.dtype
        dout = dout.to(io).contiguous()
        du = torch.empty_like(uc)
        ddelta = torch.empty_like(uc)
        dz = torch.empty_like(uc) if zc is not None else None
        dA, dB, dC, dD, dbias = _lib.scan_bwd_accumulators(batch, dim, L, N, Dc is not None, bc is not None,
                                                           uc.device)
        # deterministic: partials + fixed-order sum instead of float atomics
        flags, ws, nws = _lib.det_args(lib.simamba_scan_bwd_workspace_floats, batch, dim, L, N, ctx.ckpt_step,
                                       device=uc.device)
        _lib.count("scan_bwd_det" if flags else "scan_bwd_atomic")
        _lib.call("simamba_selective_scan_bwd_ex", uc, dc, Ac, Bc, Cc, Dc, zc, bc, dout, x_ckpt,
                  du, ddelta, dA, dB, dC, dD, dz, dbias, batch, dim, L, N, _lib.dtype_code(io),
                  int(ctx.delta_softplus), 0 if zc is None else zc.stride(0), 0,
                  Bc.stride(0), Bc.stride(1), Bc.stride(2), ctx.ckpt_step, flags, ws, nws,
                  device=uc.device, time_as="scan_bwd")
        dt_delta, dt_B, dt_C, dt_D, dt_z, dt_bias, dt_A = ctx.in_dtypes
        dB = dB.to(dt_B)
        dC = dC.to(dt_C)
        if ctx.b_grouped:
            dB = dB.unsqueeze(1)
        if ctx.c_grouped:
            dC = dC.unsqueeze(1)
        return (du, ddelta.to(dt_delta), dA.to(dt_A), dB, dC,
                None if dD is None else dD.to(dt_D),
                None if dz is None else dz.to(dt_z),
                None if dbias is None else dbias.to(dt_bias),
                None, None, None)


def selective_scan_fn(u, delta, A, B, C, D=None, z=None, delta_bias=None,
                      delta_softplus=False, return_last_state=False):
    """u, delta, z: (B, D, L); A: (D, N); B, C: (B, N, L) or (B, 1, N, L); D, delta_bias: (D).

    Returns out (B, D, L) in u's dtype, plus last_state (B, D, N) fp32 when asked.
    """
    return SelectiveScanFn.apply(u, delta, A, B, C, D, z, delta_bias, delta_softplus, return_last_state,
                                 torch.is_grad_enabled())
