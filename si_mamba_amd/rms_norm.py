"""RMSNorm: what the reference's create_block / MixerModel build for ``rms_norm=True`` (models/point_mamba.py:164,
:227; part_segmentation/models/pt_mamba.py:134, :277), imported there from mamba-ssm's Triton module
(mamba_ssm/ops/triton/layernorm.py).  Same constructor, parameter names (``weight`` only; ``bias`` is registered as
None, so a state dict holds ``*.weight`` alone) and forward signature.

On a ROCm device the forward is the add + RMSNorm kernel of add_norm.py (csrc/add_norm.hip with SIMAMBA_NORM_RMS);
on the CPU it is the composed torch formula (mamba-ssm's ``rms_norm_ref``), as nn.LayerNorm serves Block's CPU route.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .add_norm import add_rms_norm_fn


def rms_norm_composed(x, weight, residual=None, eps=1e-5, prenorm=False, residual_in_fp32=False):
    """The torch formula, in fp32: -> normed (x.dtype), or (normed, residual_out) with ``prenorm``."""
    dtype = x.dtype
    xs = x.float() if residual is None else x.float() + residual.float()
    rstd = torch.rsqrt(xs.square().mean(dim=-1, keepdim=True) + eps)
    out = (xs * rstd * weight.float()).to(dtype)
    if not prenorm:
        return out
    res_dtype = torch.float32 if residual_in_fp32 else (residual.dtype if residual is not None else dtype)
    return out, xs.to(res_dtype)


class RMSNorm(nn.Module):
    def __init__(self, hidden_size, eps=1e-5, device=None, dtype=None):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.empty(hidden_size, device=device, dtype=dtype))
        self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.ones_(self.weight)

    def forward(self, x, residual=None, prenorm=False, residual_in_fp32=False):
        """normed = x' / sqrt(mean(x'^2) + eps) * weight with x' = x + residual (or x); returned in x's dtype.
        ``prenorm``: -> (normed, x') with x' in fp32 when ``residual_in_fp32``, else in residual's (or x's) dtype.
        On a ROCm device the kernel takes fp32 / bf16 ``x``, ``hidden_size % 4 == 0`` and ``hidden_size <= 2048`` (every
        model of this package: d_model 384); anything else raises -- there is no eager fallback on the device."""
        if not x.is_cuda:
            return rms_norm_composed(x, self.weight, residual, self.eps, prenorm, residual_in_fp32)
        d = x.shape[-1]
        if x.dtype not in (torch.float32, torch.bfloat16) or d % 4 or d > 2048:
            raise ValueError(f"RMSNorm on {x.device}: the HIP kernel takes float32 / bfloat16 inputs with a last "
                             f"dimension divisible by 4 and at most 2048, got {x.dtype} x {d}")
        x3 = x.reshape(1, -1, d)
        r3 = None if residual is None else residual.reshape(1, -1, d)
        normed, res_out = add_rms_norm_fn(x3, r3, self.weight, self.eps, out_dtype=x.dtype)
        normed = normed.view(x.shape)
        if not prenorm:
            return normed
        res_dtype = torch.float32 if residual_in_fp32 else (residual.dtype if residual is not None else x.dtype)
        return normed, res_out.view(x.shape).to(res_dtype)

    def extra_repr(self):
        return f"{self.weight.shape[0]}, eps={self.eps}"
