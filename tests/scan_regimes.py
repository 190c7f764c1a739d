"""Selective-scan inputs outside the initialisation regime, and the float64 reference / error metric they are judged by.

TEST INFRASTRUCTURE (shared by test_oracle_scan_regimes.py, CPU, and test_gpu_scan_regimes.py).  Every other scan test
draws from ``si_mamba_amd.synthetic.scan_inputs``: x = delta + delta_bias in about [-8, -1], A about -(1..16), z ~ N(0,1).
Each regime here is a function of (batch, dim, L, N, seed) that returns the same dict and moves ONE of those ranges:

  init           scan_inputs itself (the control)
  small_dt       x spread over [-15, -5]: per channel through the bias (a stratified spread over [-14.5, -5.5]), along
                 time through delta in [-0.5, 0.5]
  series_branch  x in [-30, -15), where softplus(x) = exp(x) to 1.5e-7; channels 0 and 1 carry, at every even step,
                 x = -15 - 1 ulp and x = -15 + 1 ulp (the two sides of the kernels' seam; the second is the one
                 element kind of this regime that is not below -15)
  large_dt       x in [15, 100]: a third of the channels around 20 (both sides of torch's threshold), a third between,
                 a third above 88 (exp(x) overflows fp32 behind the select); |A| in [3e-4, 0.015] so that the
                 recurrence stays a recurrence at steps of 15 .. 100
  long_memory    A in [-1e-2, -1e-4], steps 0.01 .. 0.1 (meant for L = 1024: eight carried chunks that hardly decay)
  fast_decay     delta * A in [-100, -20]: steps in [2, 3.9], A[:, 0] = -10 (so state 0 of every channel stays above
                 -40 and no channel's dA scale is a denormal), the other states down to -25.6
  gate_ends      z in [-30, 30]; channels 0 mod 4 only in [-30, -15], 1 mod 4 only in [15, 30], so that each end sets
                 the scale of some channels on its own
  mixed          channel d takes its bias from regime d mod 4 of (init, small_dt, series_branch, large_dt) and its A from
                 d mod 3 of (init, long_memory, -(0.1 .. 2)); the 4-step pack p of row d is moved, through delta, into
                 regime (d + p) mod 4: adjacent channels of a wave and successive packs of a row differ within one launch

u, delta, z, B, C and dout are exactly representable in bf16 (rounded once here), so one float64 reference serves the
fp32 and the bf16 rows; A, D and delta_bias are fp32 parameters.  Where the step is tiny (small_dt, series_branch, mixed)
D is zero on the even channels: with D ~ 1 the skip term D * u would be 1e6 .. 1e13 times the scan's own contribution
to ``out`` and ``du`` and hide it from every comparison.
"""
import math

import torch
import torch.nn.functional as F

from oracle import scan_ref
from si_mamba_amd.synthetic import scan_inputs

ACT = ("u", "delta", "z", "B", "C", "dout")
LEAVES = ("u", "delta", "A", "B", "C", "D", "z", "delta_bias")
ULP15 = 2.0 ** -20                      # fp32 spacing just below 16


def _bf16(t):
    return t.to(torch.bfloat16).float()


def _base(batch, dim, L, N, seed):
    inp = scan_inputs(batch, dim, L, N, seed)
    for k in ACT:
        inp[k] = _bf16(inp[k])
    return inp, torch.Generator().manual_seed(seed + 7919)


def _spread(dim, lo, hi, g):
    """dim values stratified over [lo, hi] (one per equal cell), in a random channel order."""
    cells = (torch.arange(dim) + torch.rand(dim, generator=g)) / dim
    return (lo + (hi - lo) * cells)[torch.randperm(dim, generator=g)]


def _uniform(shape, lo, hi, g):
    return lo + (hi - lo) * torch.rand(shape, generator=g)


def init(batch, dim, L, N, seed):
    return _base(batch, dim, L, N, seed)[0]


def small_dt(batch, dim, L, N, seed):
    inp, g = _base(batch, dim, L, N, seed)
    inp["delta_bias"] = _spread(dim, -14.5, -5.5, g)
    inp["delta"] = _bf16(_uniform((batch, dim, L), -0.5, 0.5, g))
    inp["D"][::2] = 0.0
    return inp


def series_branch(batch, dim, L, N, seed):
    inp, g = _base(batch, dim, L, N, seed)
    bias = _spread(dim, -28.75, -16.25, g)
    delta = _bf16(_uniform((batch, dim, L), -1.0, 1.0, g))
    if dim >= 2:                        # the seam: x = bias exactly where delta = 0
        bias[0], bias[1] = -15.0 - ULP15, -15.0 + ULP15
        delta[:, :2] = _bf16(_uniform((batch, 2, L), -8.0, -1.0, g))
        delta[:, :2, ::2] = 0.0
    inp["delta_bias"], inp["delta"] = bias, delta
    inp["D"][::2] = 0.0
    return inp


def large_dt(batch, dim, L, N, seed):
    inp, g = _base(batch, dim, L, N, seed)
    third = torch.arange(dim) % 3
    bias = torch.where(third == 0, _uniform((dim,), 15.5, 24.5, g),
                       torch.where(third == 1, _uniform((dim,), 24.5, 88.0, g), _uniform((dim,), 88.5, 99.5, g)))
    inp["delta_bias"] = bias
    inp["delta"] = _bf16(_uniform((batch, dim, L), -0.5, 0.5, g))
    inp["A"] = -0.01 * (torch.arange(1, N + 1).float() / N)[None] * _uniform((dim, N), 0.5, 1.5, g)
    return inp


def long_memory(batch, dim, L, N, seed):
    inp, g = _base(batch, dim, L, N, seed)
    inp["A"] = -torch.exp(_uniform((dim, N), math.log(1e-4), math.log(1e-2), g))
    dt = torch.exp(_uniform((dim,), math.log(0.0135), math.log(0.074), g)).double()
    inp["delta_bias"] = (dt + torch.log(-torch.expm1(-dt))).float()          # softplus^-1
    inp["delta"] = _bf16(_uniform((batch, dim, L), -0.25, 0.25, g))            # steps stay inside [0.01, 0.1]
    return inp


def fast_decay(batch, dim, L, N, seed):
    inp, g = _base(batch, dim, L, N, seed)
    inp["delta_bias"] = _uniform((dim,), 2.2, 3.6, g)
    inp["delta"] = _bf16(_uniform((batch, dim, L), -0.25, 0.25, g))            # x in [1.95, 3.85]: steps in [2.08, 3.88]
    A = -_uniform((dim, N), 10.0, 25.6, g)
    A[:, 0] = -10.0
    inp["A"] = A
    return inp


def gate_ends(batch, dim, L, N, seed):
    inp, g = _base(batch, dim, L, N, seed)
    z = _uniform((batch, dim, L), -30.0, 30.0, g)
    z[:, 0::4] = _uniform(z[:, 0::4].shape, -30.0, -15.0, g)
    z[:, 1::4] = _uniform(z[:, 1::4].shape, 15.0, 30.0, g)
    inp["z"] = _bf16(z)
    return inp


_MIX_X = ((-4.0, 2.0), (-10.0, 4.5), (-22.5, 6.5), (57.0, 41.0))     # (centre, half width) of x in the four x regimes


def mixed(batch, dim, L, N, seed):
    inp, g = _base(batch, dim, L, N, seed)
    centre = torch.tensor([c for c, _ in _MIX_X])
    width = torch.tensor([w for _, w in _MIX_X])
    d = torch.arange(dim)
    bias = centre[d % 4] + _uniform((dim,), -0.25, 0.25, g)
    reg = (d[:, None] + torch.arange(L)[None] // 4) % 4                          # (dim, L): regime of pack t // 4 of row d
    x = centre[reg][None] + width[reg][None] * _uniform((batch, dim, L), -1.0, 1.0, g)
    inp["delta"] = _bf16(x - bias[None, :, None])                                # bf16 rounding moves x by < 0.3
    inp["delta_bias"] = bias
    A = inp["A"].clone()
    A[1::3] = -torch.exp(_uniform(A[1::3].shape, math.log(1e-4), math.log(1e-2), g))
    A[2::3] = -_uniform(A[2::3].shape, 0.1, 2.0, g)
    inp["A"] = A
    inp["D"][::2] = 0.0
    return inp


REGIMES = {f.__name__: f for f in (init, small_dt, series_branch, large_dt, long_memory, fast_decay, gate_ends, mixed)}


def x_of(inp):
    """delta + delta_bias in float64 (exact: both operands are fp32 values)."""
    return inp["delta"].double() + inp["delta_bias"].double()[None, :, None]


# ---- reference and oracles ------------------------------------------------------------------------------------------
TENSORS = ("out", "last_state", "du", "ddelta", "dz", "dA", "dB", "dC", "dD", "ddelta_bias")
_GRAD_NAME = {"u": "du", "delta": "ddelta", "z": "dz", "A": "dA", "B": "dB", "C": "dC", "D": "dD",
              "delta_bias": "ddelta_bias"}


def run_ref(inp, mode, delta_softplus=True):
    """{'out', 'last_state', 'du', ..., 'ddelta_bias'} of oracle.scan_ref.selective_scan_ref on ``inp``.
    mode 'f64': double leaves, float64 accumulation -- the reference.  'f32': the fp32 CPU oracle.  'bf16': the same fp32
    oracle on bf16-rounded activations (a no-op here: they are bf16 values already), with the output and the activation
    gradients rounded to bf16 where the device returns bf16 tensors."""
    f64 = mode == "f64"
    leaf = {}
    for k in LEAVES:
        if inp.get(k) is not None:
            v = inp[k].double() if f64 else (_bf16(inp[k]) if (mode == "bf16" and k in ACT) else inp[k].clone())
            leaf[k] = v.requires_grad_(True)
    out, last = scan_ref.selective_scan_ref(leaf["u"], leaf["delta"], leaf["A"], leaf["B"], leaf["C"], leaf.get("D"),
                                            leaf.get("z"), leaf.get("delta_bias"), delta_softplus=delta_softplus,
                                            return_last_state=True,
                                            acc_dtype=torch.float64 if f64 else torch.float32)
    out.backward(inp["dout"].double() if f64 else inp["dout"])
    res = {"out": out.detach(), "last_state": last.detach()}
    res.update({_GRAD_NAME[k]: v.grad for k, v in leaf.items()})
    if mode == "bf16":
        for k in ("out", "du", "ddelta", "dz", "dB", "dC"):
            if k in res:
                res[k] = _bf16(res[k])
    return res


# ---- the metric ---------------------------------------------------------------------------------------------------
CHANNEL_DIM = {"out": 1, "last_state": 1, "du": 1, "ddelta": 1, "dz": 1, "dA": 0}      # the others: the tensor's own scale


def channel_err(got, want, dim):
    """max over channels of (max |got - want| over the other axes) / (max |want| of the same channel), in float64.  A
    channel whose reference is all zero has no scale: inf, so that a bound on the result fails instead of skipping it."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    other = [a for a in range(want.dim()) if a != dim]
    diff = (got - want).abs()
    num = diff.amax(other) if other else diff
    den = want.abs().amax(other) if other else want.abs()
    return torch.where(den > 0, num / den, torch.full_like(num, math.inf)).max().item()


def errors(got, want):
    """name -> {'chan': the per-channel scaled error (tensors with a channel axis; for dD / ddelta_bias, dB / dC the max
    error on the tensor's own scale), 'max', 'rms': helpers.scaled_err on the whole tensor, 'elem': worst single-element
    relative error (dD and ddelta_bias only; reported, not bounded)}."""
    from helpers import scaled_err
    res = {}
    for k, w in want.items():
        if k not in got or got[k] is None:
            continue
        mx, rms = scaled_err(got[k], w)
        e = {"chan": channel_err(got[k], w, CHANNEL_DIM[k]) if k in CHANNEL_DIM else mx, "max": mx, "rms": rms}
        if k in ("dD", "ddelta_bias"):
            wd = w.detach().double().cpu()
            e["elem"] = ((got[k].detach().double().cpu() - wd).abs() / wd.abs().clamp_min(1e-300)).max().item()
        res[k] = e
    return res


def channel_floor(want):
    """name -> the smallest per-channel max |want| (tensors with a channel axis): above 1e-30 means no channel is left
    out of, or divides by nothing in, the per-channel comparison."""
    res = {}
    for k, dim in CHANNEL_DIM.items():
        if k in want:
            w = want[k].detach().double().abs()
            other = [a for a in range(w.dim()) if a != dim]
            res[k] = w.amax(other).min().item()
    return res


# ---- the kernels' softplus, restated on the CPU (reference-side evidence only) -----------------------------------------
def softplus_log2_form_f32(x):
    """float32 restatement of the form the kernels used: log2(1 + exp2(x log2 e)) * ln 2 with correctly rounded exp2 and
    log2, e below x = -15, x above 20.  1 + e drops the low bits of e: this is what the small_dt bound must catch."""
    import numpy as np
    x = x.detach().cpu().numpy().astype(np.float32)
    log2e, ln2 = np.float32(1.4426950408889634), np.float32(0.6931471805599453)
    with np.errstate(over="ignore"):
        e = np.exp2((x * log2e).astype(np.float64)).astype(np.float32)
        sp = (np.log2((np.float32(1) + e).astype(np.float64)).astype(np.float32) * ln2).astype(np.float32)
    sp = np.where(x < np.float32(-15), e, sp)
    return torch.from_numpy(np.where(x > np.float32(20), x, sp).astype(np.float32))


def softplus_torch_f32(x):
    return F.softplus(x.float())
