"""Shared pieces of the tests: the error metrics, the random point clouds and the bit-for-bit comparison.

TEST INFRASTRUCTURE.  One definition of each, so that a bound such as ``nerr(...) < 1e-3`` reads the same in every file.
Every metric is evaluated in float64 on detached CPU copies: the operands are fp32 / bf16 tensors, so the float64
value is the exact value of the formula.
"""
import numpy as np
import torch


def _f64(t):
    return t.detach().double().cpu()


# ---- error metrics ---------------------------------------------------------------------------------------------------
def nerr(got, want):
    """max |got - want| / max(1, max |want|): the normalised error the north-star tolerances are stated on."""
    got, want = _f64(got), _f64(want)
    return ((got - want).abs().max() / max(1.0, want.abs().max().item())).item()


def scaled_err(got, want):
    """(max |got - want| / max |want|, rms(got - want) / rms(want)) in float64: the error on the tensor's OWN scale, with
    no floor of 1 -- what a gradient of order 1e-3 needs (``nerr`` lets an absolute 1e-3 through, i.e. all of it).
    Explicit fallback for a reference that is exactly zero (no scale to divide by): the two ABSOLUTE errors
    (max |got|, rms(got)); a bound stated on the ratio then demands |got| below that bound outright."""
    got, want = _f64(got), _f64(want)
    diff = got - want
    dmax, drms = diff.abs().max().item(), diff.square().mean().sqrt().item()
    wmax, wrms = want.abs().max().item(), want.square().mean().sqrt().item()
    if wmax == 0.0:
        return dmax, drms
    return dmax / wmax, drms / wrms


def peak_err(got, want):
    """max |got - want| / (max |want| + 1e-12): the error on the reference's peak, with no floor of 1 (much stricter
    than ``nerr`` for tensors below 1); the epsilon only keeps an all-zero reference from dividing by zero."""
    got, want = _f64(got), _f64(want)
    return float((got - want).abs().max() / (want.abs().max() + 1e-12))


def max_scaled(got, want):
    """max |got - want| / max |want|, with neither floor nor epsilon."""
    got, want = _f64(got), _f64(want)
    return float((got - want).abs().max() / want.abs().max())


def relerr(got, want):
    """The largest elementwise |got - want| / |want|."""
    got, want = _f64(got), _f64(want)
    return float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())


def pinned_bound(ref32_err, cap):
    """The bound of an assertion against a reference-pinned fixture: 8 x ``ref32_err`` (the reference's own fp32 run
    against its float64 run under the assertion's metric; three bits for another summation order and split-K partials),
    never above ``cap`` (what the op's older tests allow).  Floor 8 x 2^-24: a recorded ``ref32_err`` is ONE draw of a
    rounding error -- for a single number such as a gradient norm it can lie far below fp32's resolution by chance -- and
    no fp32 result can be held below half an ulp of its peak."""
    return min(max(8.0 * float(ref32_err), 8.0 * 2.0 ** -24), cap)


# ---- point clouds ----------------------------------------------------------------------------------------------------
def clouds_from(B, N, gen):
    """N(0,1) points from the generator ``gen``, centred and scaled into the unit ball per cloud (a single point
    cannot be centred: it is scaled only)."""
    p = torch.randn(B, N, 3, generator=gen)
    if N > 1:
        p = p - p.mean(1, keepdim=True)
    return p / p.norm(dim=-1).max(dim=1)[0][:, None, None]


def clouds(B, N, seed):
    """(B, N, 3) N(0,1) points of the seed, centred and scaled into the unit ball per cloud."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(B, N, 3, generator=g)
    p = p - p.mean(1, keepdim=True)
    return p / p.norm(dim=-1).max(dim=1)[0][:, None, None]


# ---- parameters from an integer formula ------------------------------------------------------------------------------
def formula_tensor(shape, salt, scale=1.0, offset=0.0, dtype=torch.float32):
    """offset + scale * v with v in [-1, 1) on a grid of 1/1024, from int64 arithmetic alone: element i (row-major) hashes
    to h = mix(i * 2654435761 + salt) mod 2^32 and v = ((h >> 21) - 1024) / 1024.  No generator and no platform is
    involved, so the fixture recipe (oracle/pin_from_reference.py) and a test build the same weights without the fixture
    carrying them.  The second multiply-xorshift round breaks the period of 2048 the plain product would have."""
    n = int(np.prod(shape)) if len(shape) else 1
    m32 = (1 << 32) - 1
    h = (torch.arange(n, dtype=torch.int64) * 2654435761 + int(salt)) & m32
    h = ((h ^ (h >> 15)) * 2246822519) & m32
    h = h ^ (h >> 13)
    v = ((h >> 21) - 1024).double() / 1024.0
    return (offset + scale * v).to(dtype).reshape(shape)


def formula_parameters(module, salt, running=False):
    """Fill a module's parameters (and, with ``running``, its BatchNorm running statistics) from ``formula_tensor``, in
    named_parameters() order: weights of a layer with fan-in f spread over +-2/sqrt(f), biases over +-0.1, BatchNorm
    scales over 1 +- 0.25; running means over +-0.2 and running variances over 1 +- 0.5."""
    with torch.no_grad():
        for k, (name, p) in enumerate(module.named_parameters()):
            s = salt + 7919 * k
            if p.dim() >= 2:
                fan_in = int(np.prod(p.shape[1:]))
                p.copy_(formula_tensor(p.shape, s, 2.0 / fan_in ** 0.5))
            elif name.endswith("weight"):
                p.copy_(formula_tensor(p.shape, s, 0.25, 1.0))
            else:
                p.copy_(formula_tensor(p.shape, s, 0.1))
        if running:
            for k, (name, b) in enumerate(module.named_buffers()):
                s = salt + 104729 * (k + 1)
                if name.endswith("running_mean"):
                    b.copy_(formula_tensor(b.shape, s, 0.2))
                elif name.endswith("running_var"):
                    b.copy_(formula_tensor(b.shape, s, 0.5, 1.0))
    return module


HEAD_PARTS = ("norm", "label_conv", "propagation_0", "convs1", "bns1", "convs2", "bns2", "convs3")


def formula_head(model, salt, running=False):
    """formula_parameters on each module of a segmentation head by NAME (the reference's get_model and PartSegMamba
    register them in different orders): part i gets salt + 1000 i."""
    for i, name in enumerate(HEAD_PARTS):
        formula_parameters(getattr(model, name), salt + 1000 * i, running=running)
    return model


# ---- bit-for-bit comparison of 32-bit tensors ------------------------------------------------------------------------
def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))
