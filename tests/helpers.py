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


# ---- bit-for-bit comparison of 32-bit tensors ------------------------------------------------------------------------
def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))
