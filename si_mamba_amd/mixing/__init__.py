"""Mixing and deforming augmentations on the device (csrc/mix.hip): what the ModelNet-C study (Ren, Pan, Liu, ICML
2022) lowers the corruption error of ``corruptions.evaluate_robustness`` with.

``cutmix``                PointCutMix-R / -K (Zhang et al. 2021): part of every cloud is replaced by part of a partner
                          cloud of the batch; one launch.
``pointwolf``             locally weighted deformation after PointWOLF (Kim et al. 2021); one launch.  Written from the
                          paper's description, not a reproduction of its draws.
``mixup``                 PointMixup (Chen et al. 2020): interpolation along the optimal assignment, composed from
                          ``earth_movers_distance``; no kernel of its own.
``mixed_cross_entropy``   the label arithmetic on top: ``(1 - ratio) CE(labels) + ratio CE(labels[partner])``.
``draw_pairs``            the partner map and the lambdas the three draw when they are given none.

Random numbers are counter based (Philox4x32-10 under a key of their own; the layout is in include/simamba.h): one
``AugmentState`` feeds ``transforms``, ``corruptions`` and this package without sharing a stream, and a call inside a
captured graph (``GraphedTrainStep``) draws anew at every replay.  Nothing is read on the host.

Not built: RSMix; Beta-distributed lambdas drawn in the kernel (draw them on the device and pass ``lam``); per-point
labels for segmentation (``src`` has what they need); clouds above 8192 points; partners across ranks.  There is no
CPU route and nothing here but ``mixup`` and ``mixed_cross_entropy`` is differentiable.
"""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn.functional as F

from .. import _lib
from ..emd import EMD_MAX_POINTS, earth_movers_distance
from ..transforms import AugmentState, _check_points, _index, default_state

__all__ = ["cutmix", "pointwolf", "mixup", "mixed_cross_entropy", "draw_pairs", "MODES"]

MODES = {"r": _lib.MIX_CUT_R, "k": _lib.MIX_CUT_K}


def _state(state, dev, what):
    if state is None:
        return default_state(dev)
    if not isinstance(state, AugmentState):
        raise TypeError(f"{what}: state must be an AugmentState, got {type(state).__name__}")
    if state.device != dev:
        raise ValueError(f"{what}: the state is on {state.device}, the points are on {dev}")
    return state


def _lam(lam, B, what, dev):
    if not torch.is_tensor(lam):
        raise TypeError(f"{what}: lam must be a ({B},) float32 device tensor (a host number would be baked into a "
                        "captured graph), got " + type(lam).__name__)
    if lam.device != dev:
        raise ValueError(f"{what}: lam is on {lam.device}, the points are on {dev}")
    if tuple(lam.shape) != (B,) or lam.dtype != torch.float32:
        raise ValueError(f"{what}: lam must be ({B},) float32, got {tuple(lam.shape)} {lam.dtype}")
    return lam.contiguous()


def _out(out, points, shape, what, alias_ok):
    dev = points.device
    if out is None:
        return torch.empty(shape, device=dev, dtype=torch.float32)
    if out is points and alias_ok:
        return out
    if (not torch.is_tensor(out) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or out.device != dev
            or not out.is_contiguous()):
        raise ValueError(f"{what}: out must be a contiguous {tuple(shape)} float32 tensor on {dev}")
    if out.requires_grad:
        raise RuntimeError(f"{what}: out requires grad")
    return out


def draw_pairs(B, state=None, device=None, *, partner=True, lam=True):
    """``(partner (B,) int64, lam (B,) float32)`` on the device, as ``cutmix`` and ``mixup`` draw them at the state's
    present step when they are given none: ``partner`` is a permutation of the batch (a cloud may meet itself), ``lam``
    uniform in [0, 1).  The step is not advanced.  Either can be switched off (None in its place)."""
    if state is None:
        state = default_state(device if device is not None else "cuda")
    elif not isinstance(state, AugmentState):
        raise TypeError(f"draw_pairs: state must be an AugmentState, got {type(state).__name__}")
    if B < 1 or not (partner or lam):
        raise ValueError("draw_pairs: need B >= 1 and at least one of partner and lam")
    dev = state.device
    p = torch.empty(B, device=dev, dtype=torch.int64) if partner else None
    l = torch.empty(B, device=dev, dtype=torch.float32) if lam else None
    _lib.call("simamba_mix_draw", p, l, state.tensor, B, device=dev)
    return p, l


def cutmix(points, mode="k", *, lam=None, partner=None, lengths=None, state=None, out=None, return_src=False):
    """PointCutMix of every cloud with a partner of the batch, in one launch: ``(out, partner, ratio)`` or, with
    ``return_src``, ``(out, partner, ratio, src)``.

    ``points`` (B, N, 3) float32 on the device, N <= 8192.  ``mode``: ``"r"`` (the rows that go and the rows that come
    are chosen at random) or ``"k"`` (the rows nearest to a random seed row go, the partner's rows nearest to a seed row
    of its own come, where they are).  ``partner`` (B,) integers on the device: cloud ``b`` is mixed with
    ``partner[b]``; None: a keyed permutation of the batch, drawn on the device.  ``lam`` (B,) float32 on the device in
    [0, 1]: the share of the cloud that is replaced; None: uniform in [0, 1).  A Beta-distributed ``lam`` is the
    caller's to draw on the device and pass in.  Entries of ``partner`` outside [0, B) and of ``lam`` outside [0, 1]
    are clamped on the device, a NaN becomes 0: nothing may be read on the host.  ``lengths`` (B,) integers: cloud
    ``b`` has ``lengths[b]`` real rows (clamped to [1, N]).  ``state``: an ``AugmentState`` (default: the device's
    ``default_state``); its step advances by 1.  ``out`` (B, N, 3) float32: the result's storage; it may not overlap
    ``points``.

    Cloud ``b`` loses ``m = min(int(n_b * lam), n_b, n_partner)`` rows and gains as many: its survivors stand first, in
    their input order, then the partner's rows in the partner's order; the rows behind ``n_b`` are 0.  Returns
    ``partner`` (B,) int64 on the device (so ``labels[partner]`` needs no host read), ``ratio`` (B,) float32 =
    ``m / n_b`` -- the weight of the partner's label -- and ``src`` (B, N) int32: the own input row, ``-1 - i`` for
    partner row ``i``, INT_MIN behind the length.  The call can be captured in a graph."""
    what = "cutmix"
    _check_points(points, what)
    if mode not in MODES:
        raise ValueError(f"{what}: mode must be 'r' or 'k', got {mode!r}")
    dev = points.device
    B, N, _ = points.shape
    p = points.contiguous()
    if lengths is not None:
        lengths = _index(lengths, (B,), f"{what}: lengths", dev)
    state = _state(state, dev, what)
    if lam is not None:
        lam = _lam(lam, B, what, dev)
    given = partner is not None
    if given:
        partner = _index(partner, (B,), f"{what}: partner", dev).clamp(0, B - 1)   # as the kernel does
    else:                                                        # what the kernel draws from NULL, for the caller
        partner, _ = draw_pairs(B, state, lam=False)
    out = _out(out, points, (B, N, 3), what, alias_ok=False)
    ratio = torch.empty(B, device=dev, dtype=torch.float32)
    src = torch.empty(B, N, device=dev, dtype=torch.int32) if return_src else None
    _lib.count("cutmix_points")
    _lib.call("simamba_cutmix_points", p, lengths, partner if given else None, lam, out, ratio, src, state.tensor,
              MODES[mode], B, N, device=dev, time_as="cutmix_points")
    return (out, partner, ratio, src) if return_src else (out, partner, ratio)


def pointwolf(points, *, anchors=4, sigma=0.5, rot=math.radians(10), scale=3.0, trans=0.25, renorm=True, lengths=None,
              state=None, out=None, return_anchors=False):
    """Locally weighted deformation of every cloud, in one launch: ``out`` or, with ``return_anchors``,
    ``(out, anchor_rows (B, anchors) int32)``.  After PointWOLF (Kim et al. 2021), written from the paper's description:
    the distributions are the paper's, the draws are not.

    ``anchors`` (1..8) rows of each cloud are chosen by farthest-point sampling from a random first one.  Each gets a
    transform of its own about itself: rotations about x, y, z by angles in ``[-rot, rot)`` radians, per-axis factors in
    ``[1, scale)`` or their reciprocals, shifts in ``[-trans, trans)``.  Every point moves to the mean of its images
    under the transforms, weighted by ``exp(-d^2 / (2 sigma^2))`` of its distance to the anchor.  ``renorm``: follow with
    the unit-sphere normalisation.  ``points`` (B, N, 3) float32 on the device, ``lengths``, ``state`` as in ``cutmix``;
    ``out`` may be ``points`` itself (in place).  The call can be captured in a graph."""
    what = "pointwolf"
    _check_points(points, what)
    if not (isinstance(anchors, int) and 1 <= anchors <= _lib.WOLF_MAX_ANCHORS):
        raise ValueError(f"{what}: anchors must be an integer in [1, {_lib.WOLF_MAX_ANCHORS}], got {anchors!r}")
    host = (ctypes.c_float * 4)(float(sigma), float(rot), float(scale), float(trans))
    if not (host[0] > 0 and host[1] >= 0 and host[2] >= 1 and host[3] >= 0 and all(math.isfinite(v) for v in host)
            and math.isfinite(1.0 / (2.0 * host[0] * host[0]))):
        raise ValueError(f"{what}: need sigma > 0, rot >= 0, scale >= 1, trans >= 0, all finite; got sigma={sigma!r}, "
                         f"rot={rot!r}, scale={scale!r}, trans={trans!r}")
    dev = points.device
    B, N, _ = points.shape
    if lengths is not None:
        lengths = _index(lengths, (B,), f"{what}: lengths", dev)
    state = _state(state, dev, what)
    p = points.contiguous()
    out = _out(out, points, (B, N, 3), what, alias_ok=True)
    target = p if out is points else out                         # a non-contiguous in-place input: through its copy
    rows = torch.empty(B, anchors, device=dev, dtype=torch.int32) if return_anchors else None
    _lib.count("pointwolf_points")
    _lib.call("simamba_pointwolf_points", p, lengths, target, rows, state.tensor, anchors, host,
              _lib.WOLF_RENORM if renorm else 0, B, N, device=dev, time_as="pointwolf_points")
    if target is not out:
        out.copy_(target)
    return (out, rows) if return_anchors else out


def mixup(points, *, lam=None, partner=None, state=None):
    """PointMixup (Chen et al. 2020): every cloud moves the share ``lam`` of the way to its partner along the optimal
    assignment between the two, ``a + lam (b[assign] - a)``: ``(out, partner, lam)``, for
    ``mixed_cross_entropy(logits, labels, partner, lam)``.

    Composed from ``earth_movers_distance(points, points[partner], return_assignment=True)`` and torch ops; no kernel
    of its own.  ``points`` (B, N, 3) float32 on the device with every cloud N rows long (there is no ``lengths``: the
    assignment is one-to-one) and N <= 1024, the auction's limit.  ``partner`` and ``lam`` as in ``cutmix``, drawn by
    the same rule (``draw_pairs``) when None; ``lam`` given is clamped to [0, 1], a NaN becomes 0.  The state's step
    advances by 1, on the device."""
    what = "mixup"
    _check_points(points, what)
    dev = points.device
    B, N, _ = points.shape
    if N > EMD_MAX_POINTS:
        raise ValueError(f"{what}: N = {N} rows per cloud; the assignment (earth_movers_distance) takes at most "
                         f"{EMD_MAX_POINTS}")
    state = _state(state, dev, what)
    drawn_p, drawn_l = draw_pairs(B, state, partner=partner is None, lam=lam is None) \
        if partner is None or lam is None else (None, None)
    partner = drawn_p if partner is None else _index(partner, (B,), f"{what}: partner", dev).clamp(0, B - 1)
    lam = drawn_l if lam is None else torch.nan_to_num(_lam(lam, B, what, dev), nan=0.0).clamp(0.0, 1.0)
    state.tensor[1] += 1                                         # on the device, in stream order
    a = points.contiguous()
    b = a[partner]
    _, assign, _, _ = earth_movers_distance(a, b, return_assignment=True)
    matched = torch.gather(b, 1, assign.long().unsqueeze(-1).expand(B, N, 3))
    return a + lam.view(B, 1, 1) * (matched - a), partner, lam


def mixed_cross_entropy(logits, labels, partner, ratio, reduction="mean"):
    """``(1 - ratio) * CE(logits, labels) + ratio * CE(logits, labels[partner])`` per cloud, in torch ops (so it is
    differentiable in ``logits``): the loss of a batch that ``cutmix`` or ``mixup`` produced.  ``logits`` (B, classes),
    ``labels`` (B,) and ``partner`` (B,) integers, ``ratio`` (B,) floats.  ``reduction``: "mean", "sum" or "none"."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"mixed_cross_entropy: reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
    if logits.dim() != 2 or labels.shape != logits.shape[:1] or partner.shape != labels.shape \
            or ratio.shape != labels.shape:
        raise ValueError(f"mixed_cross_entropy: need logits (B, classes) and labels, partner, ratio (B,), got "
                         f"{tuple(logits.shape)}, {tuple(labels.shape)}, {tuple(partner.shape)}, {tuple(ratio.shape)}")
    labels = labels.long()
    ratio = ratio.to(logits.dtype)
    own = F.cross_entropy(logits, labels, reduction="none")
    other = F.cross_entropy(logits, labels[partner.long()], reduction="none")
    loss = (1 - ratio) * own + ratio * other
    return loss.mean() if reduction == "mean" else loss.sum() if reduction == "sum" else loss
