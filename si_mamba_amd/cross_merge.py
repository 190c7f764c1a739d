"""Per-layer cross-merge of the SAST orderings (the reference's model option ``add_after_layer``).

With the option on the reference runs ``MixerModel_add`` (models/point_mamba.py:281-428): after every block it sums the
2 k copies of each patch token that the SAST sequence holds (``cross_merg``, :350-370: k eigenvector orderings, each
forward and reversed) and lays the sums out again in the same 2 k orderings (:394-409).  Written as the reference
writes it that is about twenty torch ops and some eight passes over the (B, L, C) hidden tensor per layer and
direction; here it is one pass (csrc/cross_merge.hip): L rows read, L rows written.

``G`` patches, ``k`` orderings, ``L = 2 k G``; ``order[b, i, r]`` is the patch at rank r of ordering i
(``spectral.spectral_order``) and ``R[b, i, g]`` its inverse, the rank of patch g.  The sequence holds patch
``order[i][r]`` at position ``i G + r`` and, in its second half, the flip of the whole first half.
"""
from __future__ import annotations

import torch

from . import _lib


def cross_merge_maps(order):
    """(B, k, G) orders -> (src, dst), both (B, 2 k, G) int32: rows 0 .. k-1 the forward copies, k .. 2k-1 the reversed.

        src_f[b, i, g] = i G + R[b, i, g]                    dst_f[b, i, g] = i G + R[b, i, g]
        src_r[b, i, g] = (k + i) G + G - 1 - R[b, i, g]      dst_r[b, i, g] = k G + (k G - 1 - (i G + R[b, i, g]))

    merged[b, g] sums the rows src[b, :, g] and is written to the rows dst[b, :, g]; both maps are bijections of [0, L).
    The reference's quirk, kept because a checkpoint trained with the option expects it: cross_merg flips each G-row
    segment of the reversed half in place, but that half holds the orderings in the order k-1 .. 0, so src_r[i] names
    the row of patch order[k-1-i][R[i][g]] -- patch g itself only for the middle ordering of an odd k.  dst_r is the
    true position of patch g.  The quirk lives here alone; the kernel takes whatever maps it is given.

    Index arithmetic on ``order``'s device: no host read (a step with it captures into a graph), CPU tensors work."""
    B, k, G = order.shape
    ranks = torch.arange(G, device=order.device, dtype=order.dtype).expand(B, k, G)
    R = torch.empty_like(order).scatter_(2, order, ranks)                        # inverse permutation of every row
    fwd = R + G * torch.arange(k, device=order.device, dtype=order.dtype).view(1, k, 1)
    src = torch.cat((fwd, fwd + (k * G + G - 1) - 2 * R), 1)
    dst = torch.cat((fwd, (2 * k * G - 1) - fwd), 1)
    return src.to(torch.int32).contiguous(), dst.to(torch.int32).contiguous()


def _gather_sum_scatter(x, gather_idx, scatter_idx, what):
    B, L, C = x.shape
    M, G = gather_idx.shape[1:]
    y = torch.empty_like(x)
    _lib.call("simamba_gather_sum_scatter", x, gather_idx, scatter_idx, y, B, L, G, M, C, _lib.dtype_code(x.dtype),
              device=x.device, time_as=what)
    return y


class CrossMergeFn(torch.autograd.Function):
    """out[b, dst[b, m, g]] = sum over m' of hidden[b, src[b, m', g]] (the order of additions: include/simamba.h).
    The backward is the same kernel with the two maps swapped: dh[b, src[m, g]] = sum over m' of dout[b, dst[m', g]]."""

    @staticmethod
    def forward(ctx, hidden, src, dst):
        _lib.require_gpu(hidden, "cross_merge")
        ctx.save_for_backward(src, dst)
        return _gather_sum_scatter(hidden.contiguous(), src, dst, "cross_merge_fwd")

    @staticmethod
    def backward(ctx, dout):
        src, dst = ctx.saved_tensors
        return _gather_sum_scatter(dout.contiguous(), dst, src, "cross_merge_bwd"), None, None


def cross_merge(hidden, maps):
    """hidden (B, L, C) fp32 / bf16, ``maps`` = cross_merge_maps(order) -> the merged and re-expanded sequence."""
    src, dst = maps
    if hidden.dim() != 3 or src.shape != dst.shape or src.dim() != 3 or src.dtype != torch.int32 \
            or dst.dtype != torch.int32 or src.shape[0] != hidden.shape[0] \
            or src.shape[1] * src.shape[2] != hidden.shape[1] or src.device != hidden.device \
            or dst.device != hidden.device or not (src.is_contiguous() and dst.is_contiguous()):
        raise ValueError(f"cross_merge: hidden {tuple(hidden.shape)} needs contiguous int32 maps (B, 2k, G) on its "
                         f"device with 2k * G == L, got {tuple(src.shape)} / {tuple(dst.shape)}")
    _lib.count("cross_merge")
    return CrossMergeFn.apply(hidden, src, dst)


def cross_merge_composed(hidden, order):
    """The same result through the reference's own sequence of torch ops (:350-370, :394-409), on any device: the test
    and benchmark yardstick behind ``MixerModel_add.composed``.  The reference re-sorts the eigenvectors at every layer
    (one sort for the merge, k for the expansion); the given ``order`` stands in for those sorts, so this form is, if
    anything, cheaper than the reference's."""
    B, L, C = hidden.shape
    k, G = order.shape[1:]
    segs = hidden.reshape(B, 2 * k, G, C).permute(0, 1, 3, 2)                       # (B, 2k, C, G)
    rank = torch.argsort(order.transpose(1, 2), 1).permute(0, 2, 1)                 # (B, k, G): R
    at = rank.unsqueeze(2).expand(-1, -1, C, -1)
    fwd = torch.gather(segs[:, :k].reshape(B, k, C, G), -1, at)
    rev = torch.gather(segs[:, k:].reshape(B, k, C, G).flip(-1), -1, at)
    pairs = fwd + rev
    merged = 0
    for i in range(k):
        merged = merged + pairs[:, i]
    merged = merged.permute(0, 2, 1)                                                # (B, G, C)
    seq = None
    for i in range(k):
        part = torch.gather(merged, 1, order[:, i].unsqueeze(-1).expand(-1, -1, C))
        seq = part if seq is None else torch.cat((seq, part), 1)
    return torch.cat((seq, seq.flip(1)), 1)
