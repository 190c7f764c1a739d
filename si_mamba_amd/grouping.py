"""Tokeniser ops ahead of the hot path ("next" row 1).

``sample_farthest_points`` mirrors ``pytorch3d.ops.sample_farthest_points(points, K=...)`` as the reference
calls it (models/point_mamba.py:93): returns ``(centers (B,K,3), idx (B,K))``, first pick = point 0.

Ragged batches: both ops take per-cloud ``lengths`` for clouds padded to a common N.  Cloud b then consists of its
first ``lengths[b]`` points; the padding is never read and every row of the result is what the op returns for that
cloud alone at its true length.
"""
from __future__ import annotations

import torch

from . import _lib


def _per_cloud(t, B, device, what):
    """A per-cloud integer argument as the kernels read it: (B,) int64 on ``device``.  No host read."""
    if t is None:
        return None
    if not torch.is_tensor(t):
        t = torch.as_tensor(t, device=device)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError(f"{what} must hold integers, got {t.dtype}")
    if t.device != device:
        raise ValueError(f"{what} is on {t.device}, the points are on {device}")
    if t.shape != (B,):
        raise ValueError(f"{what} must have shape ({B},), got {tuple(t.shape)}")
    return t.to(torch.int64).contiguous()


def sample_farthest_points(points, K, lengths=None, start_idx=None):
    """(B,N,3) -> (centers (B,K,3), idx (B,K)).  ``lengths`` (B,): the point count of every cloud (values outside
    [1, N] are clamped into it by the kernel); a cloud with fewer than K points gets ``lengths[b]`` picks, the remaining
    ``idx`` are -1 and the remaining ``centers`` 0 (pytorch3d's padding).  ``start_idx`` (B,): the first pick of every
    cloud, ``0 <= start_idx[b] < lengths[b]``, instead of point 0."""
    _lib.require_gpu(points, "sample_farthest_points")
    p = points.detach().float().contiguous()
    B, N, F = p.shape
    if F != 3:
        raise ValueError("sample_farthest_points expects (B, N, 3)")
    ln = _per_cloud(lengths, B, p.device, "sample_farthest_points: lengths")
    st = _per_cloud(start_idx, B, p.device, "sample_farthest_points: start_idx")
    idx = torch.empty(B, K, device=p.device, dtype=torch.int64)
    centers = torch.empty(B, K, 3, device=p.device, dtype=torch.float32)
    _lib.call("simamba_farthest_point_sample_ex", p, ln, st, idx, centers, B, N, int(K), device=p.device,
              time_as="fps")
    return centers.to(points.dtype), idx


def knn_group(centers, points, K, lengths=None, center_lengths=None):
    """(B,G,3) centres, (B,N,3) points -> (B,G,K) int64: the K nearest points of every centre (the reference's
    pytorch3d.ops.knn_points(center, xyz, K, return_sorted=False).idx at models/point_mamba.py:96).  ``lengths`` (B,):
    the point count of every cloud; with fewer than K points the first ``lengths[b]`` slots of a row are filled and the
    rest is 0.  ``center_lengths`` (B,): the number of centre rows of every cloud; the rows beyond it are 0."""
    _lib.require_gpu(points, "knn_group")
    p = points.detach().float().contiguous()
    c = centers.detach().float().contiguous()
    B, N, _ = p.shape
    G = c.shape[1]
    ln = _per_cloud(lengths, B, p.device, "knn_group: lengths")
    lc = _per_cloud(center_lengths, B, p.device, "knn_group: center_lengths")
    idx = torch.empty(B, G, int(K), device=p.device, dtype=torch.int64)
    _lib.call("simamba_knn_group_ex", p, c, ln, lc, idx, B, N, G, int(K), device=p.device, time_as="knn_group")
    return idx
