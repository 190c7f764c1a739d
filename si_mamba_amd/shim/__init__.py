"""Import shim: makes the reference's import lines resolve to this framework.

The reference does ``from mamba_ssm.modules.mamba_simple import Mamba`` (models/point_mamba.py:25,
part_segmentation/models/pt_mamba.py:16), ``from mamba_ssm.modules.mamba2 import Mamba2``
(models/point_mamba.py:26, imported, never used) and -- inside try/except --
``from mamba_ssm.ops.triton.layernorm import ...`` (models/block.py:9-12).  ``install_shim()``
registers synthetic ``mamba_ssm`` / ``causal_conv1d`` modules in ``sys.modules`` that point at the
HIP-backed implementations; the Triton sub-module is deliberately absent so the reference's
try/except falls back to plain ``nn.LayerNorm`` (the only path its configs use).

``install_shim(pytorch3d=True)`` additionally registers ``pytorch3d.ops`` / ``pytorch3d.loss`` stand-ins for the
three pytorch3d entry points the reference calls (models/point_mamba.py:24, :37;
part_segmentation/models/pt_mamba.py:13): ``sample_farthest_points``, ``knn_points`` and ``chamfer_distance``,
on the HIP kernels, with the call forms and return shapes the reference uses, plus the ``lengths`` /
``random_start_point`` arguments of the first two for ragged batches (clouds padded to a common point count), and
everything but the normals of the third (``x_lengths`` / ``y_lengths``, ``weights``, ``norm``, ``point_reduction``,
``single_directional``).

``install_shim(pointnet2=True)`` registers ``pointnet2_ops.pointnet2_utils`` with the two calls the reference's runners
make (tools/runner_finetune.py:15, :191-194; tools/runner_pretrain.py:17; utils/misc.py:10;
part_segmentation/models/pt_mamba.py:11): ``furthest_point_sample(xyz, K) -> (B, K) int32`` on the FPS kernel and
``gather_operation(features (B, C, N), idx (B, K)) -> (B, C, K)``, differentiable in ``features``.  (The sampling and
the gather fused with the augmentation chain is ``si_mamba_amd.transforms.sample_and_augment``.)
"""
from __future__ import annotations

import sys
import types


def install_shim(force: bool = False, pytorch3d: bool = False, pointnet2: bool = False):
    """Register ``mamba_ssm`` and ``causal_conv1d`` (and, on request, ``pytorch3d`` and ``pointnet2_ops``) stand-ins.
    Refuses to shadow real packages."""
    from .. import causal_conv1d as _cc
    from .. import mamba_simple as _ms
    from .. import selective_scan as _ss

    if not force:
        for name in ("mamba_ssm", "causal_conv1d") + (("pytorch3d",) if pytorch3d else ()) \
                + (("pointnet2_ops",) if pointnet2 else ()):
            mod = sys.modules.get(name)
            if mod is not None and not getattr(mod, "__simamba_shim__", False):
                raise RuntimeError(f"a real '{name}' package is already imported; pass force=True to shadow it")

    def _mod(name, **attrs):
        m = types.ModuleType(name)
        m.__simamba_shim__ = True
        m.__path__ = []          # behaves as a package: sub-imports consult sys.modules first
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    class Mamba2:  # imported by the reference, never constructed
        def __init__(self, *a, **kw):
            raise NotImplementedError("Mamba2 is imported but never used by SI-Mamba; not built")

    root = _mod("mamba_ssm", Mamba=_ms.Mamba)
    modules = _mod("mamba_ssm.modules")
    simple = _mod("mamba_ssm.modules.mamba_simple", Mamba=_ms.Mamba)
    m2 = _mod("mamba_ssm.modules.mamba2", Mamba2=Mamba2)
    ops = _mod("mamba_ssm.ops")
    ssi = _mod("mamba_ssm.ops.selective_scan_interface", selective_scan_fn=_ss.selective_scan_fn,
               SelectiveScanFn=_ss.SelectiveScanFn)
    root.modules, root.ops = modules, ops
    modules.mamba_simple, modules.mamba2 = simple, m2
    ops.selective_scan_interface = ssi
    _mod("causal_conv1d", causal_conv1d_fn=_cc.causal_conv1d_fn)
    if pytorch3d:
        _install_pytorch3d(_mod)
    if pointnet2:
        _install_pointnet2(_mod)
    return root


def _install_pointnet2(_mod):
    """The two pointnet2_ops calls of the reference's runners, with their argument forms:
         fps_idx = pointnet2_utils.furthest_point_sample(points, point_all)                    (runner_finetune.py:191)
         pointnet2_utils.gather_operation(points.transpose(1, 2).contiguous(), fps_idx)        (:193)."""
    import torch

    from .. import _lib, grouping

    def furthest_point_sample(xyz, npoint):
        """(B, N, 3), K -> (B, K) int32: farthest-point sampling from point 0, ties to the lower index."""
        return grouping.sample_farthest_points(xyz, int(npoint))[1].to(torch.int32)

    def gather_operation(features, idx):
        """features (B, C, N), idx (B, K) integers -> (B, C, K) = features[b, :, idx[b, k]]; differentiable in
        ``features`` (the gradient is scattered back and summed over repeated indices)."""
        _lib.require_gpu(features, "gather_operation")
        if features.dim() != 3 or idx.dim() != 2 or idx.shape[0] != features.shape[0]:
            raise ValueError(f"gather_operation: features (B, C, N) and idx (B, K), got {tuple(features.shape)} and "
                             f"{tuple(idx.shape)}")
        return torch.gather(features, 2, idx.long().unsqueeze(1).expand(-1, features.shape[1], -1))

    root = _mod("pointnet2_ops")
    root.pointnet2_utils = _mod("pointnet2_ops.pointnet2_utils", furthest_point_sample=furthest_point_sample,
                                gather_operation=gather_operation)


def _install_pytorch3d(_mod):
    """The three pytorch3d calls of the reference, with its argument forms:
         sample_farthest_points(points=xyz, K=G)[0]                      (models/point_mamba.py:93)
         knn_points(center, xyz, K=M, return_sorted=False).idx           (:96)
         chamfer_distance(pred, gt, batch_reduction=None)[0]             (:3203)."""
    import collections

    import torch

    from .. import _lib, grouping, mae

    KNN = collections.namedtuple("_KNN", ["dists", "idx", "knn"])

    def sample_farthest_points(points, lengths=None, K=50, random_start_point=False):
        """(points (B,K,3), idx (B,K)); with ``lengths`` a cloud shorter than K is padded with 0 / -1."""
        start = None
        if random_start_point:
            _lib.require_gpu(points, "sample_farthest_points")
            B, N = points.shape[:2]
            n = torch.full((B,), N, device=points.device) if lengths is None else lengths.to(points.device)
            start = (torch.rand(B, device=points.device) * n).floor().long()
            start = torch.minimum(start, n.long() - 1)               # rand(B) * n can round up to n
        return grouping.sample_farthest_points(points, K, lengths=lengths, start_idx=start)

    def knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, version=-1, return_nn=False,
                   return_sorted=True):
        if norm != 2 or return_nn:
            raise NotImplementedError("knn_points shim: squared L2, indices and distances only")
        idx = grouping.knn_group(p1, p2, K, lengths=lengths2, center_lengths=lengths1)   # ascending: valid for sorted
        nb = torch.gather(p2.unsqueeze(1).expand(-1, p1.shape[1], -1, -1), 2,
                          idx.unsqueeze(-1).expand(-1, -1, -1, p2.shape[-1]))
        dists = ((nb - p1.unsqueeze(2)) ** 2).sum(-1)
        if lengths2 is not None:                                     # slots without a neighbour: idx 0, distance 0
            dists = dists.masked_fill(torch.arange(K, device=idx.device) >= lengths2.view(-1, 1, 1), 0)
        if lengths1 is not None:
            dists = dists.masked_fill(torch.arange(p1.shape[1], device=idx.device).view(1, -1, 1)
                                      >= lengths1.view(-1, 1, 1), 0)
        return KNN(dists=dists, idx=idx, knn=None)

    def chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, weights=None,
                         batch_reduction="mean", point_reduction="mean", norm=2, single_directional=False,
                         abs_cosine=True):
        """(loss, None); with ``point_reduction=None`` ((cham_x, cham_y), None), or (cham_x, None) when one-way."""
        if x_normals is not None or y_normals is not None:
            raise NotImplementedError("chamfer_distance shim: x_normals / y_normals are not built")
        if batch_reduction not in ("mean", "sum", None):
            raise ValueError(f"chamfer_distance shim: batch_reduction must be 'mean', 'sum' or None, got "
                             f"{batch_reduction!r}")
        if point_reduction is None and batch_reduction is not None:
            raise ValueError("chamfer_distance shim: point_reduction=None needs batch_reduction=None")
        extra = any(a is not None for a in (x_lengths, y_lengths, weights)) or norm != 2 \
            or point_reduction != "mean" or single_directional
        if extra and not (x.is_cuda and y.is_cuda):
            raise NotImplementedError("chamfer_distance shim: lengths are taken by the HIP kernels only (a ROCm "
                                      "device, sets of up to 8192 points), and so are weights, norm, "
                                      "point_reduction and single_directional")
        d = mae.chamfer_distance(x, y, x_lengths=x_lengths, y_lengths=y_lengths, weights=weights, norm=norm,
                                 point_reduction=point_reduction, single_directional=single_directional)
        if point_reduction is None:
            return (d[0] if single_directional else d), None
        if batch_reduction == "sum":
            d = d.sum()
        elif batch_reduction == "mean":
            if weights is None:
                d = d.mean() if d.shape[0] else d.sum()              # the mean over max(P, 1) pairs
            else:
                total = weights.sum()
                d = torch.where(total > 0, d.sum() / torch.where(total > 0, total, torch.ones_like(total)),
                                torch.zeros_like(total))
        return d, None

    root3d = _mod("pytorch3d")
    root3d.ops = _mod("pytorch3d.ops", sample_farthest_points=sample_farthest_points, knn_points=knn_points)
    root3d.loss = _mod("pytorch3d.loss", chamfer_distance=chamfer_distance)
