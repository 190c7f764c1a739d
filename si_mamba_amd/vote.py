"""Test-time voting for the classifier: the inner loop of the reference's ``validate_vote`` / ``test_vote``
(tools/runner_finetune.py:345-406) on the device, with no host read.

Per batch the reference samples ``point_all`` points by farthest-point sampling once, then ``times`` times draws
``npoints`` of them, gathers, applies the test transform (``PointcloudScaleAndTranslate``), runs the model and averages
the logits.  Here the subset is a ``torch.randperm`` on the device and the gather, the subset and the transform are one
launch (``transforms.sample_and_augment``).  Voting for part segmentation (per-point scores, a different loop) is not
built.
"""
from __future__ import annotations

import torch

from . import _lib, grouping
from .transforms import PointcloudScaleAndTranslate, sample_and_augment

# npoints -> how many points the one FPS keeps (runner_finetune.py:191-203, :356-363)
POINT_ALL = {1024: 1200, 2048: 2400, 4096: 4800, 8192: 8192}


def vote_logits(model, points_raw, npoints, times=10, point_all=None, transforms=None, state=None):
    """The mean over ``times`` augmented re-samples of ``model``'s logits: ``(B, N, 3) -> (B, classes)``.

    ``point_all``: how many points the farthest-point sampling keeps; None: the reference's table (1024 -> 1200,
    2048 -> 2400, 4096 -> 4800, 8192 -> 8192), capped at the cloud size as the reference caps it.  ``transforms``: the
    test-time chain, default ``[PointcloudScaleAndTranslate()]``.  ``state``: the ``AugmentState`` the chain draws from
    (its step advances by ``times``); the subsets come from torch's device generator.  Runs under ``no_grad``; put the
    model in ``eval()`` first, as the reference does."""
    _lib.require_gpu(points_raw, "vote_logits")
    if points_raw.dim() != 3 or points_raw.shape[-1] != 3:
        raise ValueError(f"vote_logits: points_raw must be (B, N, 3), got {tuple(points_raw.shape)}")
    npoints, times = int(npoints), int(times)
    if times < 1:
        raise ValueError(f"vote_logits: times must be at least 1, got {times}")
    if point_all is None:
        if npoints not in POINT_ALL:
            raise NotImplementedError(f"vote_logits: no point_all for npoints = {npoints} (the reference knows "
                                      f"{sorted(POINT_ALL)}); pass point_all")
        point_all = POINT_ALL[npoints]
    point_all = min(int(point_all), points_raw.shape[1])
    if not 1 <= npoints <= point_all:
        raise ValueError(f"vote_logits: npoints = {npoints} of point_all = {point_all}")
    chain = [PointcloudScaleAndTranslate()] if transforms is None else transforms
    with torch.no_grad():
        pts = points_raw.detach().float().contiguous()
        fps_idx = grouping.sample_farthest_points(pts, point_all)[1]
        total = None
        for _ in range(times):
            sel = torch.randperm(point_all, device=pts.device)[:npoints]
            logits = model(sample_and_augment(pts, chain, idx=fps_idx, sel=sel, state=state))
            total = logits if total is None else total + logits
        return total / times
