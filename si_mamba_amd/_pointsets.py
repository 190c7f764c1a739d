"""Argument shaping the point-set distances share (chamfer.py, emd.py, sinkhorn.py).  Each entry point keeps its own
checks and messages; only what comes after them lives here."""
from __future__ import annotations

import torch


def as_pairs(x, y):
    """(x3, y3, single): ``(n, 3)`` against ``(m, 3)`` is one pair, returned as ``(1, n, 3)`` and ``(1, m, 3)``."""
    single = x.dim() == 2
    if single:
        x, y = x.unsqueeze(0), y.unsqueeze(0)
    return x, y, single


def lengths_i32(t):
    """A per-pair length tensor of any integer dtype as the kernels read it: int32.  Widened to int64 first, so that the
    clamp's bounds fit whatever dtype came in (int8, uint8, int16 included); the kernels clamp into [1, padded], and the
    clamp here only keeps 2^32 + 5 from becoming 5.  No host read."""
    return None if t is None else t.to(torch.int64).clamp(-1, 1 << 20).to(torch.int32).contiguous()
