"""Device-resident datasets (csrc/dataset.hip): the reference's ``torch.utils.data.DataLoader`` over its four dataset
classes -- epoch shuffle, per-item point sampling, ``pc_norm``, collate and the host-to-device copy -- as one launch per
batch with no host work and no host read.

``DeviceDataset`` holds every cloud of a split in device memory (the largest of the reference's, ShapeNet-55 at 8192
points, is 5.2 GB); ``DeviceLoader.fetch()`` gathers a batch out of it.  Which cloud goes into which slot and which of
its rows are taken are counter-based functions of ``(seed, epoch, position in the epoch)`` (a keyed bijection over
Philox4x32-10, csrc/keyed_perm.h; the layout is in include/simamba.h), read from a device tensor ``[seed, step]`` that
a one-lane kernel advances: a call inside a captured graph yields the next batch at every replay, and an epoch is
``len(loader)`` replays.  The reference's numpy streams cannot be reproduced on a device and are not: the distributions
are the reference's, the draws are not.

Not built: file parsing (the caller reads its files and hands arrays over), extra channels such as normals, more than
8192 points per cloud in a batch, weighted or class-balanced sampling, ModelNet's ``uniform`` farthest-point
preprocessing (``grouping.sample_farthest_points`` can do that once, when the store is built).  There is no CPU route.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .transforms import AugmentState, _MASK64

__all__ = ["DeviceDataset", "DeviceLoader", "Batch"]

Batch = namedtuple("Batch", ["points", "label", "point_label", "index", "lengths"])

_ROWS = {"first": _lib.DS_FIRST, "permute": _lib.DS_PERMUTE, "choice": _lib.DS_CHOICE}
_NORM = {None: _lib.DS_NONE, "unit_sphere": _lib.DS_UNIT_SPHERE}


def _device(device, what):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{what}: device is {device}; si_mamba_amd runs on a ROCm device only (no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class DeviceDataset:
    """The clouds of one split, back to back in device memory: ``points`` (T, 3) float32, ``offsets`` (S + 1) int64 or
    None for a store of ``stride`` points per cloud, ``labels`` (S) int64 or None, ``point_labels`` (T) int32 or None."""

    def __init__(self, points, offsets, stride, labels, point_labels):
        self.points, self.offsets, self.stride, self.labels, self.point_labels = (points, offsets, stride, labels,
                                                                                  point_labels)
        self._len = (offsets.numel() - 1) if offsets is not None else points.shape[0] // stride

    @classmethod
    def from_arrays(cls, points, labels=None, point_labels=None, device="cuda"):
        """``points``: an (S, n, 3) array or tensor, or a sequence of (n_s, 3) arrays for a ragged store.  ``labels``:
        (S,) integers.  ``point_labels``: (S, n) integers, or a sequence of (n_s,) arrays.  Everything is copied to
        ``device`` once; whole-cloud preprocessing (``normalize_``) runs there afterwards."""
        what = "DeviceDataset.from_arrays"
        device = _device(device, what)
        ragged = isinstance(points, (list, tuple))
        if ragged:
            clouds = [torch.as_tensor(np.asarray(c) if not torch.is_tensor(c) else c) for c in points]
            if not clouds or any(c.dim() != 2 or c.shape[1] != 3 for c in clouds):
                raise ValueError(f"{what}: a ragged store is a non-empty sequence of (n_s, 3) arrays")
            counts = [c.shape[0] for c in clouds]
            flat = torch.cat([c.to(torch.float32) for c in clouds]).to(device)
            offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64, device=device)
            stride, S = 0, len(clouds)
        else:
            pts = torch.as_tensor(points)
            if pts.dim() != 3 or pts.shape[2] != 3 or pts.shape[0] < 1 or pts.shape[1] < 1:
                raise ValueError(f"{what}: points must be (S, n, 3) or a sequence of (n_s, 3), got {tuple(pts.shape)}")
            S, stride = pts.shape[0], pts.shape[1]
            counts = [stride] * S
            flat = pts.to(torch.float32).reshape(S * stride, 3).to(device).contiguous()
            offsets = None
        if S >= 1 << 31:
            raise ValueError(f"{what}: {S} clouds, a store takes fewer than 2^31")
        if labels is not None:
            labels = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels)
            if tuple(labels.shape) != (S,):
                raise ValueError(f"{what}: labels must be ({S},), got {tuple(labels.shape)}")
            labels = labels.to(torch.int64).to(device).contiguous()
        if point_labels is not None:
            if isinstance(point_labels, (list, tuple)):
                pl = [torch.as_tensor(np.asarray(c) if not torch.is_tensor(c) else c).reshape(-1) for c in point_labels]
            else:
                pl = torch.as_tensor(point_labels)
                pl = list(pl) if pl.dim() == 2 else None
            if pl is None or [c.shape[0] for c in pl] != counts:
                raise ValueError(f"{what}: point_labels must give one label per point of every cloud")
            point_labels = torch.cat(pl).to(torch.int32).to(device).contiguous()
        return cls(flat, offsets, stride, labels, point_labels)

    def __len__(self):
        return self._len

    @property
    def device(self):
        return self.points.device

    @property
    def nbytes(self):
        """Bytes of device memory the store holds."""
        return sum(t.numel() * t.element_size()
                   for t in (self.points, self.offsets, self.labels, self.point_labels) if t is not None)

    def counts(self):
        """(S,) int64 on the device: the points of every cloud."""
        if self.offsets is None:
            return torch.full((len(self),), self.stride, dtype=torch.int64, device=self.device)
        return self.offsets[1:] - self.offsets[:-1]

    @torch.no_grad()
    def normalize_(self):
        """Every WHOLE cloud to the unit sphere, in place, once (``pc_normalize`` at part_segmentation/dataset.py:153 and
        ModelNetDataset.py:167): subtract the cloud's mean, divide by its largest norm; a cloud whose
        points all coincide becomes zeros.  Torch ops: this is preprocessing, not the per-batch path."""
        S = len(self)
        if self.offsets is None:
            v = self.points.view(S, self.stride, 3)
            v -= v.mean(1, keepdim=True)
            m = v.norm(dim=2).amax(1)
            v /= torch.where(m > 0, m, torch.ones_like(m))[:, None, None]
            return self
        counts = self.counts()
        cloud = torch.repeat_interleave(torch.arange(S, device=self.device), counts)
        mean = torch.zeros(S, 3, device=self.device).index_add_(0, cloud, self.points)
        mean /= counts.clamp(min=1)[:, None]
        self.points -= mean[cloud]
        m = torch.zeros(S, device=self.device).scatter_reduce_(0, cloud, self.points.norm(dim=1), "amax")
        self.points /= torch.where(m > 0, m, torch.ones_like(m))[cloud][:, None]
        return self


class DeviceLoader:
    """``DataLoader(dataset, batch_size, shuffle, drop_last)`` with the dataset's per-item sampling, on the device.

    ``npoints``: rows per cloud in a batch (1 .. 8192).  ``subsample``: ``"permute"`` -- ``npoints`` of the candidates
    without replacement, in random order (``random_sample`` of ShapeNet55Dataset.py:55-58, the ``pt_idxs`` shuffle of
    ScanObjectNNDataset.py:38-41 and ModelNetDataset.py:176-178); ``"choice"`` -- with replacement
    (``np.random.choice(len(seg), npoints, replace=True)``, part_segmentation/dataset.py:155-158); ``"first"`` -- the
    first ``npoints`` in order (the test splits).  ``first``: the candidates are the cloud's first ``first`` rows
    (0: all).  ``normalize``: None or ``"unit_sphere"`` (``pc_norm`` of the SELECTED rows, ShapeNet55Dataset.py:47-53;
    rows that all coincide give zeros where the reference divides by zero).  ``rank`` / ``world``: slot ``b`` of step
    ``pos`` takes position ``(pos * batch_size + b) * world + rank`` of the epoch's order, so the ranks' batches are
    disjoint and a slot does not depend on ``batch_size``.

    ``len(loader)``: steps per epoch, ``S // (batch_size * world)`` with ``drop_last`` (fewer clouds than one step is
    a ValueError), else the ceiling; the slots of the last batch that fall behind the dataset are empty: index -1,
    label -1, length 0, rows 0.

    ``fetch(out=None)`` enqueues one launch and returns ``Batch(points (B, K, 3) float32, label (B,) int64 | None,
    point_label (B, K) int32 | None, index (B,) int64, lengths (B,) int32)``; ``lengths`` is what
    ``PointMamba(..., lengths=)`` takes, rows behind it are 0 and their point labels -1.  ``out``: a Batch of an
    earlier call to write into.  ``state`` is the ``AugmentState``-shaped device tensor ``[seed, step]``; ``step`` and
    ``epoch`` read it back (a synchronisation: for tests and logging), ``manual_seed`` rewinds it.  Iterating yields
    ``len(loader)`` fetches.

    Nothing is read on the host, so ``fetch`` can be captured.  Inside ``GraphedTrainStep`` the loader takes the place
    of the static inputs; the step wants at least one, so hand it a dummy:

        loader = DeviceLoader(train_set, 64, 1024, normalize="unit_sphere", seed=seed)     # before the capture
        aug = AugmentState(seed, device)
        def loss_fn(_):
            batch = loader.fetch()
            pts = sample_and_augment(batch.points, train_transforms, state=aug)
            return criterion(model(pts), batch.label)
        step = GraphedTrainStep(loss_fn, optimizer, (torch.zeros(1, device=device),))
        loader.manual_seed(seed)              # the warm-up steps ran eagerly and took batches: back to step 0
        for _ in range(epochs * len(loader)):
            loss = step()                     # the next batch of the epoch's order; no input is copied
    """

    def __init__(self, dataset, batch_size, npoints, shuffle=True, drop_last=True, subsample="permute", normalize=None,
                 first=0, seed=0, rank=0, world=1):
        what = "DeviceLoader"
        if not isinstance(dataset, DeviceDataset):
            raise TypeError(f"{what}: dataset must be a DeviceDataset, got {type(dataset).__name__}")
        if subsample not in _ROWS:
            raise ValueError(f"{what}: subsample must be one of {sorted(_ROWS)}, got {subsample!r}")
        if normalize not in _NORM:
            raise ValueError(f"{what}: normalize must be None or 'unit_sphere', got {normalize!r}")
        batch_size, npoints, first, rank, world = int(batch_size), int(npoints), int(first), int(rank), int(world)
        if batch_size < 1 or not 1 <= npoints <= _lib.DS_MAX_POINTS or first < 0 or world < 1 or not 0 <= rank < world:
            raise ValueError(f"{what}: need batch_size >= 1, 1 <= npoints <= {_lib.DS_MAX_POINTS}, first >= 0 and "
                             f"0 <= rank < world, got {batch_size}, {npoints}, {first}, {rank}, {world}")
        S, per_step = len(dataset), batch_size * world
        if drop_last and S < per_step:
            raise ValueError(f"{what}: {S} clouds are fewer than one step of {batch_size} x {world} with drop_last")
        self.dataset, self.batch_size, self.npoints, self.first = dataset, batch_size, npoints, first
        self.shuffle, self.drop_last, self.subsample, self.normalize = bool(shuffle), bool(drop_last), subsample, normalize
        self.rank, self.world = rank, world
        self.steps_per_epoch = S // per_step if drop_last else -(-S // per_step)
        self.state = AugmentState(seed, dataset.device)

    def __len__(self):
        return self.steps_per_epoch

    @property
    def step(self):
        return self.state.step

    @property
    def epoch(self):
        return self.state.step // self.steps_per_epoch

    def manual_seed(self, seed, step=0):
        """Set the seed and put the step back to ``step`` (``epoch * len(loader)`` resumes at an epoch)."""
        self.state.manual_seed(seed, step)
        return self

    def _empty(self):
        ds, B, K, dev = self.dataset, self.batch_size, self.npoints, self.dataset.device
        return Batch(torch.empty(B, K, 3, device=dev, dtype=torch.float32),
                     None if ds.labels is None else torch.empty(B, device=dev, dtype=torch.int64),
                     None if ds.point_labels is None else torch.empty(B, K, device=dev, dtype=torch.int32),
                     torch.empty(B, device=dev, dtype=torch.int64), torch.empty(B, device=dev, dtype=torch.int32))

    def _check_out(self, out):
        what = "DeviceLoader.fetch"
        ds, B, K, dev = self.dataset, self.batch_size, self.npoints, self.dataset.device
        if not isinstance(out, Batch):
            raise TypeError(f"{what}: out must be a Batch of an earlier fetch, got {type(out).__name__}")
        want = Batch(((B, K, 3), torch.float32), None if ds.labels is None else ((B,), torch.int64),
                     None if ds.point_labels is None else ((B, K), torch.int32), ((B,), torch.int64), ((B,), torch.int32))
        for name, t, w in zip(Batch._fields, out, want):
            if (t is None) != (w is None):
                raise ValueError(f"{what}: out.{name} does not match the dataset (labels it has or has not)")
            if t is None:
                continue
            _lib.require_gpu(t, what)
            if tuple(t.shape) != w[0] or t.dtype != w[1] or t.device != dev or not t.is_contiguous():
                raise ValueError(f"{what}: out.{name} must be a contiguous {w[0]} {w[1]} tensor on {dev}")

    def fetch(self, out=None):
        """The batch of the state's step, in one launch; the step advances by 1.  Returns a ``Batch``."""
        ds = self.dataset
        if out is None:
            out = self._empty()
        else:
            self._check_out(out)
        _lib.count("dataset_fetch")
        _lib.call("simamba_dataset_fetch", ds.points, ds.offsets, ds.labels, ds.point_labels, self.state.tensor,
                  out.points, out.label, out.point_label, out.index, out.lengths, ds.points.shape[0], len(ds), ds.stride,
                  self.batch_size, self.npoints, self.first, self.steps_per_epoch, self.rank, self.world,
                  _lib.DS_SHUFFLE if self.shuffle else _lib.DS_SEQUENTIAL, _ROWS[self.subsample],
                  _NORM[self.normalize], device=ds.device, time_as="dataset_fetch")
        return out

    def __iter__(self):
        for _ in range(self.steps_per_epoch):
            yield self.fetch()


def keyed_perm(n, seed, stream, first=0, count=None):
    """``perm(n, seed, stream, first .. first + count - 1)`` of csrc/keyed_perm.h on the HOST, as an int64 numpy array:
    the bijection the loader shuffles and samples with, for tests and for reconstructing an epoch's order."""
    import ctypes
    count = n - first if count is None else count
    out = np.empty(max(count, 0), dtype=np.int64)
    seed, stream = int(seed) & _MASK64, int(stream) & _MASK64
    as_i64 = lambda v: v - (1 << 64) if v >= 1 << 63 else v      # noqa: E731
    rc = _lib.load().simamba_keyed_perm(as_i64(seed), as_i64(stream), n, first, count,
                                        out.ctypes.data_as(ctypes.c_void_p))
    _lib.check(rc, "simamba_keyed_perm")
    return out
