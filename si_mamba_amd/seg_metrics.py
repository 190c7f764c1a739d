"""Part-segmentation scoring on the device (csrc/part_metrics.hip): the restricted argmax and the four numbers every
ShapeNetPart paper reports, the reference's evaluation loop (part_segmentation/main.py:269-334) without its host copy
and Python loops.

The label of a point is chosen only among the parts of its shape's category; a part that is neither present nor
predicted counts as IoU 1; ties go to the lower label.  ``part_seg_eval`` scores one batch, ``PartSegMetrics``
accumulates a whole evaluation pass with no host read until ``compute()``.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib

MAX_PARTS = 16      # parts per category (the kernel's register counters)
MAX_LABELS = 256    # C


class PartTable:
    """The categories of a part-segmentation label space: ``names[i]`` owns the labels
    ``first[i] .. first[i] + count[i] - 1``.  Categories are kept in ascending label order, which for ShapeNetPart is
    the dataset's own category index (Airplane 0 ... Table 15)."""

    def __init__(self, names, first, count):
        self.names, self.first, self.count = tuple(names), tuple(first), tuple(count)
        self.num_labels = sum(self.count)
        self.label_category = tuple(i for i, n in enumerate(self.count) for _ in range(n))
        self._on = {}

    @classmethod
    def from_label_lists(cls, seg_classes):
        """From the reference's form, ``{name: [labels]}`` (main.py:32-35).  The reference's restricted argmax adds
        ``seg_classes[cat][0]`` to an index into the category's columns, which is right only when every category's
        labels are a contiguous ascending run; and every label has to belong to exactly one category.  ValueError
        otherwise, and for a category of more than 16 parts or a table of more than 256 labels."""
        rows = []
        for name, labels in seg_classes.items():
            labels = [int(l) for l in labels]
            if not labels:
                raise ValueError(f"part table: category {name!r} has no labels")
            if labels != list(range(labels[0], labels[0] + len(labels))):
                raise ValueError(f"part table: the labels of {name!r} are not a contiguous ascending run: {labels}")
            if len(labels) > MAX_PARTS:
                raise ValueError(f"part table: {name!r} has {len(labels)} parts, at most {MAX_PARTS} are supported")
            rows.append((labels[0], len(labels), str(name)))
        if not rows:
            raise ValueError("part table: no categories")
        rows.sort()
        nxt = 0
        for first, count, name in rows:
            if first != nxt:
                raise ValueError(f"part table: the categories do not partition range(C): {name!r} starts at {first}, "
                                 f"the labels before it end at {nxt - 1} ({'overlap' if first < nxt else 'gap'})")
            nxt = first + count
        if nxt > MAX_LABELS:
            raise ValueError(f"part table: {nxt} labels, at most {MAX_LABELS} are supported")
        return cls([r[2] for r in rows], [r[0] for r in rows], [r[1] for r in rows])

    def __len__(self):
        return len(self.names)

    def as_label_lists(self):
        return {n: list(range(f, f + c)) for n, f, c in zip(self.names, self.first, self.count)}

    def on(self, device):
        """(first int32 (ncat), count int32 (ncat), label -> category int64 (C)) on ``device``; made once per device.
        The first call copies from the host: make it before capturing a graph."""
        device = torch.device(device)
        got = self._on.get(device)
        if got is None:
            got = (torch.tensor(self.first, dtype=torch.int32, device=device),
                   torch.tensor(self.count, dtype=torch.int32, device=device),
                   torch.tensor(self.label_category, dtype=torch.int64, device=device))
            self._on[device] = got
        return got


SHAPENETPART = PartTable(
    ["Airplane", "Bag", "Cap", "Car", "Chair", "Earphone", "Guitar", "Knife", "Lamp", "Laptop", "Motorbike", "Mug",
     "Pistol", "Rocket", "Skateboard", "Table"],
    [0, 4, 6, 8, 12, 16, 19, 22, 24, 28, 30, 36, 38, 41, 44, 47],
    [4, 2, 2, 4, 4, 3, 3, 2, 4, 2, 6, 2, 3, 3, 3, 3])

PartSegEval = namedtuple("PartSegEval", ["pred", "inter", "uni", "shape_iou", "correct", "seen_class",
                                         "correct_class", "category"])


def _is_index(t):
    return not (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool)


def _check(what, scores, target, category, table, lengths):
    if not isinstance(table, PartTable):
        raise ValueError(f"{what}: table must be a PartTable, got {type(table).__name__}")
    if scores.dim() != 3 or scores.shape[0] < 1 or scores.shape[1] < 1:
        raise ValueError(f"{what}: scores must be (B, N, C) with B, N >= 1, got {tuple(scores.shape)}")
    B, N, C = scores.shape
    if C != table.num_labels:
        raise ValueError(f"{what}: scores have {C} labels, the table has {table.num_labels}")
    if scores.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{what}: scores must be float32 or bfloat16, got {scores.dtype}")
    if tuple(target.shape) != (B, N) or not _is_index(target):
        raise ValueError(f"{what}: target must be ({B}, {N}) integers, got {tuple(target.shape)} {target.dtype}")
    if category is not None and (tuple(category.shape) != (B,) or not _is_index(category)):
        raise ValueError(f"{what}: category must be ({B},) integers, got {tuple(category.shape)} {category.dtype}")
    if lengths is not None and (tuple(lengths.shape) != (B,) or not _is_index(lengths)):
        raise ValueError(f"{what}: lengths must be ({B},) integers, got {tuple(lengths.shape)} {lengths.dtype}")
    for t in (scores, target, category, lengths):
        if t is not None:
            _lib.require_gpu(t, what)


def _launch(scores, target, category, table, lengths, return_pred, seen_class=None, correct_class=None):
    """The call itself, on arguments that passed _check; seen_class / correct_class: the totals to add into."""
    B, N, C = scores.shape
    dev = scores.device
    scores = scores.contiguous()
    target = target.long().contiguous()
    lengths = None if lengths is None else lengths.long().contiguous()
    tfirst, tcount, label_cat = table.on(dev)
    if category is None:
        category = label_cat[target[:, 0].clamp(0, C - 1)]            # a device gather: nothing is read on the host
    else:
        category = category.long().clamp(0, len(table) - 1)
    first, count = tfirst[category], tcount[category]
    pred = torch.empty(B, N, device=dev, dtype=torch.int64) if return_pred else None
    inter = torch.empty(B, MAX_PARTS, device=dev, dtype=torch.int32)
    uni = torch.empty(B, MAX_PARTS, device=dev, dtype=torch.int32)
    shape_iou = torch.empty(B, device=dev, dtype=torch.float64)
    correct = torch.empty(B, device=dev, dtype=torch.int32)
    if seen_class is None:
        seen_class = torch.zeros(C, device=dev, dtype=torch.int64)
        correct_class = torch.zeros(C, device=dev, dtype=torch.int64)
    _lib.count("part_seg_eval")
    _lib.call("simamba_part_seg_eval", scores, target, first, count, lengths, pred, inter, uni, shape_iou, correct,
              seen_class, correct_class, B, N, C, _lib.dtype_code(scores.dtype), device=dev, time_as="part_seg_eval")
    return PartSegEval(pred, inter, uni, shape_iou, correct, seen_class, correct_class, category)


def part_seg_eval(scores, target, category=None, *, table=SHAPENETPART, lengths=None, return_pred=True):
    """Score one batch of part-segmentation output on the device.

    ``scores`` (B, N, C) float32 or bfloat16: log-probabilities or logits, only their order matters.  ``target`` (B, N)
    integers, the true part labels.  ``category`` (B,) integers indexing ``table`` (values outside it are clamped into
    it); None: the category that owns ``target[b, 0]``, as the reference takes it (main.py:296, :311), looked up on the
    device.  ``lengths`` (B,) integers or None: shape ``b`` is its first ``lengths[b]`` points (clamped to [1, N]);
    nothing at or behind a length is read.

    Returns the named tuple ``PartSegEval``:
      pred (B, N) int64   the category's first label + the argmax over the category's columns: the first maximum, a NaN
                          greater than every number (numpy's argmax); -1 behind a length.  None with return_pred=False.
      inter, uni (B, 16) int32   per part of the shape's category: points with target == l and pred == l, and with
                          target == l or pred == l; columns beyond the category's parts are 0.
      shape_iou (B,) float64     the mean over the category's parts of inter / uni, an absent and unpredicted part
                          counting 1.0.
      correct (B,) int32  points with pred == target.
      seen_class, correct_class (C,) int64   over the batch: points with target == l, and with pred == l == target.
      category (B,) int64 the category used.
    A target outside the shape's category matches no prediction but counts in seen_class; one outside [0, C) counts
    nowhere.  Integer counting until the last division, no float atomics: the same bits every call.  Nothing is read
    on the host, so the call can be captured in a graph behind the model's forward (after one call outside the
    capture, which puts the table on the device)."""
    _check("part_seg_eval", scores, target, category, table, lengths)
    return _launch(scores, target, category, table, lengths, return_pred)


class PartSegMetrics:
    """The accumulator of one evaluation pass: ``update`` per batch, ``compute`` once at the end.

    The state is a handful of device tensors: per category the float64 sum of the shape IoUs and the number of shapes,
    the correct and seen points, and per label ``seen_class`` / ``correct_class``.  ``update`` reads nothing on the
    host and does not synchronise, so it can be captured in a graph; the first ``update`` (or ``device=`` here) creates
    the state and copies the table to the device, which has to happen outside a capture.  Everything but the IoU sums
    is an integer; the IoU sums are added with ordinary (atomic-free) reductions, so a pass gives the same bits every
    run."""

    def __init__(self, table=SHAPENETPART, device=None):
        if not isinstance(table, PartTable):
            raise ValueError(f"PartSegMetrics: table must be a PartTable, got {type(table).__name__}")
        self.table = table
        self._state = None
        if device is not None:
            self._init(torch.device(device))

    _FIELDS = ("iou_sum", "shape_count", "correct", "seen", "seen_class", "correct_class")

    def _init(self, device):
        ncat, C = len(self.table), self.table.num_labels
        z = lambda n, dt: torch.zeros(n, device=device, dtype=dt)      # noqa: E731
        self._state = dict(iou_sum=z(ncat, torch.float64), shape_count=z(ncat, torch.int64), correct=z(1, torch.int64),
                           seen=z(1, torch.int64), seen_class=z(C, torch.int64), correct_class=z(C, torch.int64))
        self._cats = torch.arange(ncat, device=device)
        self.table.on(device)

    def state(self):
        """The state tensors by name (None before the first update)."""
        return self._state

    def update(self, scores, target, category=None, lengths=None):
        """Add a batch (the arguments of ``part_seg_eval``).  No host read, no synchronisation."""
        _check("PartSegMetrics.update", scores, target, category, self.table, lengths)
        if self._state is None:
            self._init(scores.device)
        s = self._state
        r = _launch(scores, target, category, self.table, lengths, False, s["seen_class"], s["correct_class"])
        B, N, _ = scores.shape
        onehot = r.category[:, None] == self._cats[None, :]                      # (B, ncat)
        s["iou_sum"] += (onehot.to(torch.float64) * r.shape_iou[:, None]).sum(0)
        s["shape_count"] += onehot.sum(0)
        s["correct"] += r.correct.sum(dtype=torch.int64)
        s["seen"] += B * N if lengths is None else lengths.long().clamp(1, N).sum()
        return self

    def merge_(self, other):
        """Add another accumulator's state (same table).  The IoU sums are float64 additions: the merged sums are those
        of one accumulator fed everything up to the rounding of a different order of additions."""
        if other.table is not self.table and other.table.as_label_lists() != self.table.as_label_lists():
            raise ValueError("PartSegMetrics.merge_: the accumulators have different tables")
        if other._state is None:
            return self
        if self._state is None:
            self._init(other._state["seen"].device)
        for k in self._FIELDS:
            self._state[k] += other._state[k].to(self._state[k].device)
        return self

    def all_reduce_(self, group=None):
        """Sum the state over the ranks of ``group`` (torch.distributed, initialised by the caller)."""
        import torch.distributed as dist
        if self._state is None:
            raise RuntimeError("PartSegMetrics.all_reduce_: no state yet; construct with device= or update first, "
                               "so that every rank takes part")
        for k in self._FIELDS:
            dist.all_reduce(self._state[k], op=dist.ReduceOp.SUM, group=group)
        return self

    def reset(self):
        if self._state is not None:
            for t in self._state.values():
                t.zero_()
        return self

    def compute(self):
        """The single host read.  Returns the reference's four keys, spelled as the reference spells them, plus
        ``category_iou``:
          accuracy            correct points / seen points
          class_avg_accuracy  mean over the C labels of correct_class / seen_class; as in the reference it is NaN when
                              some label never occurred in the targets (0 / 0)
          class_avg_iou       mean over the categories of the category's mean shape IoU.  A category with no shapes is
                              left out of it and reported as NaN in category_iou (the reference takes np.mean of an
                              empty list there: a warning, and NaN for the whole average)
          inctance_avg_iou    mean of the shape IoU over all shapes
          category_iou        {name: the category's mean shape IoU}
        Before any update every value is NaN."""
        import numpy as np
        ncat, C = len(self.table), self.table.num_labels
        nan = float("nan")
        if self._state is None:
            return dict(accuracy=nan, class_avg_accuracy=nan, class_avg_iou=nan, inctance_avg_iou=nan,
                        category_iou={n: nan for n in self.table.names})
        s = self._state
        flat = torch.cat([s["iou_sum"].view(torch.int64)] + [s[k] for k in self._FIELDS[1:]]).cpu().numpy()
        iou_sum = flat[:ncat].view(np.float64)
        shape_count = flat[ncat:2 * ncat]
        correct, seen = int(flat[2 * ncat]), int(flat[2 * ncat + 1])
        seen_class = flat[2 * ncat + 2:2 * ncat + 2 + C]
        correct_class = flat[2 * ncat + 2 + C:]
        with np.errstate(divide="ignore", invalid="ignore"):
            cat_iou = iou_sum / shape_count.astype(np.float64)
            class_acc = np.mean(correct_class / seen_class.astype(np.float64))
        have = shape_count > 0
        return dict(accuracy=correct / float(seen) if seen else nan,
                    class_avg_accuracy=float(class_acc),
                    class_avg_iou=float(np.mean(cat_iou[have])) if have.any() else nan,
                    inctance_avg_iou=float(iou_sum.sum() / float(shape_count.sum())) if have.any() else nan,
                    category_iou={n: float(v) for n, v in zip(self.table.names, cat_iou)})
