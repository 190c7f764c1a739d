"""Host restatement of part-segmentation scoring, the yardstick of tests/test_part_metrics_abi.py and
tests/test_gpu_part_metrics.py: what the reference's evaluation loop computes (part_segmentation/main.py:269-334), in
numpy on float64 / int64, with this project's ``lengths`` extension (shape b is its first lengths[b] points, clamped to
[1, N]; nothing behind them is looked at).

  restricted_argmax   the label of every point, chosen among the labels of the shape's category only
  batch_counts        per shape and part inter / uni, the shape IoU, correct points; per label seen / correct
  Pass                the accumulation over batches and the four averages

The shape IoU is summed the way the device is specified to: divide, add in part order, divide by the number of parts,
in Python floats.  For fewer than 8 parts (every ShapeNetPart category) that is np.mean of the list bit for bit, which
is what the reference calls; from 8 parts on np.mean adds in another order (eight running sums).
"""
import numpy as np

MAX_PARTS = 16


class Table:
    """{name: [labels]} (the reference's seg_classes) -> categories in ascending label order: names, first, count and
    the label -> category map."""

    def __init__(self, seg_classes):
        rows = sorted((labels[0], len(labels), name) for name, labels in seg_classes.items())
        self.names = [r[2] for r in rows]
        self.first = np.array([r[0] for r in rows], dtype=np.int64)
        self.count = np.array([r[1] for r in rows], dtype=np.int64)
        self.num_labels = int(self.count.sum())
        self.label_category = np.repeat(np.arange(len(rows)), self.count)
        assert list(self.label_category) == [c for c, r in enumerate(rows) for _ in range(r[1])]
        for f, n, name in rows:
            assert list(seg_classes[name]) == list(range(f, f + n)), name


def clamp_lengths(lengths, B, N):
    if lengths is None:
        return np.full(B, N, dtype=np.int64)
    return np.clip(np.asarray(lengths, dtype=np.int64), 1, N)


def restricted_argmax(scores, first, count, lengths=None):
    """scores (B, N, C) -> pred (B, N) int64: first[b] + np.argmax over the columns first[b] .. first[b] + count[b] - 1
    (the first maximum; NaN above every number, the first NaN wins); -1 behind a length."""
    scores = np.asarray(scores, dtype=np.float64)
    B, N, _ = scores.shape
    lens = clamp_lengths(lengths, B, N)
    pred = np.full((B, N), -1, dtype=np.int64)
    for b in range(B):
        f, c, n = int(first[b]), int(count[b]), int(lens[b])
        pred[b, :n] = np.argmax(scores[b, :n, f:f + c], axis=1) + f
    return pred


def shape_iou(inter, uni, count):
    total = 0.0
    for k in range(count):
        total += 1.0 if uni[k] == 0 else int(inter[k]) / float(int(uni[k]))
    return total / count


def batch_counts(pred, target, first, count, num_labels, lengths=None):
    target = np.asarray(target, dtype=np.int64)
    B, N = target.shape
    lens = clamp_lengths(lengths, B, N)
    inter = np.zeros((B, MAX_PARTS), dtype=np.int64)
    uni = np.zeros((B, MAX_PARTS), dtype=np.int64)
    iou = np.zeros(B, dtype=np.float64)
    correct = np.zeros(B, dtype=np.int64)
    seen_class = np.zeros(num_labels, dtype=np.int64)
    correct_class = np.zeros(num_labels, dtype=np.int64)
    valid = np.arange(N)[None, :] < lens[:, None]
    allp, alll = pred[valid], target[valid]
    for l in range(num_labels):
        seen_class[l] = np.sum(alll == l)
        correct_class[l] = np.sum((allp == l) & (alll == l))
    for b in range(B):
        n, f, c = int(lens[b]), int(first[b]), int(count[b])
        segp, segl = pred[b, :n], target[b, :n]
        correct[b] = np.sum(segp == segl)
        for k in range(c):
            inter[b, k] = np.sum((segl == f + k) & (segp == f + k))
            uni[b, k] = np.sum((segl == f + k) | (segp == f + k))
        iou[b] = shape_iou(inter[b], uni[b], c)
    return dict(inter=inter, uni=uni, shape_iou=iou, correct=correct, seen_class=seen_class,
                correct_class=correct_class)


def evaluate_batch(table, scores, target, category=None, lengths=None):
    """One batch: pred, the counts of batch_counts and the category of every shape (given, or the one that owns
    target[b, 0] as in the reference)."""
    target = np.asarray(target, dtype=np.int64)
    if category is None:
        category = table.label_category[target[:, 0]]
    category = np.asarray(category, dtype=np.int64)
    first, count = table.first[category], table.count[category]
    pred = restricted_argmax(scores, first, count, lengths)
    out = batch_counts(pred, target, first, count, table.num_labels, lengths)
    out.update(pred=pred, category=category, seen=int(clamp_lengths(lengths, *target.shape).sum()))
    return out


class Pass:
    """The reference's accumulation over an evaluation pass and its four averages.  A category without shapes is left
    out of class_avg_iou and is NaN in category_iou (the reference would take np.mean of an empty list there)."""

    def __init__(self, table):
        self.table = table
        self.total_correct = 0
        self.total_seen = 0
        self.seen_class = np.zeros(table.num_labels, dtype=np.int64)
        self.correct_class = np.zeros(table.num_labels, dtype=np.int64)
        self.shape_ious = {name: [] for name in table.names}

    def add(self, scores, target, category=None, lengths=None):
        r = evaluate_batch(self.table, scores, target, category, lengths)
        self.total_correct += int(r["correct"].sum())
        self.total_seen += r["seen"]
        self.seen_class += r["seen_class"]
        self.correct_class += r["correct_class"]
        for b, c in enumerate(r["category"]):
            self.shape_ious[self.table.names[c]].append(float(r["shape_iou"][b]))
        return r

    def num_shapes(self):
        return sum(len(v) for v in self.shape_ious.values())

    def result(self):
        every = [v for ious in self.shape_ious.values() for v in ious]
        cat = {name: (float(np.mean(ious)) if ious else float("nan")) for name, ious in self.shape_ious.items()}
        have = [v for name, v in cat.items() if self.shape_ious[name]]
        with np.errstate(divide="ignore", invalid="ignore"):
            class_acc = float(np.mean(self.correct_class / self.seen_class.astype(np.float64)))
        return dict(accuracy=self.total_correct / float(self.total_seen), class_avg_accuracy=class_acc,
                    class_avg_iou=float(np.mean(have)), inctance_avg_iou=float(np.mean(every)), category_iou=cat)
