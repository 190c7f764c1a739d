"""CPU: the part-segmentation scoring entry point (csrc/part_metrics.hip) validates its arguments before touching a
device, the category table equals the reference's, the Python route refuses CPU tensors after checking its arguments,
and the numpy restatement the GPU tests compare against (part_metrics_ref.py) gives the hand-worked answers."""
import json
import os

import numpy as np
import pytest
import torch

import part_metrics_ref as pr
from abi_tables import E_DTYPE, E_NULLPTR, E_SHAPE, P, check_rows
from conftest import GOLDEN
from si_mamba_amd import _lib

ARGS = dict(scores=P, target=P, part_first=P, part_count=P, lengths=None, pred=None, inter=P, uni=P, shape_iou=P,
            correct=P, seen_class=P, correct_class=P, batch=16, n=2048, c=50, io_dtype=_lib.F32, stream=None)
REQUIRED = ["scores", "target", "part_first", "part_count", "inter", "uni", "shape_iou", "correct", "seen_class",
            "correct_class"]

ROWS = [
    (dict(c=0), E_SHAPE), (dict(c=-1), E_SHAPE), (dict(c=257), E_SHAPE), (dict(n=0), E_SHAPE), (dict(n=-4), E_SHAPE),
    (dict(batch=0), E_SHAPE), (dict(batch=-1), E_SHAPE), (dict(batch=1 << 31), E_SHAPE), (dict(batch=1 << 40), E_SHAPE),
    (dict(io_dtype=2), E_DTYPE), (dict(io_dtype=-1), E_DTYPE),
    *[({k: None}, E_NULLPTR) for k in REQUIRED],
    # the limits of c and both element types, with a null pointer so that nothing is launched
    (dict(c=1, scores=None), E_NULLPTR), (dict(c=256, scores=None), E_NULLPTR),
    (dict(c=256, io_dtype=_lib.BF16, target=None), E_NULLPTR), (dict(n=1, batch=1, uni=None), E_NULLPTR),
    (dict(batch=(1 << 31) - 1, correct=None), E_NULLPTR),
    # two faults: the shape in front of the null pointers, the dtype in front of them too
    (dict(c=257, scores=None), E_SHAPE), (dict(c=0, target=None), E_SHAPE), (dict(n=0, inter=None), E_SHAPE),
    (dict(batch=0, shape_iou=None), E_SHAPE), (dict(batch=1 << 40, seen_class=None), E_SHAPE),
    (dict(io_dtype=7, scores=None), E_DTYPE), (dict(c=257, io_dtype=7), E_SHAPE),
]


def test_return_codes_without_a_device():
    check_rows("simamba_part_seg_eval", ARGS, ROWS)


def _fixture():
    with open(os.path.join(GOLDEN, "shapenetpart_seg_classes.json")) as fh:
        return json.load(fh)


def test_shapenetpart_table_equals_the_reference():
    from si_mamba_amd import SHAPENETPART, PartTable
    ref = _fixture()
    assert len(ref) == 16 and len(SHAPENETPART) == 16 and SHAPENETPART.num_labels == 50
    assert set(SHAPENETPART.names) == set(ref)
    for name, first, count in zip(SHAPENETPART.names, SHAPENETPART.first, SHAPENETPART.count):
        assert list(range(first, first + count)) == ref[name], name
    assert list(SHAPENETPART.first) == sorted(SHAPENETPART.first)              # the dataset's category index
    for label, cat in enumerate(SHAPENETPART.label_category):
        assert label in ref[SHAPENETPART.names[cat]]
    built = PartTable.from_label_lists(ref)
    assert (built.names, built.first, built.count) == (SHAPENETPART.names, SHAPENETPART.first, SHAPENETPART.count)
    assert built.as_label_lists() == {k: ref[k] for k in built.names}
    t = pr.Table(ref)
    assert t.names == list(SHAPENETPART.names) and list(t.first) == list(SHAPENETPART.first)
    assert list(t.count) == list(SHAPENETPART.count) and list(t.label_category) == list(SHAPENETPART.label_category)


@pytest.mark.parametrize("bad", [
    {"a": [0, 1], "b": [3, 4]},                  # a gap
    {"a": [0, 1, 2], "b": [2, 3]},               # an overlap
    {"a": [1, 0], "b": [2, 3]},                  # a descending run
    {"a": [0, 2], "b": [1, 3]},                  # not contiguous
    {"a": [1, 2], "b": [3]},                     # does not cover range(C): label 0 is nobody's
    {"a": [0, 1], "b": []},                      # an empty category
    {"a": list(range(17))},                      # more parts than the kernel counts
    {},
])
def test_table_constructor_refuses(bad):
    from si_mamba_amd import PartTable
    with pytest.raises(ValueError):
        PartTable.from_label_lists(bad)


def test_table_constructor_accepts_a_partition_in_any_order():
    from si_mamba_amd import PartTable
    t = PartTable.from_label_lists({"two": [17, 18], "one": [0], "sixteen": list(range(1, 17))})
    assert (t.names, t.first, t.count, t.num_labels) == (("one", "sixteen", "two"), (0, 1, 17), (1, 16, 2), 19)


def test_python_route_refuses_cpu_tensors():
    from si_mamba_amd import PartSegMetrics, part_seg_eval
    scores, target = torch.zeros(2, 8, 50), torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        part_seg_eval(scores, target)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        part_seg_eval(scores.bfloat16(), target, torch.zeros(2, dtype=torch.int64), lengths=torch.tensor([3, 8]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PartSegMetrics().update(scores, target)
    assert np.isnan(PartSegMetrics().compute()["accuracy"])


def test_python_route_checks_its_arguments_first():
    from si_mamba_amd import PartSegMetrics, part_seg_eval
    z = torch.zeros
    i64 = torch.int64
    bad = [
        (z(2, 8, 49), z(2, 8, dtype=i64), {}),                                   # C is not the table's
        (z(2, 8), z(2, 8, dtype=i64), {}), (z(0, 8, 50), z(0, 8, dtype=i64), {}), (z(2, 0, 50), z(2, 0, dtype=i64), {}),
        (z(2, 8, 50), z(2, 7, dtype=i64), {}), (z(2, 8, 50), z(2, 8), {}),       # target: shape, float
        (z(2, 8, 50, dtype=torch.float64), z(2, 8, dtype=i64), {}), (z(2, 8, 50, dtype=torch.float16), z(2, 8, dtype=i64), {}),
        (z(2, 8, 50), z(2, 8, dtype=i64), dict(category=z(3, dtype=i64))),
        (z(2, 8, 50), z(2, 8, dtype=i64), dict(category=z(2))),
        (z(2, 8, 50), z(2, 8, dtype=i64), dict(lengths=z(2, 1, dtype=i64))),
        (z(2, 8, 50), z(2, 8, dtype=i64), dict(lengths=z(2))),
    ]
    for scores, target, kw in bad:
        with pytest.raises(ValueError):
            part_seg_eval(scores, target, **kw)
        with pytest.raises(ValueError):
            PartSegMetrics().update(scores, target, **kw)
    with pytest.raises(ValueError):
        part_seg_eval(z(2, 8, 50), z(2, 8, dtype=i64), table={"a": [0]})


# ---- the restatement against cases worked by hand -------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
HAND_TABLE = {"B": [3, 4], "A": [0, 1, 2]}
# shape 0, category A (labels 0 1 2; columns 3 4 are another category's and hold the largest scores of every row):
#   point  scores over A        pred   target
#   0      .5  .1  .0           0      0      correct
#   1      .2  .2  .1           0      0      a tie: the lower label
#   2      .0  nan .9           1      1      a NaN is above every number
#   3      .7  .1  .3           0      1      wrong
#   4      .1  .9  .2           1      4      a target of another category: no match, still seen
#   part 0: target {0 1}, pred {0 1 3}: 2 / 3;  part 1: target {2 3}, pred {2 4}: 1 / 3;  part 2: absent, unpredicted: 1
# shape 1, category B (labels 3 4), every target 3:
#   0      -inf -inf            3      a tie of -inf      1   +inf 1 -> 3      2   .1 -inf -> 3
#   3      -inf 0 -> 4          4   1 2 -> 4
#   part 3: target {0..4}, pred {0 1 2}: 3 / 5;  part 4: absent but predicted: 0 / 2
HAND_SCORES = np.array([
    [[.5, .1, .0, 9, 9], [.2, .2, .1, 9, 9], [.0, NAN, .9, 9, 9], [.7, .1, .3, 9, 9], [.1, .9, .2, 9, 9]],
    [[9, 9, 9, -INF, -INF], [9, 9, 9, INF, 1], [9, 9, 9, .1, -INF], [9, 9, 9, -INF, 0], [9, 9, 9, 1, 2]]])
HAND_TARGET = np.array([[0, 0, 1, 1, 4], [3, 3, 3, 3, 3]])


def test_restatement_on_hand_worked_cases():
    table = pr.Table(HAND_TABLE)
    assert table.names == ["A", "B"] and list(table.label_category) == [0, 0, 0, 1, 1]
    for category in (None, [0, 1]):
        p = pr.Pass(table)
        r = p.add(HAND_SCORES, HAND_TARGET, category)
        assert r["pred"].tolist() == [[0, 0, 1, 0, 1], [3, 3, 3, 4, 4]]
        assert r["inter"][:, :3].tolist() == [[2, 1, 0], [3, 0, 0]] and not r["inter"][:, 3:].any()
        assert r["uni"][:, :3].tolist() == [[3, 3, 0], [5, 2, 0]] and not r["uni"][:, 3:].any()
        assert r["shape_iou"].tolist() == [(2 / 3 + 1 / 3 + 1.0) / 3, (3 / 5 + 0.0) / 2]
        assert r["correct"].tolist() == [3, 3]
        assert r["seen_class"].tolist() == [2, 2, 0, 5, 1] and r["correct_class"].tolist() == [2, 1, 0, 3, 0]
        got = p.result()
        iou = r["shape_iou"]
        assert got["accuracy"] == 6 / 10 and np.isnan(got["class_avg_accuracy"])          # label 2 never occurs
        assert got["category_iou"] == {"A": iou[0], "B": iou[1]}
        assert got["class_avg_iou"] == got["inctance_avg_iou"] == np.mean([iou[0], iou[1]])
    # lengths: shape 0 is its first three points (the padding is never looked at), shape 1 all five (7 is clamped)
    r = pr.evaluate_batch(table, HAND_SCORES, HAND_TARGET, None, lengths=[3, 7])
    assert r["pred"].tolist() == [[0, 0, 1, -1, -1], [3, 3, 3, 4, 4]] and r["seen"] == 8
    assert r["shape_iou"].tolist() == [(1.0 + 1.0 + 1.0) / 3, (3 / 5 + 0.0) / 2] and r["correct"].tolist() == [3, 3]
    assert r["seen_class"].tolist() == [2, 1, 0, 5, 0]
    # a category that no shape belongs to is NaN by name and left out of the class average
    p = pr.Pass(table)
    p.add(HAND_SCORES[:1], HAND_TARGET[:1])
    got = p.result()
    assert np.isnan(got["category_iou"]["B"]) and got["class_avg_iou"] == got["category_iou"]["A"]


def test_restatement_shape_iou_is_np_mean_below_eight_parts():
    rng = np.random.default_rng(0)
    for count in range(1, 8):
        for _ in range(50):
            uni = rng.integers(0, 40, count)
            inter = np.minimum(rng.integers(0, 40, count), uni)
            ious = [1.0 if u == 0 else i / float(u) for i, u in zip(inter, uni)]
            assert pr.shape_iou(inter, uni, count) == np.mean(ious)
