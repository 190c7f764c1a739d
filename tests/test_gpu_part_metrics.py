"""GPU: part-segmentation scoring (csrc/part_metrics.hip, si_mamba_amd/seg_metrics.py) against the numpy restatement
of the reference's evaluation loop (part_metrics_ref.py).  Everything up to the last division is integer counting, so
the comparison is by equality: pred, inter, uni, correct, seen_class and correct_class exactly, shape_iou bit for bit.
compute()'s IoU averages are sums of n float64 values in [0, 1] taken in another order than numpy's pairwise one:
each of the two sums is within (n - 1) 2^-53 relative of the exact one, each final division adds 2^-53, so they agree
within n 2^-52 relative, n the number of shapes averaged.  The two accuracies are quotients of equal integers: equal."""
import json
import os

import numpy as np
import pytest
import torch

import part_metrics_ref as pr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "shapenetpart_seg_classes.json")) as _fh:
    SHAPENET = json.load(_fh)
MADE_UP = {"one": [0], "sixteen": list(range(1, 17)), "two": [17, 18]}      # C = 19: 1 part, 16 parts, 2 parts
TABLES = {"shapenetpart": SHAPENET, "made_up": MADE_UP}
KINDS = ("random", "quantised", "special", "absent")
BIG = 1 << 40


def _tables(name):
    from si_mamba_amd import SHAPENETPART, PartTable
    dev = SHAPENETPART if name == "shapenetpart" else PartTable.from_label_lists(MADE_UP)
    return pr.Table(TABLES[name]), dev


def make_batch(table, B, N, kind, seed):
    """scores (B, N, C) float32 and target (B, N) int64 on the host, with the category of every shape.  Every shape's
    targets use a subset of its category's parts; 6 % of them lie outside the category and 3 % outside [0, C), never at
    point 0 (from which the category may be derived)."""
    rng = np.random.default_rng(seed)
    C, ncat = table.num_labels, len(table.names)
    category = (rng.integers(0, ncat, B) + np.arange(B)) % ncat if B > 1 else np.array([seed % ncat])
    target = np.empty((B, N), dtype=np.int64)
    if kind == "quantised":
        scores = np.round(rng.uniform(-1, 1, (B, N, C)) * 4) / 4               # ties in most rows
    else:
        scores = rng.standard_normal((B, N, C))
    scores = scores.astype(np.float32)
    for b in range(B):
        f, c = int(table.first[category[b]]), int(table.count[category[b]])
        keep = np.flatnonzero(rng.random(c) < 0.6)
        keep = keep if keep.size else np.array([rng.integers(0, c)])
        target[b] = f + keep[rng.integers(0, keep.size, N)]
        if kind == "absent":                                                    # the parts the target misses are
            gone = np.setdiff1d(np.arange(c), keep)                             # (nearly) never predicted either
            scores[b][:, f + gone] -= 1000.0 if b % 2 == 0 else 3.0
        u = rng.random(N)
        out = np.flatnonzero(u < 0.06)
        target[b, out] = rng.integers(0, C, out.size)
        far = np.flatnonzero(u > 0.97)
        target[b, far] = rng.choice([-1, -3, C, C + 7, 255, 256, BIG, -BIG], far.size)
        target[b, 0] = f + keep[0]
        if kind == "special":
            rows = rng.permutation(N)
            for j, i in enumerate(rows[:min(N, 12)]):
                scores[b, i] = (1.5, np.nan, -np.inf, np.inf)[j % 4]            # all-equal / all-NaN / all-inf rows
            m = rng.random((N, C))
            part = scores[b]
            keep_rows = np.ones(N, dtype=bool)
            keep_rows[rows[:min(N, 12)]] = False
            part[(m < 0.04) & keep_rows[:, None]] = np.nan                      # scattered NaN and +-inf
            part[(m > 0.92) & (m < 0.96) & keep_rows[:, None]] = np.inf
            part[(m > 0.96) & keep_rows[:, None]] = -np.inf
    return scores, target, category


def make_lengths(B, N):
    return np.array([(1, N - 1, N, N + 5)[b % 4] for b in range(B)], dtype=np.int64)


def pad(scores, target, lengths):
    """The padding holds what must never be read: NaN scores and labels that would index out of range."""
    scores, target = scores.copy(), target.copy()
    for b, n in enumerate(np.clip(lengths, 1, scores.shape[1])):
        scores[b, n:] = np.nan
        target[b, n:] = BIG if b % 2 else -7
    return scores, target


def to_device(scores, dtype, device):
    """The device's scores, and the same values on the host in float64 (what the restatement ranks)."""
    t = torch.from_numpy(scores).to(dtype)
    return t.to(device), t.double().numpy()


def assert_batch_equal(got, want):
    assert np.array_equal(got.pred.cpu().numpy(), want["pred"])
    for k in ("inter", "uni", "correct", "seen_class", "correct_class"):
        assert np.array_equal(getattr(got, k).cpu().numpy(), want[k]), k
    assert getattr(got, "inter").dtype == torch.int32 and got.seen_class.dtype == torch.int64
    assert got.shape_iou.dtype == torch.float64
    assert np.array_equal(got.shape_iou.cpu().numpy().view(np.int64), want["shape_iou"].view(np.int64))
    assert np.array_equal(got.category.cpu().numpy(), want["category"])


def same_float(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def assert_result_close(got, ref_pass):
    want, n = ref_pass.result(), ref_pass.num_shapes()
    assert got["accuracy"] == want["accuracy"]
    assert same_float(got["class_avg_accuracy"], want["class_avg_accuracy"])
    tol = n * 2.0 ** -52
    for k in ("class_avg_iou", "inctance_avg_iou"):
        print(k, got[k], want[k], abs(got[k] - want[k]), tol * abs(want[k]))
        assert abs(got[k] - want[k]) <= tol * abs(want[k]), k
    assert set(got["category_iou"]) == set(want["category_iou"])
    for name, w in want["category_iou"].items():
        g = got["category_iou"][name]
        assert (np.isnan(g) and np.isnan(w)) or abs(g - w) <= tol * abs(w), name


def assert_state_equal(a, b):
    sa, sb = a.state(), b.state()
    assert set(sa) == set(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype
        assert torch.equal(sa[k].view(torch.int64), sb[k].view(torch.int64)), k      # float64 sums bit for bit


@pytest.mark.parametrize("table_name", list(TABLES))
@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 2048])
def test_batch_equals_restatement(N, B, table_name, device):
    """Every content, element type, category source and lengths form at one (N, B, table): the lane (63 / 64 / 65),
    workgroup (255 / 256 / 257) and many-trips (2048) seams of the point loop, one and several workgroups."""
    from si_mamba_amd import PartSegMetrics, part_seg_eval
    ref_table, dev_table = _tables(table_name)
    lengths = make_lengths(B, N)
    for kind in KINDS:
        scores, target, category = make_batch(ref_table, B, N, kind, seed=1000 * N + 10 * B + KINDS.index(kind))
        padded = pad(scores, target, lengths)
        for dtype in (torch.float32, torch.bfloat16):
            for s, t, lens in ((scores, target, None), (*padded, lengths)):
                dev_scores, host_scores = to_device(s, dtype, device)
                dev_target = torch.from_numpy(t).to(device)
                dev_lens = None if lens is None else torch.from_numpy(lens).to(device)
                for cat in (None, category):
                    want = pr.evaluate_batch(ref_table, host_scores, t, cat, lens)
                    dev_cat = None if cat is None else torch.from_numpy(cat).to(device)
                    got = part_seg_eval(dev_scores, dev_target, dev_cat, table=dev_table, lengths=dev_lens)
                    assert_batch_equal(got, want)
                    if lens is not None:
                        assert (want["pred"] == -1).sum() == (N - np.clip(lens, 1, N)).sum()
                # the accumulator on the same batch, once per content / type / lengths form
                acc = PartSegMetrics(dev_table).update(dev_scores, dev_target, lengths=dev_lens)
                ref = pr.Pass(ref_table)
                ref.add(host_scores, t, None, lens)
                assert_result_close(acc.compute(), ref)


def test_return_pred_false_and_accumulation_into_the_class_counts(device):
    from si_mamba_amd import part_seg_eval
    from si_mamba_amd.seg_metrics import _launch
    ref_table, dev_table = _tables("shapenetpart")
    scores, target, category = make_batch(ref_table, 3, 300, "quantised", 5)
    ds, dt = torch.from_numpy(scores).to(device), torch.from_numpy(target).to(device)
    a = part_seg_eval(ds, dt, return_pred=False)
    b = part_seg_eval(ds, dt)
    assert a.pred is None and torch.equal(a.inter, b.inter) and torch.equal(a.shape_iou, b.shape_iou)
    seen = torch.full((50,), 7, device=device, dtype=torch.int64)
    corr = torch.full((50,), -2, device=device, dtype=torch.int64)
    _launch(ds, dt, None, dev_table, None, False, seen, corr)
    assert torch.equal(seen, b.seen_class + 7) and torch.equal(corr, b.correct_class - 2)


def _pass_batches(ref_table, shapes, seed):
    out = []
    for j, (B, N) in enumerate(shapes):
        scores, target, category = make_batch(ref_table, B, N, KINDS[j % len(KINDS)], seed + j)
        lens = make_lengths(B, N) if j % 2 else None
        if lens is not None:
            scores, target = pad(scores, target, lens)
        out.append((scores, target, category if j % 3 == 0 else None, lens))
    return out


def _feed(acc, batches, device, dtype=torch.float32):
    for scores, target, category, lens in batches:
        acc.update(to_device(scores, dtype, device)[0], torch.from_numpy(target).to(device),
                   None if category is None else torch.from_numpy(category).to(device),
                   None if lens is None else torch.from_numpy(lens).to(device))
    return acc


def test_three_updates_equal_the_restatement_of_the_concatenation(device):
    from si_mamba_amd import PartSegMetrics
    ref_table, dev_table = _tables("shapenetpart")
    batches = _pass_batches(ref_table, [(17, 65), (3, 257), (5, 64)], 40)
    acc = _feed(PartSegMetrics(dev_table), batches, device)
    ref = pr.Pass(ref_table)
    for scores, target, category, lens in batches:
        ref.add(scores.astype(np.float64), target, category, lens)
    s = acc.state()
    assert np.array_equal(s["seen_class"].cpu().numpy(), ref.seen_class)
    assert np.array_equal(s["correct_class"].cpu().numpy(), ref.correct_class)
    assert int(s["correct"]) == ref.total_correct and int(s["seen"]) == ref.total_seen
    assert s["shape_count"].tolist() == [len(ref.shape_ious[n]) for n in ref_table.names]
    assert ref.num_shapes() == 25
    assert_result_close(acc.compute(), ref)


def test_merge_reset_and_reproducibility(device):
    from si_mamba_amd import PartSegMetrics
    ref_table, dev_table = _tables("shapenetpart")
    batches = _pass_batches(ref_table, [(17, 257), (3, 2048), (5, 63), (4, 256)], 70)
    # halves, one update each: the merged float64 sums are the same two additions in the other order -- bit for bit
    whole = _feed(PartSegMetrics(dev_table), batches[:2], device)
    first, second = (_feed(PartSegMetrics(dev_table), [b], device) for b in batches[:2])
    assert_state_equal(first.merge_(second), whole)
    assert_state_equal(PartSegMetrics(dev_table).merge_(whole), whole)               # into an empty accumulator
    # halves of two updates each: the integers are equal, the IoU sums are float64 sums in another order
    whole = _feed(PartSegMetrics(dev_table), batches, device)
    merged = _feed(PartSegMetrics(dev_table), batches[:2], device).merge_(
        _feed(PartSegMetrics(dev_table), batches[2:], device))
    for k in ("shape_count", "correct", "seen", "seen_class", "correct_class"):
        assert torch.equal(merged.state()[k], whole.state()[k]), k
    n = int(whole.state()["shape_count"].sum())
    assert n == 29
    a, b = merged.state()["iou_sum"], whole.state()["iou_sum"]
    assert bool(((a - b).abs() <= n * 2.0 ** -52 * b.abs()).all())
    # the same pass again: the same bits
    again = _feed(PartSegMetrics(dev_table), batches, device)
    assert_state_equal(again, whole)
    # reset: the state of a new accumulator, and the pass after it gives the same bits once more
    again.reset()
    assert_state_equal(again, PartSegMetrics(dev_table, device=device))
    assert all(not bool(t.any()) for t in again.state().values())
    assert_state_equal(_feed(again, batches, device), whole)


def test_update_is_captured_in_a_graph(device):
    """A host read or a synchronisation inside update() fails the capture: that failure is the check.  The graph is
    replayed on two batches copied into the captured buffers and leaves the state the eager calls leave."""
    from si_mamba_amd import PartSegMetrics
    ref_table, dev_table = _tables("shapenetpart")
    B, N = 5, 300
    batches = [make_batch(ref_table, B, N, kind, 90 + j) for j, kind in enumerate(("random", "quantised"))]
    lens = torch.from_numpy(make_lengths(B, N)).to(device)
    acc = PartSegMetrics(dev_table, device=device)        # the state and the table are on the device before the capture
    scores = torch.zeros(B, N, 50, device=device)
    target = torch.zeros(B, N, device=device, dtype=torch.int64)
    acc.update(scores, target, lengths=lens)              # every kernel of the op has run once; then from zero again
    acc.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        acc.update(scores, target, lengths=lens)
    acc.reset()
    eager = PartSegMetrics(dev_table, device=device)
    for s, t, _ in batches:
        scores.copy_(torch.from_numpy(s))
        target.copy_(torch.from_numpy(t))
        graph.replay()
        eager.update(scores.clone(), target.clone(), lengths=lens)
    torch.cuda.synchronize()
    assert int(acc.state()["shape_count"].sum()) == 2 * B
    assert_state_equal(acc, eager)
    ref = pr.Pass(ref_table)
    for s, t, _ in batches:
        ref.add(s.astype(np.float64), t, None, lens.cpu().numpy())
    assert_result_close(acc.compute(), ref)


def test_scores_of_the_model(device):
    """The tiny PartSegMamba of tests/test_gpu_seg.py in eval(): one forward, its log-probabilities into update()."""
    from si_mamba_amd import PartSegMetrics
    from si_mamba_amd.seg import PartSegMamba, default_seg_config
    ref_table, dev_table = _tables("shapenetpart")
    torch.manual_seed(0)
    cfg = default_seg_config(trans_dim=64, depth=4, fetch_idx=(1, 2, 3), num_group=32, group_size=16, drop_path=0.,
                             drop_path_rate=0., knn_graph=6, method="HLT", k_top_eigenvectors=3)
    m = PartSegMamba(50, cfg).to(device).eval()
    B, N = 2, 512
    g = torch.Generator().manual_seed(3)
    pts = torch.randn(B, N, 3, generator=g)
    pts = pts - pts.mean(1, keepdim=True)
    pts = (pts / pts.norm(dim=-1).max(dim=1)[0][:, None, None]).transpose(1, 2).contiguous()
    category = torch.tensor([3, 10])
    label = torch.nn.functional.one_hot(category, 16).float()
    first, count = ref_table.first[category.numpy()], ref_table.count[category.numpy()]
    target = torch.stack([torch.randint(int(f), int(f + c), (N,), generator=g) for f, c in zip(first, count)])
    with torch.no_grad():
        out = m(pts.to(device), label.to(device))
    assert out.shape == (B, N, 50)
    acc = PartSegMetrics().update(out, target.to(device), category.to(device))
    ref = pr.Pass(ref_table)
    r = ref.add(out.double().cpu().numpy(), target.numpy(), category.numpy())
    s = acc.state()
    assert int(s["correct"]) == int(r["correct"].sum()) and int(s["seen"]) == B * N
    assert np.array_equal(s["seen_class"].cpu().numpy(), r["seen_class"])
    assert np.array_equal(s["correct_class"].cpu().numpy(), r["correct_class"])
    assert_result_close(acc.compute(), ref)
