"""CPU checks of tests/lattice_clouds.py: the lattice inputs are exact in fp32, its float64 references agree with the
oracle's restatements (oracle/fps_ref.py, oracle/seg_ref.py, oracle/mae_ref.py) on them, and every case that
test_gpu_lattice_selection.py runs really contains the ties it is there for.  No kernel is involved: the tie counts come
from the inputs alone, in float64.

Two of the tie conditions cannot hold for every case and are stated for the cases where they can: a k-NN row whose cloud
has no more than K points has no K boundary (there the ties inside the row are counted, and one point has none at all),
and a Chamfer direction with a single candidate (n = 1 or m = 1) has no arg-min to tie."""
import numpy as np
import pytest
import torch

import lattice_clouds as lc
from oracle import fps_ref, mae_ref, seg_ref


# ---- the builders are exact --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [2, 4, 8, 12])
def test_lattice_distances_are_exact_in_fp32(R):
    pts = lc.lattice(2, 700, R, R)
    centres = lc.subset(pts, 96, R + 1)
    assert float(pts.abs().max()) == R / 8 and torch.equal(pts * 8, (pts * 8).round())
    want = lc.direct_distance(pts.double(), centres.double())
    assert torch.equal(lc.direct_distance(pts, centres).double(), want)
    expanded = seg_ref.square_distance(pts, centres)                 # -2 p.c + |p|^2 + |c|^2, fp32
    assert expanded.dtype == torch.float32 and torch.equal(expanded.double(), want)
    assert float(expanded.min()) == 0.0 and bool((expanded.min(1)[0] == 0).all())     # every centre is a point


def test_directed_builders_hold_one_tie():
    p = lc.fps_pair(1024, 300, 44)
    d = lc.direct_distance(p.double(), p[:, :1].double())[0, :, 0]
    assert d.nonzero().flatten().tolist() == [44, 300] and float(d[44]) == float(d[300]) == 1.0
    assert lc.fps_ref(p, 5)[1].tolist() == [[0, 44, 300, 0, 0]]
    where = [9, 700, 10, 73, 41]
    c, q = lc.knn_shell(1024, where)
    d = lc.direct_distance(c.double(), q.double())[0, 0]
    assert len(set(map(tuple, q[0, where].tolist()))) == len(where)              # distinct points ...
    assert d[where].unique().numel() == 1                                          # ... at one distance
    assert float(d[where][0]) == 14 / 64 and float(np.delete(d.numpy(), where).min()) > 1000
    assert lc.knn_ref(c, q, 4).tolist() == [[[9, 10, 41, 73]]]


# ---- the references agree with the oracle's --------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,R", [(100, 17, 4), (257, 32, 4), (300, 300, 2), (1024, 128, 6)])
def test_fps_ref_agrees_with_oracle(N, K, R):
    pts = lc.fps_case(N, K, R)
    centers, idx = lc.fps_ref(pts, K)
    for dtype in (torch.float32, torch.float64):
        oc, oi = fps_ref.sample_farthest_points(pts.to(dtype), K)
        assert torch.equal(oi, idx) and torch.equal(oc.float(), centers)
    if N == K:                                                       # every site taken: index 0 again, from there on
        sites = len({tuple(r) for r in pts[0].tolist()})
        assert sites < K and bool((idx[0, sites:] == 0).all()) and idx[0, :sites].unique().numel() == sites


@pytest.mark.parametrize("last", [False, True])
def test_fps_ref_lengths_and_start(last):
    K = 32
    pts, lengths, start = lc.fps_ragged_case(1024, K, 4, last)
    centers, idx = lc.fps_ref(pts, K, lengths, start)
    for b, n in enumerate(lengths.tolist()):
        k, s = min(K, n), int(start[b])
        assert bool((idx[b, k:] == -1).all()) and bool((centers[b, k:] == 0).all())
        assert torch.equal(centers[b, :k], pts[b, idx[b, :k]]) and int(idx[b, :k].max()) < n
        # the oracle starts at point 0: hand it the cloud alone with a copy of the start point in front.  The order of
        # the real points, and with it every tie among them, is unchanged; the copy itself is only ever picked again
        # once every site is taken, which these clouds (k distinct picks) do not reach.
        assert len({tuple(r) for r in centers[b, :k].tolist()}) == k
        alone = torch.cat([pts[b:b + 1, s:s + 1], pts[b:b + 1, :n]], 1)
        oi = fps_ref.sample_farthest_points(alone, k)[1][0] - 1
        oi[0] = s
        assert torch.equal(oi, idx[b, :k])


def test_knn_ref_is_the_lexicographic_order():
    centres, pts = lc.knn_case(100, 17, 9, 3)
    lengths = torch.tensor([100, 5])
    got = lc.knn_ref(centres, pts, 9, lengths)
    for b, n in enumerate(lengths.tolist()):
        d = lc.direct_distance(centres[b:b + 1].double(), pts[b:b + 1, :n].double())[0].numpy()
        for g in range(17):
            order = np.lexsort((np.arange(n), d[g]))[:9]             # by distance, then by index
            assert got[b, g, :len(order)].tolist() == order.tolist() and bool((got[b, g, len(order):] == 0).all())


@pytest.mark.parametrize("B,N,S,R", lc.NN_CASES)
def test_three_nn_ref_agrees_with_oracle(B, N, S, R):
    xyz1, xyz2 = lc.nn_case(B, N, S, R)
    idx, w = lc.three_nn_ref(xyz1, xyz2)
    assert abs(float(w.sum(-1).min()) - 1) < 1e-12 and float(w.min()) >= 0
    if S < 3:
        assert bool((idx[..., S:] == idx[..., S - 1:S]).all()) and float(w[..., S:].max()) < 1e-30
        return
    feats = torch.randn(B, S, 8, generator=torch.Generator().manual_seed(S))
    out, oidx, ow = seg_ref.three_nn_interpolate(xyz1, xyz2, feats)              # fp32, stable sort
    assert torch.equal(oidx, idx)
    assert float((ow.double() - w).abs().max()) < 1e-6
    want, mag = lc.interpolate_ref(feats, idx, w)
    assert float((out.double() - want).abs().max()) < 1e-5 * float(mag.max())


def test_interpolate_grad_ref_agrees_with_autograd():
    xyz1, xyz2, feats, dout = lc.interp_case(2, 130, 2, 3, 8, torch.float32)
    idx, w = lc.three_nn_ref(xyz1, xyz2)
    f = feats.double().requires_grad_(True)
    (seg_ref.index_points(f, idx) * w[..., None]).sum(2).backward(dout.double())
    grad, mag, cnt = lc.interpolate_grad_ref(dout, idx, w, 2)
    assert float((grad - f.grad).abs().max()) <= 1e-12 * float(mag.max())
    assert int(cnt.sum()) == 2 * 130 * 3 and int(cnt.max()) > 130    # a centre named more often than there are points


@pytest.mark.parametrize("n,m", lc.CHAMFER_SHAPES)
def test_chamfer_ref_agrees_with_oracle(n, m):
    pred, gt, ddist = lc.chamfer_case(n, m, 5)
    ref = lc.chamfer_ref(pred, gt, ddist)
    assert torch.equal(mae_ref.chamfer_distance(pred.double(), gt.double()), ref["dist"])
    assert torch.equal(mae_ref.chamfer_distance(pred, gt).double(), ref["dist"])   # fp32: the same numbers
    # the gradient formula, where autograd has no tie to decide: a Gaussian pair
    g = torch.Generator().manual_seed(n + m)
    p = torch.randn(3, n, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    t = torch.randn(3, m, 3, generator=g, dtype=torch.float64)
    w = torch.tensor([1.0, -2.0, 3.0], dtype=torch.float64)
    mae_ref.chamfer_distance(p, t).backward(w)
    assert float((lc.chamfer_ref(p.detach(), t, w)["dpred"] - p.grad).abs().max()) < 1e-12


def test_chamfer_duplicates_belong_to_the_lower_copy():
    pred, gt, _ = lc.chamfer_case(8, 16, 5)
    ref = lc.chamfer_ref(pred, gt)
    assert torch.equal(pred[0, 7], pred[0, 0]) and torch.equal(gt[0, 15], gt[0, 0]) and torch.equal(pred[0, 0], gt[0, 0])
    assert int(ref["idx1"][0, 0]) == 0 and int(ref["idx1"][0, 7]) == 0           # never target 15
    assert int(ref["idx2"][0, 0]) == 0 and int(ref["idx2"][0, 15]) == 0          # never prediction 7
    assert not bool((ref["idx1"][0::2] == 15).any()) and not bool((ref["idx2"][0::2] == 7).any())


# ---- every GPU case contains its ties --------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,R", lc.FPS_CASES)
def test_fps_cases_are_tied(N, K, R):
    rounds, tied = lc.fps_tied(lc.fps_case(N, K, R), K)
    assert rounds == lc.FPS_BATCH * (K - 1) and 3 * tied >= rounds, (rounds, tied)


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("N,K,R", lc.FPS_RAGGED)
def test_fps_ragged_cases_are_tied(N, K, R, last):
    pts, lengths, start = lc.fps_ragged_case(N, K, R, last)
    rounds, tied = lc.fps_tied(pts, K, lengths, start)
    assert rounds == sum(min(K, n) - 1 for n in lengths.tolist()) and 3 * tied >= rounds, (rounds, tied)


@pytest.mark.parametrize("N", lc.FPS_PAIR_N)
def test_fps_pairs_are_tied(N):
    for off in lc.FPS_PAIR_OFFSETS:
        if lc.FPS_PAIR_A + off < N:
            assert lc.fps_tied(lc.fps_pair(N, lc.FPS_PAIR_A, lc.FPS_PAIR_A + off), 5) == (4, 3)   # all but the third


@pytest.mark.parametrize("N,G,K,R", lc.KNN_CASES)
def test_knn_cases_are_tied(N, G, K, R):
    centres, pts = lc.knn_case(N, G, K, R)
    rows, boundary, inside = lc.knn_tied(centres, pts, K)
    if K < N:
        assert rows == lc.KNN_BATCH * G and 2 * boundary >= rows, (rows, boundary)
    elif N > 1:                                                      # K = N: no boundary; the order inside the row
        assert 2 * inside >= lc.KNN_BATCH * G, inside
    if K > 1 and N > 1:
        assert inside == lc.KNN_BATCH * G                            # every row has ties among its first K


def test_knn_ragged_case_is_tied():
    centres, pts, K, lengths = lc.knn_ragged_case()
    rows, boundary, inside = lc.knn_tied(centres, pts, K, lengths)
    assert rows == centres.shape[1] * int((lengths > K).sum()) and 2 * boundary >= rows, (rows, boundary)


@pytest.mark.parametrize("B,N,S,R", [c for c in lc.NN_CASES if c[2] > 3])
def test_three_nn_cases_are_tied(B, N, S, R):
    rows, tied = lc.three_nn_tied(*lc.nn_case(B, N, S, R))
    assert rows == B * N and 4 * tied >= rows, (rows, tied)


def test_interp_cases_use_the_three_nn_clouds():
    assert {c[:4] for c in lc.INTERP_CASES} <= set(lc.NN_CASES)


@pytest.mark.parametrize("pairs", lc.CHAMFER_PAIRS)
@pytest.mark.parametrize("n,m", lc.CHAMFER_SHAPES)
def test_chamfer_cases_are_tied(n, m, pairs):
    pred, gt, _ = lc.chamfer_case(n, m, pairs)
    tied1, tied2 = lc.chamfer_tied(pred, gt)
    assert tied1 >= 1 or m == 1, tied1                               # a prediction with two nearest targets
    assert tied2 >= 1 or n == 1, tied2                               # a target with two nearest predictions
