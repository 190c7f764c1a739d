"""The tie rule of the selection kernels, index for index: FPS (csrc/fps.hip), k-NN grouping (csrc/knn_group.hip), 3-NN
and the interpolation it feeds (csrc/interp.hip) and the one-wave Chamfer kernels (csrc/chamfer.hip) on the lattice
clouds of tests/lattice_clouds.py, against its float64 references.

On a binary lattice every fp32 distance is exact, so equal distances are equal on the device too and the lower index
must win: every index comparison below is torch.equal on the whole tensor, nothing masked or sampled.
test_oracle_lattice_clouds.py checks, without a kernel, that each case here contains the ties it is meant to hold
(FPS: a third of the rounds; k-NN: the K boundary in half the rows; 3-NN: third == fourth in a quarter of the rows;
Chamfer: both directions).  The directed cases put one tie at a chosen pair of indices, so that each level of the
reductions -- the registers of a lane, the lanes of a wave, the waves of a workgroup -- decides it once.

Bounds of the floating-point comparisons (from the arithmetic, not from a run):
  3-NN weights     each is four fp32 roundings (d + eps, 1 / x, the sum of three, r / norm) of a quantity <= 1:
                   8 * 2^-24 = 4.8e-7 at most; asserted at 1e-6 absolute against the float64 formula with 1e-8f.
  interpolation    against the float64 sum over the kernel's own idx and w: an fma chain of m terms is off by at most
                   m * 2^-24 * sum |w v| (to first order); asserted at twice that, per element.  m = 3 forward, the number
                   of (point, slot) entries that name the centre backward.  bf16 results add one rounding to bf16,
                   bounded by 2^-8 relative."""
import pytest
import torch

import lattice_clouds as lc
from si_mamba_amd import _lib

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24


# ---- FPS -------------------------------------------------------------------------------------------------------------
def run_fps(points, K, device, lengths=None, start_idx=None):
    from si_mamba_amd.grouping import sample_farthest_points
    dev = lambda t: None if t is None else t.to(device)
    centers, idx = sample_farthest_points(points.to(device), K, lengths=dev(lengths), start_idx=dev(start_idx))
    return centers.cpu(), idx.cpu()


@pytest.mark.parametrize("N,K,R", lc.FPS_CASES)
def test_fps_lattice(N, K, R, device):
    pts = lc.fps_case(N, K, R)
    want_c, want_i = lc.fps_ref(pts, K)
    got_c, got_i = run_fps(pts, K, device)
    assert torch.equal(got_i, want_i)
    assert torch.equal(got_c, want_c)


@pytest.mark.parametrize("last", [False, True], ids=["start0", "startlast"])
@pytest.mark.parametrize("N,K,R", lc.FPS_RAGGED)
def test_fps_lattice_ragged(N, K, R, last, device):
    pts, lengths, start = lc.fps_ragged_case(N, K, R, last)
    want_c, want_i = lc.fps_ref(pts, K, lengths, start)
    got_c, got_i = run_fps(pts, K, device, lengths, start)
    assert torch.equal(got_i, want_i)
    assert torch.equal(got_c, want_c)


@pytest.mark.parametrize("N", lc.FPS_PAIR_N)
def test_fps_directed_pairs(N, device):
    a = lc.FPS_PAIR_A
    pairs = [(a, a + off) for off in lc.FPS_PAIR_OFFSETS if a + off < N]
    pairs += [(b, a) for a, b in pairs]                              # (1, 0, 0) at the higher index as well
    pts = torch.cat([lc.fps_pair(N, a, b) for a, b in pairs])
    want = torch.tensor([[0, min(p), max(p), 0, 0] for p in pairs])
    got_c, got_i = run_fps(pts, 5, device)
    assert torch.equal(got_i, want)
    assert torch.equal(got_c, torch.gather(pts, 1, want[..., None].expand(-1, -1, 3)))
    assert torch.equal(want, lc.fps_ref(pts, 5)[1])


@pytest.mark.parametrize("N", lc.FPS_PAIR_N)
def test_fps_directed_pair_across_the_length(N, device):
    """One of the two tied points lies behind lengths[b] (in another wave, or in the next register of the same lane):
    it is never picked, whichever of the two mirrored positions it holds."""
    a = lc.FPS_PAIR_A
    behind = [a + 64, a + 64, a + 256, a + 256]
    pts = torch.cat([lc.fps_pair(N, a, behind[0]), lc.fps_pair(N, behind[1], a),
                     lc.fps_pair(N, a, behind[2]), lc.fps_pair(N, behind[3], a)])
    lengths = torch.tensor(behind)                                   # cloud = the points in front of the second one
    want = torch.tensor([[0, a, 0, 0, 0]] * 4)
    got_c, got_i = run_fps(pts, 5, device, lengths)
    assert torch.equal(got_i, want)
    assert torch.equal(got_c, torch.gather(pts, 1, want[..., None].expand(-1, -1, 3)))
    assert torch.equal(want, lc.fps_ref(pts, 5, lengths)[1])


# ---- k-NN grouping ---------------------------------------------------------------------------------------------------
def run_knn(centres, pts, K, device, lengths=None):
    from si_mamba_amd.grouping import knn_group
    return knn_group(centres.to(device), pts.to(device), K,
                     lengths=None if lengths is None else lengths.to(device)).cpu()


@pytest.mark.parametrize("N,G,K,R", lc.KNN_CASES)
def test_knn_lattice(N, G, K, R, device):
    centres, pts = lc.knn_case(N, G, K, R)
    assert torch.equal(run_knn(centres, pts, K, device), lc.knn_ref(centres, pts, K))


def test_knn_lattice_ragged(device):
    centres, pts, K, lengths = lc.knn_ragged_case()
    assert torch.equal(run_knn(centres, pts, K, device, lengths), lc.knn_ref(centres, pts, K, lengths))


@pytest.mark.parametrize("N", lc.KNN_SHELL_N)
def test_knn_directed_rows(N, device):
    a = lc.KNN_SHELL_A
    for off in lc.KNN_SHELL_OFFSETS:                                 # one tie: the lower of the two is the neighbour
        for where in ([a, a + off], [a + off, a]):
            centre, pts = lc.knn_shell(N, where)
            assert run_knn(centre, pts, 1, device).tolist() == [[[a]]], where
    where = [a + off for off in reversed(lc.KNN_SHELL_OFFSETS)] + [a, N - 1, 3]
    centre, pts = lc.knn_shell(N, where)                             # all levels in one row: the K lowest, ascending
    K = len(where) - 1
    assert run_knn(centre, pts, K, device).tolist() == [[sorted(where)[:K]]]
    assert torch.equal(lc.knn_ref(centre, pts, K), torch.tensor([[sorted(where)[:K]]]))


# ---- 3-NN and interpolation ------------------------------------------------------------------------------------------
def run_three_nn(xyz1, xyz2, device):
    from si_mamba_amd.interp import three_nn                         # a plain call of simamba_three_nn, for every S >= 1
    return three_nn(xyz1.to(device), xyz2.to(device))


@pytest.mark.parametrize("B,N,S,R", lc.NN_CASES)
def test_three_nn_lattice(B, N, S, R, device):
    xyz1, xyz2 = lc.nn_case(B, N, S, R)
    want_i, want_w = lc.three_nn_ref(xyz1, xyz2)
    idx, w = run_three_nn(xyz1, xyz2, device)
    assert torch.equal(idx.cpu().long(), want_i)
    err = float((w.cpu().double() - want_w).abs().max())
    print(f"three_nn weights ({B}, {N}, {S}): max abs error {err:.3e}")
    assert err <= 1e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,N,S,R,C", lc.INTERP_CASES)
def test_interpolate_lattice(B, N, S, R, C, dtype, device):
    from si_mamba_amd.interp import three_interpolate
    xyz1, xyz2, feats, dout = lc.interp_case(B, N, S, R, C, dtype)
    idx, w = run_three_nn(xyz1, xyz2, device)
    assert torch.equal(idx.cpu().long(), lc.three_nn_ref(xyz1, xyz2)[0])
    f = feats.to(device).to(dtype).requires_grad_(True)
    out = three_interpolate(f, idx, w)
    out.backward(dout.to(device).to(dtype))
    assert out.dtype == dtype and f.grad.dtype == dtype
    round_out = 2.0 ** -8 if dtype == torch.bfloat16 else 0.0

    want, mag = lc.interpolate_ref(feats, idx.cpu(), w.cpu())
    err = (out.detach().cpu().double() - want).abs()
    bound = 2 * 3 * U32 * mag + round_out * want.abs()
    print(f"interpolate fwd ({B}, {N}, {S}, {C}) {dtype}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())

    want, mag, cnt = lc.interpolate_grad_ref(dout, idx.cpu(), w.cpu(), S)
    err = (f.grad.cpu().double() - want).abs()
    bound = 2 * cnt[..., None] * U32 * mag + round_out * want.abs()
    print(f"interpolate bwd ({B}, {N}, {S}, {C}) {dtype}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}"
          f", most entries on one centre {int(cnt.max())}")
    assert bool((err <= bound).all())
    assert bool((f.grad[cnt.to(device) == 0] == 0).all())            # a centre nobody names gets exactly 0


# ---- one-wave Chamfer ------------------------------------------------------------------------------------------------
def run_chamfer(pred, gt, ddist, device):
    lib = _lib.load()
    pairs, n, _ = pred.shape
    m = gt.shape[1]
    p, g, dd = pred.to(device), gt.to(device), ddist.to(device)
    dist = torch.empty(pairs, device=device)
    i1 = torch.empty(pairs, n, device=device, dtype=torch.uint8)
    i2 = torch.empty(pairs, m, device=device, dtype=torch.uint8)
    dp = torch.empty_like(p)
    with torch.cuda.device(device):
        stream = _lib.stream_ptr(device)
        _lib.check(lib.simamba_chamfer_fwd(p.data_ptr(), g.data_ptr(), dist.data_ptr(), i1.data_ptr(), i2.data_ptr(),
                                           pairs, n, m, stream), "simamba_chamfer_fwd")
        _lib.check(lib.simamba_chamfer_bwd(p.data_ptr(), g.data_ptr(), dd.data_ptr(), i1.data_ptr(), i2.data_ptr(),
                                           dp.data_ptr(), pairs, n, m, stream), "simamba_chamfer_bwd")
    return {"dist": dist.cpu(), "idx1": i1.cpu().long(), "idx2": i2.cpu().long(), "dpred": dp.cpu()}


@pytest.mark.parametrize("pairs", lc.CHAMFER_PAIRS)
@pytest.mark.parametrize("n,m", lc.CHAMFER_SHAPES)
def test_chamfer_lattice(n, m, pairs, device):
    pred, gt, ddist = lc.chamfer_case(n, m, pairs)
    want = lc.chamfer_ref(pred, gt, ddist)
    got = run_chamfer(pred, gt, ddist, device)
    assert torch.equal(got["idx1"], want["idx1"])
    assert torch.equal(got["idx2"], want["idx2"])
    assert torch.equal(got["dist"], want["dist"].float())
    assert torch.equal(got["dpred"], want["dpred"].float())
