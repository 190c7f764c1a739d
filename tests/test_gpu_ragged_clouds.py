"""GPU: ragged point-cloud batches -- per-cloud ``lengths`` in farthest-point sampling, the k-NN grouping, ``Group`` /
``PointMamba`` and the pytorch3d stand-ins.

The yardstick is the project's own fixed-length kernels (held to the oracle by tests/test_gpu_encoder.py and
tests/test_gpu_dense_clouds.py): every cloud of a padded batch is also run alone at its true length, and the ragged
call has to return exactly that, bit for bit."""
import pytest
import torch

from helpers import clouds

pytestmark = pytest.mark.gpu

# (N the batch is padded to, patches G): the 256-lane FPS kernel at 1024 and 4096 points, the 1024-lane one at 8192
SHAPES = [(1024, 128), (4096, 512), (8192, 512)]
M = 32          # group_size


def spread_lengths(lo, hi, B=8):
    """B lengths from lo to hi inclusive (both ends are hit), the ones in between off every power of two."""
    ln = torch.linspace(lo, hi, B).round().long()
    ln[1:-1] += torch.arange(1, B - 1) % 3 - 1
    assert ln[0] == lo and ln[-1] == hi and ln.min() >= lo and ln.max() <= hi
    return ln


def padded(N, ln, seed, fill=0.0):
    """(B, N, 3): every cloud centred and scaled on its real points only, ``fill`` behind them."""
    pts = torch.full((len(ln), N, 3), fill)
    for b, n in enumerate(ln.tolist()):
        pts[b, :n] = clouds(1, n, seed + b)[0] if n > 1 else torch.tensor([0.25, -0.5, 0.125])
    return pts


def fps(points, K, **kw):
    from si_mamba_amd import grouping
    return grouping.sample_farthest_points(points, K, **kw)


def knn(centers, points, K, **kw):
    from si_mamba_amd import grouping
    return grouping.knn_group(centers, points, K, **kw)


@pytest.mark.parametrize("N,G", SHAPES)
def test_fps_and_knn_equal_every_cloud_alone(N, G, device):
    ln = spread_lengths(G, N)
    pts = padded(N, ln, seed=N).to(device)
    lnd = ln.to(device)
    centers, idx = fps(pts, G, lengths=lnd)
    nn_idx = knn(centers, pts, M, lengths=lnd)
    assert idx.shape == (8, G) and centers.shape == (8, G, 3) and nn_idx.shape == (8, G, M)
    for b, n in enumerate(ln.tolist()):
        wc, wi = fps(pts[b:b + 1, :n], G)
        assert torch.equal(idx[b], wi[0]), (b, n)
        assert torch.equal(centers[b], wc[0]), (b, n)
        want = knn(wc, pts[b:b + 1, :n], M)
        assert torch.equal(nn_idx[b], want[0]), (b, n)
        assert int(idx[b].min()) >= 0 and int(idx[b].max()) < n and int(nn_idx[b].max()) < n
        assert len(set(idx[b].tolist())) == G


@pytest.mark.parametrize("lengths_dtype", [torch.int32, torch.int16])
def test_lengths_of_any_integer_dtype(lengths_dtype, device):
    ln = spread_lengths(128, 1024)
    pts = padded(1024, ln, seed=5).to(device)
    c0, i0 = fps(pts, 128, lengths=ln.to(device))
    c1, i1 = fps(pts, 128, lengths=ln.to(device, lengths_dtype))
    assert torch.equal(i0, i1) and torch.equal(c0, c1)
    assert torch.equal(knn(c0, pts, M, lengths=ln.to(device)), knn(c0, pts, M, lengths=ln.to(device, lengths_dtype)))


@pytest.mark.parametrize("N,G", SHAPES)
def test_padding_is_never_read_into_a_result(N, G, device):
    ln = spread_lengths(G, N)
    lnd = ln.to(device)
    base = padded(N, ln, seed=N + 1).to(device)
    c0, i0 = fps(base, G, lengths=lnd)
    k0 = knn(c0, base, M, lengths=lnd)
    st = (ln // 3).to(device)
    cs0, is0 = fps(base, G, lengths=lnd, start_idx=st)
    for fill in (float("nan"), float("inf"), 1e30):
        pts = padded(N, ln, seed=N + 1, fill=fill).to(device)
        c, i = fps(pts, G, lengths=lnd)
        assert torch.equal(i, i0) and torch.equal(c, c0), fill
        assert torch.isfinite(c).all()
        assert torch.equal(knn(c0, pts, M, lengths=lnd), k0), fill
        cs, is_ = fps(pts, G, lengths=lnd, start_idx=st)
        assert torch.equal(is_, is0) and torch.equal(cs, cs0), fill
    assert (i0 < lnd[:, None]).all() and (i0 >= 0).all()
    assert (k0 < lnd[:, None, None]).all() and (k0 >= 0).all()


@pytest.mark.parametrize("N,K", [(1024, 128), (8192, 512)])
def test_fps_short_clouds_are_padded(N, K, device):
    ln = torch.tensor([1, 5, 64, K - 1, K, K + 1, N - 1, N])
    pts = padded(N, ln, seed=7, fill=float("nan")).to(device)
    centers, idx = fps(pts, K, lengths=ln.to(device))
    for b, n in enumerate(ln.tolist()):
        k = min(K, n)
        wc, wi = fps(pts[b:b + 1, :n], k)
        assert torch.equal(idx[b, :k], wi[0]) and torch.equal(centers[b, :k], wc[0]), (b, n)
        assert (idx[b, k:] == -1).all() and (centers[b, k:] == 0).all(), (b, n)
        if n <= K:
            assert sorted(idx[b, :k].tolist()) == list(range(n))       # every point of a short cloud is picked once


@pytest.mark.parametrize("N", [1024, 8192])
def test_knn_short_clouds_and_centre_lengths(N, device):
    G = 128
    ln = torch.tensor([1, 7, M - 1, M, M + 1, 100, N - 1, N])
    lc = torch.tensor([G, 0, 1, 5, G - 1, G, 64, G + 7])
    pts = padded(N, ln, seed=11, fill=float("nan")).to(device)
    cen = clouds(8, G, seed=12).to(device)
    got = knn(cen, pts, M, lengths=ln.to(device))
    for b, n in enumerate(ln.tolist()):
        k = min(M, n)
        want = knn(cen[b:b + 1], pts[b:b + 1, :n], k)
        assert torch.equal(got[b, :, :k], want[0]), (b, n)              # same order, not just the same set
        assert (got[b, :, k:] == 0).all(), (b, n)
    both = knn(cen, pts, M, lengths=ln.to(device), center_lengths=lc.to(device))
    only = knn(cen, padded(N, torch.full((8,), N), seed=13).to(device), M, center_lengths=lc.to(device))
    full = knn(cen, padded(N, torch.full((8,), N), seed=13).to(device), M)
    for b, g in enumerate(lc.clamp(max=G).tolist()):
        assert torch.equal(both[b, :g], got[b, :g]) and (both[b, g:] == 0).all(), (b, g)
        assert torch.equal(only[b, :g], full[b, :g]) and (only[b, g:] == 0).all(), (b, g)


@pytest.mark.parametrize("N,K", [(1024, 128), (8192, 512)])
def test_fps_start_idx(N, K, device):
    ln = spread_lengths(K, N)
    g = torch.Generator().manual_seed(3)
    st = (torch.rand(8, generator=g) * ln).floor().long().clamp(max=ln - 1)
    st[0], st[-1] = 0, N - 1                                            # both ends of the range
    pts = padded(N, ln, seed=21).to(device)
    centers, idx = fps(pts, K, lengths=ln.to(device), start_idx=st.to(device))
    assert torch.equal(idx[:, 0].cpu(), st)
    for b, (n, s) in enumerate(zip(ln.tolist(), st.tolist())):
        wc, wi = fps(torch.roll(pts[b:b + 1, :n], -s, dims=1), K)
        assert torch.equal(idx[b], (wi[0] + s) % n), (b, n, s)
        assert torch.equal(centers[b], wc[0]), (b, n, s)
    # start_idx alone: full-length clouds
    full = padded(N, torch.full((8,), N), seed=22).to(device)
    centers, idx = fps(full, K, start_idx=st.to(device))
    for b, s in enumerate(st.tolist()):
        wc, wi = fps(torch.roll(full[b:b + 1], -s, dims=1), K)
        assert torch.equal(idx[b], (wi[0] + s) % N) and torch.equal(centers[b], wc[0]), (b, s)


@pytest.mark.parametrize("N,G", SHAPES)
def test_without_lengths_nothing_changes(N, G, device):
    """lengths=None, start_idx=None is the existing call: the same entry point of the library, the oracle's picks."""
    from oracle import fps_ref
    from si_mamba_amd import _lib
    pts = clouds(2, N, seed=N + 2)
    d = pts.to(device)
    centers, idx = fps(d, G)
    c2, i2 = fps(d, G, lengths=None, start_idx=None)
    assert torch.equal(idx, i2) and torch.equal(centers, c2)
    wc, wi = fps_ref.sample_farthest_points(pts, G)
    assert torch.equal(idx.cpu(), wi) and torch.equal(centers.cpu(), wc)
    lib = _lib.load()
    i3, c3 = torch.empty_like(idx), torch.empty_like(centers)
    _lib.check(lib.simamba_farthest_point_sample(d.data_ptr(), i3.data_ptr(), c3.data_ptr(), 2, N, G,
                                                 _lib.stream_ptr(device)), "fps")
    assert torch.equal(i3, idx) and torch.equal(c3, centers)
    nn_idx = knn(centers, d, M)
    assert torch.equal(nn_idx, knn(centers, d, M, lengths=None, center_lengths=None))
    k3 = torch.empty_like(nn_idx)
    _lib.check(lib.simamba_knn_group(d.data_ptr(), centers.data_ptr(), k3.data_ptr(), 2, N, G, M,
                                     _lib.stream_ptr(device)), "knn_group")
    assert torch.equal(k3, nn_idx)
    # full lengths through the ragged kernels: the same again
    full = torch.full((2,), N, device=device)
    c4, i4 = fps(d, G, lengths=full)
    assert torch.equal(i4, idx) and torch.equal(c4, centers)
    assert torch.equal(knn(centers, d, M, lengths=full, center_lengths=torch.full((2,), G, device=device)), nn_idx)


def _model(device):
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    return PointMamba(default_config(drop_path=0.)).to(device)


MODEL_LENGTHS = [1024, 700, 513, 128]


def test_pointmamba_on_a_padded_batch_equals_every_cloud_alone(device):
    """neighborhood and center bit for bit; logits within the fp32 bar of DESIGN.md section 2 (the GEMMs see another
    batch shape)."""
    m = _model(device).eval()
    ln = torch.tensor(MODEL_LENGTHS)
    pts = padded(1024, ln, seed=31, fill=float("nan")).to(device)
    lnd = ln.to(device)
    with torch.no_grad():
        nb, center, nb_org = m.group_divider(pts, lengths=lnd)
        got = m(pts, lengths=lnd)
        assert torch.isfinite(nb).all() and torch.isfinite(got).all()
        worst = 0.0
        for b, n in enumerate(ln.tolist()):
            alone = pts[b:b + 1, :n].contiguous()
            wnb, wcenter, wnb_org = m.group_divider(alone)
            assert torch.equal(nb[b], wnb[0]) and torch.equal(center[b], wcenter[0]), (b, n)
            assert torch.equal(nb_org[b], wnb_org[0]), (b, n)
            want = m(alone)
            err = ((got[b:b + 1] - want).abs().max() / max(1.0, want.abs().max().item())).item()
            print(f"cloud {b}: {n} points, logits error {err:.3e}")
            worst = max(worst, err)
        assert worst <= 1e-3, worst


def test_pointmamba_train_step_with_lengths(device):
    m = _model(device).train()
    ln = torch.tensor(MODEL_LENGTHS)
    pts = padded(1024, ln, seed=32, fill=float("nan")).to(device)
    gt = torch.tensor([0, 3, 7, 14], device=device)
    loss, _ = m.get_loss_acc(m(pts, lengths=ln.to(device)), gt)
    loss.backward()
    assert torch.isfinite(loss)
    bad = [k for k, p in m.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not bad, bad


def test_lengths_precondition_and_models_without_ragged_batches(device):
    m = _model(device).eval()
    pts = padded(1024, torch.tensor([1024, 127]), seed=33).to(device)
    with pytest.raises(ValueError, match=r"127 .* 128"):
        m(pts, lengths=torch.tensor([1024, 127], device=device))
    with pytest.raises(ValueError, match=r"127 .* 128"):
        m.group_divider(pts, lengths=torch.tensor([1024, 127], device=device))
    with pytest.raises(TypeError):
        m.group_divider(pts, torch.tensor([1024, 1024], device=device))       # keyword-only
    from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
    from si_mamba_amd.seg import PartSegMamba
    ln = torch.tensor([1024, 700], device=device)
    mae = Point_MAE_Mamba(default_mae_config(trans_dim=96, encoder_dims=96, depth=2, decoder_depth=1)).to(device)
    with pytest.raises(NotImplementedError, match="lengths"):
        mae(pts, lengths=ln)
    seg = PartSegMamba(50).to(device)
    with pytest.raises(NotImplementedError, match="lengths"):
        seg(pts.transpose(1, 2).contiguous(), torch.zeros(2, 16, device=device), lengths=ln)


def test_lengths_check_is_skipped_during_a_stream_capture(device):
    """The one host read of Group (lengths.min()) would break a capture; under one it is left out and the graph
    replays the ragged kernels on whatever the static tensors then hold."""
    from si_mamba_amd.point_mamba import Group
    grp = Group(128, M)
    ln = torch.tensor(MODEL_LENGTHS)
    a, b = padded(1024, ln, seed=34).to(device), padded(1024, ln.flip(0), seed=35).to(device)
    want_a = grp(a, lengths=ln.to(device))
    want_b = grp(b, lengths=ln.flip(0).to(device))
    static_p, static_l = a.clone(), ln.to(device)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        grp(static_p, lengths=static_l)                                    # warm-up off the default stream
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = grp(static_p, lengths=static_l)
    for src, l, want in ((a, ln, want_a), (b, ln.flip(0), want_b)):
        static_p.copy_(src)
        static_l.copy_(l.to(device))
        graph.replay()
        torch.cuda.synchronize(device)
        for o, w in zip(out, want):
            assert torch.equal(o, w)


def test_pytorch3d_stand_ins_take_lengths(device):
    import sys

    from si_mamba_amd.shim import install_shim
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in ("mamba_ssm", "causal_conv1d", "pytorch3d")}
    try:
        install_shim(force=True, pytorch3d=True)
        from pytorch3d.ops import knn_points, sample_farthest_points
        G = 128
        ln = torch.tensor([1, 20, G - 1, G, 300, 700, 1023, 1024])
        pts = padded(1024, ln, seed=41, fill=float("nan")).to(device)
        lnd = ln.to(device)
        c, i = sample_farthest_points(pts, lengths=lnd, K=G)
        wc, wi = fps(pts, G, lengths=lnd)
        assert torch.equal(c, wc) and torch.equal(i, wi)
        lc = lnd.clamp(max=G)                                               # the centre rows that exist
        r = knn_points(c, pts, lengths1=lc, lengths2=lnd, K=M, return_sorted=False)
        want = knn(c, pts, M, lengths=lnd, center_lengths=lc)
        assert torch.equal(r.idx, want) and r.knn is None
        r2 = knn_points(c, pts, lengths2=lnd, K=M, return_sorted=False)
        assert torch.equal(r2.idx, knn(c, pts, M, lengths=lnd))
        assert torch.isfinite(r.dists).all() and torch.isfinite(r2.dists).all()
        for b, n in enumerate(ln.tolist()):
            k, g = min(M, n), min(G, n)
            nbr = pts[b, r.idx[b, :g, :k]]                                  # (g, k, 3)
            # a three-term fp32 sum, possibly in another order: a few ulp
            torch.testing.assert_close(r.dists[b, :g, :k], ((nbr - c[b, :g, None]) ** 2).sum(-1), rtol=1e-6, atol=1e-7)
            assert (r.dists[b, :, k:] == 0).all() and (r.dists[b, g:] == 0).all(), (b, n)
            assert (r2.dists[b, :, k:] == 0).all(), (b, n)
        # random_start_point: a start inside every cloud, drawn by torch's generator on the device
        torch.manual_seed(5)
        c1, i1 = sample_farthest_points(pts, lengths=lnd, K=G, random_start_point=True)
        torch.manual_seed(5)
        c2, i2 = sample_farthest_points(pts, lengths=lnd, K=G, random_start_point=True)
        assert torch.equal(i1, i2) and torch.equal(c1, c2)
        assert (i1[:, 0] >= 0).all() and (i1[:, 0] < lnd).all()
        wc, wi = fps(pts, G, lengths=lnd, start_idx=i1[:, 0])
        assert torch.equal(i1, wi) and torch.equal(c1, wc)
        _, i3 = sample_farthest_points(pts[-1:], K=G, random_start_point=True)
        assert 0 <= int(i3[0, 0]) < 1024 and len(set(i3[0].tolist())) == G
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] in ("mamba_ssm", "causal_conv1d", "pytorch3d")]:
            del sys.modules[k]
        sys.modules.update(saved)
