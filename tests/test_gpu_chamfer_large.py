"""GPU: the whole-cloud Chamfer kernels (csrc/chamfer_large.hip) against a float64 brute force written here.

The yardstick takes the fp32 inputs cast to double, forms every squared distance from direct differences on the host,
chunked over rows, and picks the arg-min as the lowest index among exact minima.  Bounds (derived, not fitted):
  * distances, relative 2e-6: three fp32 differences, three products and two adds give each distance a relative error
    below 6 * 2^-24 = 3.6e-7, the minimum of perturbed values inherits it, the fixed-order fp64 sum adds < 1e-7;
  * indices: equal to the float64 arg-min wherever best and second best differ by more than relative 1e-5 (at most 1 %
    of the queries may be left out, asserted);
  * integer lattice {0..15}^3: every distance and every sum up to 8192 * 675 < 2^24 is exact in fp32 and the means
    divide by powers of two, so everything is compared for equality;
  * gradients, max|got - want| / max|want| <= 1e-5: each term is a difference of fp32 coordinates times an exactly
    representable factor, and the reverse-match sums have a handful of terms.  The float64 autograd of the composed
    form runs on the device (torch's float64 ops, 2.5 GB of intermediates at the largest shape), after the host brute
    force has shown that no query of the seed has a best / second-best gap below relative 1e-5.
"""
import functools
import sys

import pytest
import torch

from helpers import clouds_from, max_scaled, relerr
from si_mamba_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(3, 65, 64),        # one point over the small kernels' limit, on one side only
          (2, 1000, 1300),    # neither size a multiple of any tile
          (1, 8192, 4099),    # the cap, and an odd size
          (300, 96, 80),      # many pairs, for the grid mapping
          (2, 1, 257),        # a single-point set
          (2, 9, 1025)]       # one full tile of targets plus one point, staged by workgroups with 9 queries
# (2, 1, 257) has one query whose reverse-match gradient sums 257 displacements (cancellation); its transpose keeps the
# single-point case with at most one reverse match per query
GRAD_SHAPES = SHAPES[:4] + [(2, 257, 1), (2, 9, 1025)]
SEED = {(3, 65, 64): 1, (2, 1000, 1300): 2, (1, 8192, 4099): 3, (300, 96, 80): 4, (2, 1, 257): 5, (2, 257, 1): 6,
        (5, 32, 32): 7, (5, 64, 64): 8, (2, 65, 32): 9, (2, 9, 1025): 10}
BIG = 1 << 30


@functools.lru_cache(maxsize=None)
def random_pair(shape):
    pairs, n, m = shape
    gen = torch.Generator().manual_seed(SEED[shape])
    return clouds_from(pairs, n, gen), clouds_from(pairs, m, gen)


def nearest64(q, t, chunk=512):
    """q (P,n,3), t (P,m,3) fp32 -> float64 (best (P,n), lowest index among exact minima (P,n) int64, second best)."""
    q, t = q.double(), t.double()
    P, n, m = q.shape[0], q.shape[1], t.shape[1]
    best, idx, second = torch.empty(P, n, dtype=torch.float64), torch.empty(P, n, dtype=torch.int64), \
        torch.empty(P, n, dtype=torch.float64)
    ar = torch.arange(m)
    for p in range(P):
        for r0 in range(0, n, chunk):
            qq = q[p, r0:r0 + chunk]
            dx, dy, dz = (qq[:, None, c] - t[p, None, :, c] for c in range(3))
            d = dx * dx + dy * dy + dz * dz
            mn = d.min(-1)[0]
            am = torch.where(d == mn[:, None], ar, BIG).min(-1)[0]
            d[torch.arange(d.shape[0]), am] = float("inf")
            best[p, r0:r0 + chunk], idx[p, r0:r0 + chunk], second[p, r0:r0 + chunk] = mn, am, d.min(-1)[0]
    return best, idx, second


def reference(x, y):
    d1, i1, s1 = nearest64(x, y)
    d2, i2, s2 = nearest64(y, x)
    return dict(dist=d1.mean(1) + d2.mean(1), d1=d1, d2=d2, idx1=i1, idx2=i2, second1=s1, second2=s2)


@functools.lru_cache(maxsize=None)
def random_reference(shape):
    return reference(*random_pair(shape))


def undecided(ref, k):
    """Queries whose best and second-best float64 distances are within relative 1e-5 of each other (a single target
    has no second best: inf)."""
    best, second = ref[f"d{k}"], ref[f"second{k}"]
    return torch.isfinite(second) & ~((second - best) > 1e-5 * second)


def run_fwd(x, y, device, queries=0):
    """One simamba_chamfer_large_fwd_ex call -> every output, on the host.  ``queries``: 0 = the library's choice of
    query points per thread (what simamba_chamfer_large_fwd passes), 1 / 2 / 4 = that kernel."""
    lib = _lib.load()
    xd, yd = x.to(device).contiguous(), y.to(device).contiguous()
    pairs, n, m = x.shape[0], x.shape[1], y.shape[1]
    o = dict(dist=torch.empty(pairs, device=device), d1=torch.empty(pairs, n, device=device),
             d2=torch.empty(pairs, m, device=device),
             idx1=torch.full((pairs, n), -1, device=device, dtype=torch.int32),
             idx2=torch.full((pairs, m), -1, device=device, dtype=torch.int32))
    rc = lib.simamba_chamfer_large_fwd_ex(xd.data_ptr(), yd.data_ptr(), o["dist"].data_ptr(), o["idx1"].data_ptr(),
                                          o["idx2"].data_ptr(), o["d1"].data_ptr(), o["d2"].data_ptr(), pairs, n, m,
                                          queries, _lib.stream_ptr(device))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


@functools.lru_cache(maxsize=None)
def random_result(shape, device, queries=0):
    return run_fwd(*random_pair(shape), device, queries)


# ---- 1, 2: random clouds ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_distances_random_clouds(shape, device):
    got, want = random_result(shape, device), random_reference(shape)
    errs = {k: relerr(got[k], want[k]) for k in ("dist", "d1", "d2")}
    print(shape, errs)
    assert all(e <= 2e-6 for e in errs.values()), errs


@pytest.mark.parametrize("shape", SHAPES)
def test_indices_random_clouds(shape, device):
    got, want = random_result(shape, device), random_reference(shape)
    for k in (1, 2):
        skip = undecided(want, k)
        share = float(skip.double().mean())
        print(shape, f"idx{k}: undecided share {share:.2e}")
        assert share <= 0.01, share
        assert torch.equal(got[f"idx{k}"].long()[~skip], want[f"idx{k}"][~skip])
        assert int(got[f"idx{k}"].min()) >= 0 and int(got[f"idx{k}"].max()) < want[f"d{3 - k}"].shape[1]


# ---- 3: exact arithmetic ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(256, 1024), (1024, 8192), (8192, 256), (8192, 8192)])
def test_integer_lattice_is_exact(n, m, device):
    gen = torch.Generator().manual_seed(n + m)
    pairs = 1 if n * m > 1 << 24 else 2
    x = torch.randint(0, 16, (pairs, n, 3), generator=gen).float()
    y = torch.randint(0, 16, (pairs, m, 3), generator=gen).float()
    got, want = run_fwd(x, y, device), reference(x, y)
    for k in ("dist", "d1", "d2"):
        assert torch.equal(got[k], want[k].float()), k
    for k in ("idx1", "idx2"):
        assert torch.equal(got[k].long(), want[k]), k


# ---- 4: duplicated targets -------------------------------------------------------------------------------------------
def test_duplicated_targets_report_the_lower_index(device):
    shape = (2, 1000, 1300)
    x, y = random_pair(shape)
    m = shape[2]
    y = y.clone()
    y[:, m // 2:m // 2 + 4] = y[:, :4]
    got, want = run_fwd(x, y, device), reference(x, y)
    hit = want["idx1"] < 4                                   # the float64 nearest is a duplicated point: lower copy
    assert int(hit.sum()) > 0
    assert torch.equal(got["idx1"].long()[hit], want["idx1"][hit])
    assert not ((got["idx1"] >= m // 2) & (got["idx1"] < m // 2 + 4)).any()
    assert relerr(got["dist"], want["dist"]) <= 2e-6


# ---- 5: gradients ----------------------------------------------------------------------------------------------------
def autograd64(x, y, w, device):
    """float64 autograd of the composed form, on the device: (dist, dx, dy) on the host."""
    xd, yd = x.double().to(device).requires_grad_(), y.double().to(device).requires_grad_()
    d = ((xd[:, :, None] - yd[:, None]) ** 2).sum(-1)
    dist = d.min(2)[0].mean(1) + d.min(1)[0].mean(1)
    dx, dy = torch.autograd.grad(dist, (xd, yd), w.double().to(device))
    return dist.detach().cpu(), dx.cpu(), dy.cpu()


@functools.lru_cache(maxsize=None)
def grad_case(shape, device):
    x, y = random_pair(shape)
    ref = random_reference(shape)
    assert not undecided(ref, 1).any() and not undecided(ref, 2).any(), "seed has a near-tie: pick another"
    w = torch.rand(shape[0], generator=torch.Generator().manual_seed(100 + SEED[shape])) + 0.5
    return x, y, w, autograd64(x, y, w, device)


@pytest.mark.parametrize("which", ["x", "y", "both"])
@pytest.mark.parametrize("shape", GRAD_SHAPES)
def test_gradients(shape, which, device):
    from si_mamba_amd.mae import chamfer_distance
    x, y, w, (_, wdx, wdy) = grad_case(shape, device)
    xd = x.to(device).requires_grad_(which in ("x", "both"))
    yd = y.to(device).requires_grad_(which in ("y", "both"))
    _lib.counters.clear()
    (chamfer_distance(xd, yd) * w.to(device)).sum().backward()
    assert _lib.counters == {"chamfer_large": 1}
    for name, t, want in (("x", xd, wdx), ("y", yd, wdy)):
        if which in (name, "both"):
            e = max_scaled(t.grad, want)
            print(shape, which, f"d{name}: {e:.2e}")
            assert e <= 1e-5, (name, e)
        else:
            assert t.grad is None


@pytest.mark.parametrize("shape", [(2, 1000, 1300), (300, 96, 80)])
def test_null_gradient_pointer_skips_that_side(shape, device):
    lib = _lib.load()
    x, y = (t.to(device) for t in random_pair(shape))
    pairs, n, m = shape
    res = random_result(shape, device)
    i1, i2 = res["idx1"].to(device), res["idx2"].to(device)
    w = torch.rand(pairs, device=device) + 0.5

    def bwd(dx, dy):
        rc = lib.simamba_chamfer_large_bwd(x.data_ptr(), y.data_ptr(), w.data_ptr(), i1.data_ptr(), i2.data_ptr(),
                                           _lib.ptr(dx), _lib.ptr(dy), pairs, n, m, _lib.stream_ptr(device))
        assert rc == 0, rc
        torch.cuda.synchronize()

    dx, dy = torch.empty_like(x), torch.empty_like(y)
    bwd(dx, dy)
    ox, oy = torch.full_like(x, 7.0), torch.full_like(y, 7.0)
    bwd(ox, None)
    assert torch.equal(ox, dx) and bool((oy == 7.0).all())
    ox.fill_(7.0)
    bwd(None, oy)
    assert torch.equal(oy, dy) and bool((ox == 7.0).all())
    bwd(None, None)


# ---- every kernel instantiation --------------------------------------------------------------------------------------
# The library picks 1, 2 or 4 query points per thread from the problem size (4 and 2 only with 512 workgroups, i.e.
# hundreds of large pairs: too much for a host brute force), and the result must not depend on it.  The _ex entry
# points force each kernel on shapes whose tails cut into a thread's 2nd .. 4th query: 1000 = 3 * 256 + 232 and
# 1300 = 1024 + 256 + 20 leave queries 2-4 of some lanes and the whole of others past the end; 8192 / 4099 fill eight
# and four-and-a-bit workgroups of 4 queries per thread; (300, 96, 80) leaves every query but the first unused.
Q_SHAPES = [(2, 1000, 1300), (1, 8192, 4099), (300, 96, 80), (2, 1, 257)]


@pytest.mark.parametrize("queries", [1, 2, 4])
@pytest.mark.parametrize("shape", Q_SHAPES)
def test_every_queries_per_thread_kernel_forward(shape, queries, device):
    got, auto, want = random_result(shape, device, queries), random_result(shape, device), random_reference(shape)
    errs = {k: relerr(got[k], want[k]) for k in ("dist", "d1", "d2")}
    print(shape, queries, errs)
    assert all(e <= 2e-6 for e in errs.values()), errs
    for k in (1, 2):
        keep = ~undecided(want, k)
        assert torch.equal(got[f"idx{k}"].long()[keep], want[f"idx{k}"][keep])
    for k in got:                                            # and bit for bit what the library's own choice gives
        assert torch.equal(got[k], auto[k]), k


@pytest.mark.parametrize("queries", [2, 4])
@pytest.mark.parametrize("n,m", [(1024, 1100), (600, 2000)])
def test_every_queries_per_thread_kernel_lattice(n, m, queries, device):
    gen = torch.Generator().manual_seed(n + m)
    x = torch.randint(0, 16, (2, n, 3), generator=gen).float()
    y = torch.randint(0, 16, (2, m, 3), generator=gen).float()
    got, want = run_fwd(x, y, device, queries), reference(x, y)
    for k in ("dist", "d1", "d2"):
        assert torch.equal(got[k], want[k].float()), k
    for k in ("idx1", "idx2"):
        assert torch.equal(got[k].long(), want[k]), k


@pytest.mark.parametrize("queries", [1, 2, 4])
@pytest.mark.parametrize("shape", [(2, 1000, 1300), (1, 8192, 4099), (300, 96, 80), (2, 257, 1)])
def test_every_queries_per_thread_kernel_backward(shape, queries, device):
    lib = _lib.load()
    x, y, w, (_, wdx, wdy) = grad_case(shape, device)
    pairs, n, m = shape
    res = random_result(shape, device)
    xd, yd, wd = x.to(device), y.to(device), w.to(device)
    i1, i2 = res["idx1"].to(device), res["idx2"].to(device)
    out = {}
    for q in (queries, 0):
        dx, dy = torch.full_like(xd, float("nan")), torch.full_like(yd, float("nan"))
        rc = lib.simamba_chamfer_large_bwd_ex(xd.data_ptr(), yd.data_ptr(), wd.data_ptr(), i1.data_ptr(), i2.data_ptr(),
                                              dx.data_ptr(), dy.data_ptr(), pairs, n, m, q, _lib.stream_ptr(device))
        assert rc == 0, rc
        torch.cuda.synchronize()
        out[q] = (dx, dy)
    ex, ey = max_scaled(out[queries][0], wdx), max_scaled(out[queries][1], wdy)
    print(shape, queries, f"dx {ex:.2e} dy {ey:.2e}")
    assert ex <= 1e-5 and ey <= 1e-5
    assert torch.equal(out[queries][0], out[0][0]) and torch.equal(out[queries][1], out[0][1])


# ---- 6: reproducibility ----------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(device):
    from si_mamba_amd.mae import chamfer_distance
    x, y = random_pair((2, 1000, 1300))
    w = torch.rand(2, generator=torch.Generator().manual_seed(0)).to(device)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        runs = []
        for _ in range(2):
            xd, yd = x.to(device).requires_grad_(), y.to(device).requires_grad_()
            d = chamfer_distance(xd, yd)
            (d * w).sum().backward()
            runs.append((d.detach().clone(), xd.grad.clone(), yd.grad.clone()))
    finally:
        torch.use_deterministic_algorithms(prev)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- 7: routes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 32, 32), (5, 64, 64)])
def test_small_sets_keep_the_one_wave_kernels(shape, device):
    from si_mamba_amd.mae import chamfer_distance
    lib = _lib.load()
    pairs, n, m = shape
    x, y = (t.to(device) for t in random_pair(shape))
    _lib.counters.clear()
    got = chamfer_distance(x.clone().requires_grad_(), y)
    assert _lib.counters == {"chamfer_small": 1}
    dist = torch.empty(pairs, device=device)
    i1 = torch.empty(pairs, n, device=device, dtype=torch.uint8)
    i2 = torch.empty(pairs, m, device=device, dtype=torch.uint8)
    assert lib.simamba_chamfer_fwd(x.data_ptr(), y.data_ptr(), dist.data_ptr(), i1.data_ptr(), i2.data_ptr(), pairs, n,
                                   m, _lib.stream_ptr(device)) == 0
    assert torch.equal(got.detach(), dist)

    # the same sets with a differentiable gt: the tiled kernels, a gt gradient, the same forward to rounding
    xs, ys, w, (_, _, wdy) = grad_case(shape, device)
    yd = ys.to(device).requires_grad_()
    _lib.counters.clear()
    large = chamfer_distance(x, yd)
    assert _lib.counters == {"chamfer_large": 1}
    (large * w.to(device)).sum().backward()
    assert max_scaled(yd.grad, wdy) <= 1e-5
    assert relerr(large.detach().cpu(), got.detach().cpu().double()) <= 2e-6


def test_one_point_over_the_limit_takes_the_tiled_kernels(device):
    from si_mamba_amd.mae import chamfer_distance
    shape = (2, 65, 32)
    x, y = (t.to(device) for t in random_pair(shape))
    _lib.counters.clear()
    got = chamfer_distance(x, y)
    assert _lib.counters == {"chamfer_large": 1}
    assert relerr(got.cpu(), random_reference(shape)["dist"]) <= 2e-6


# ---- 8: the pytorch3d stand-in ---------------------------------------------------------------------------------------
def test_shim_takes_whole_clouds(device):
    from si_mamba_amd.shim import install_shim
    names = ("mamba_ssm", "causal_conv1d", "pytorch3d")
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in names}
    try:
        install_shim(force=True, pytorch3d=True)
        from pytorch3d.loss import chamfer_distance
        gen = torch.Generator().manual_seed(21)
        for n, m in ((1024, 1024), (2048, 1024)):
            a, b = clouds_from(4, n, gen), clouds_from(4, m, gen)
            want = reference(a, b)["dist"]
            ad, bd = a.to(device), b.to(device)
            loss, normals = chamfer_distance(ad, bd)
            assert normals is None and loss.dim() == 0
            assert abs(float(loss) - float(want.mean())) <= 2e-6 * float(want.mean())
            per, _ = chamfer_distance(ad, bd, batch_reduction=None)
            assert per.shape == (4,) and relerr(per.cpu(), want) <= 2e-6
            total, _ = chamfer_distance(ad, bd, batch_reduction="sum")
            assert abs(float(total) - float(want.sum())) <= 2e-6 * float(want.sum())
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] in names]:
            del sys.modules[k]
        sys.modules.update(saved)


# ---- 9: MAE ----------------------------------------------------------------------------------------------------------
def small_mae(device, **over):
    """The issue's small model; knn_graph = 6 because the default 20-neighbour graph needs more than 16 patches."""
    from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
    torch.manual_seed(0)
    cfg = default_mae_config(trans_dim=96, encoder_dims=96, depth=2, decoder_depth=1, num_group=16, knn_graph=6,
                             **over)
    return Point_MAE_Mamba(cfg).to(device)


def test_mae_trains_with_patches_of_96_points(device):
    m = small_mae(device, group_size=96).train()
    pts = clouds_from(2, 512, torch.Generator().manual_seed(31)).to(device)
    _lib.counters.clear()
    loss = m(pts)
    assert _lib.counters.get("chamfer_large") == 1 and "chamfer_small" not in _lib.counters
    loss.backward()
    assert torch.isfinite(loss)
    # decoder_pos_embed is dead in the spectral branch (tests/test_gpu_mae.py::test_mae_train_step_reference_sizes)
    bad = [k for k, p in m.named_parameters()
           if not k.startswith("decoder_pos_embed.") and (p.grad is None or not torch.isfinite(p.grad).all())]
    assert not bad, bad


def test_mae_reconstruct(device):
    from si_mamba_amd.mae import chamfer_distance
    m = small_mae(device).eval()
    B, N, G, M = 2, 512, 16, 32
    pts = clouds_from(B, N, torch.Generator().manual_seed(32)).to(device)
    with torch.no_grad():
        _, center, _ = m.group_divider(pts)
        mask = m.MAE_encoder._mask_center_rand(center, generator=torch.Generator().manual_seed(33))
        loss, parts = m(pts, mask=mask, return_parts=True)
    nm = int(0.6 * G)
    Mtok = parts["msk_src"].shape[1]                      # every masked patch once per ordering and direction
    assert Mtok == nm * m.k_top_eigenvectors * 2
    rebuilt, visible, loss_patches = m.reconstruct(pts, mask=mask)
    assert rebuilt.shape == (B, Mtok * M, 3) and visible.shape == (B, (G - nm) * M, 3)
    assert loss_patches.shape == (B, Mtok)
    assert not rebuilt.requires_grad and not loss_patches.requires_grad
    centre = torch.gather(center, 1, parts["msk_src"].unsqueeze(-1).expand(-1, -1, 3))
    want = parts["rebuild"].float().view(B, Mtok, M, 3) + centre[:, :, None]
    assert torch.equal(rebuilt, want.reshape(B, Mtok * M, 3))        # two forwards of one eval model: same bits
    assert abs(float(loss_patches.mean()) - float(loss)) <= 1e-6 * abs(float(loss))
    whole = torch.cat([visible, rebuilt], 1)
    score = chamfer_distance(whole, pts)
    assert torch.isfinite(score).all()
    assert relerr(score.cpu(), reference(whole.cpu(), pts.cpu())["dist"]) <= 2e-6
    with pytest.raises(NotImplementedError):
        m(pts, vis=True)
