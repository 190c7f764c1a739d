"""GPU: the earth mover's distance kernels (csrc/emd.hip) against an exact assignment solver (assignment_ref.py).

An auction with final epsilon eps returns a matching within n * eps of the optimum.  On the exact-tie lattice
(lattice_clouds.lattice, R = 4, scale = 8) every cost is a multiple of 1/64, so with eps below 1 / (64 n) the matching
must cost exactly the optimum; on Gaussian clouds with the default eps = 2^-14 cmax the gap must stay within
n 2^-14 cmax.  Sizes walk both instantiations (one wave per pair up to 64 points, one workgroup above), their boundary
and lane counts off the wave multiple; five pairs leave the one-wave kernel's last workgroup partial."""
import numpy as np
import pytest
import torch

import assignment_ref as ar

pytestmark = pytest.mark.gpu


def _run(x, y, device, **kw):
    from si_mamba_amd import earth_movers_distance
    dist, assign, rounds, conv = earth_movers_distance(x.to(device), y.to(device), return_assignment=True, **kw)
    torch.cuda.synchronize()
    assert dist.dtype == torch.float32 and assign.dtype == torch.int32 and rounds.dtype == torch.int32
    assert conv.dtype == torch.uint8
    return dist.cpu(), assign.cpu().numpy(), rounds.cpu().numpy(), conv.cpu().numpy()


def _costs(x, y, assign):
    for p in range(x.shape[0]):
        assert ar.is_permutation(assign[p]), p
    return np.array([ar.matched_cost(x[p].numpy(), y[p].numpy(), assign[p]) for p in range(x.shape[0])])


@pytest.mark.parametrize("n", ar.EMD_SIZES)
def test_lattice_matching_is_the_optimum(n, device):
    from si_mamba_amd.emd import default_max_rounds
    pairs = ar.emd_pairs(n)
    x, y, opt, _ = ar.solved("lattice", pairs, n, ar.emd_seed(n))
    eps = ar.lattice_eps(n)
    assert eps < 1.0 / (64 * n)
    dist, assign, rounds, conv = _run(x, y, device, eps=eps)
    print(f"n={n} lattice rounds {rounds.tolist()} of {default_max_rounds(n)}")
    assert conv.tolist() == [1] * pairs
    assert _costs(x, y, assign).tolist() == opt.tolist()
    np.testing.assert_allclose(dist.double().numpy(), opt / n, rtol=2e-6, atol=0)


@pytest.mark.parametrize("n", ar.EMD_SIZES)
def test_gaussian_gap_within_the_auction_bound(n, device):
    from si_mamba_amd.emd import default_max_rounds
    pairs = ar.emd_pairs(n)
    x, y, opt, cmax = ar.solved("gaussian", pairs, n, ar.emd_seed(n))
    dist, assign, rounds, conv = _run(x, y, device)
    got = _costs(x, y, assign)
    bound = n * 2.0 ** -14 * cmax
    print(f"n={n} gaussian rounds {rounds.tolist()} of {default_max_rounds(n)}; gap / bound "
          f"{((got - opt) / bound).tolist()}")
    assert conv.tolist() == [1] * pairs
    assert (got - opt <= bound).all(), (got - opt, bound)
    assert (got - opt >= -1e-9 * opt).all()                               # the solver's optimum is the optimum
    np.testing.assert_allclose(dist.double().numpy(), got / n, rtol=2e-6, atol=0)


@pytest.mark.parametrize("n", [2, 32, 65, 1024])
def test_permuted_copy_is_matched_back(n, device):
    """y a permutation of x, all points distinct and at least 1/64 apart (squared): every other matching costs at
    least 2/64, more than n * eps, so the auction must return the permutation itself and the distance 0."""
    pairs = ar.emd_pairs(n)
    x = torch.stack([ar.distinct_lattice(n, 300 + n + p) for p in range(pairs)])
    g = torch.Generator().manual_seed(n)
    perm = torch.stack([torch.randperm(n, generator=g) for _ in range(pairs)])
    y = torch.gather(x, 1, perm[..., None].expand(-1, -1, 3))                # y[j] = x[perm[j]]
    dist, assign, rounds, conv = _run(x, y, device, eps=ar.lattice_eps(n))
    assert conv.tolist() == [1] * pairs
    assert dist.tolist() == [0.0] * pairs
    assert np.array_equal(assign, torch.argsort(perm, dim=1).numpy())       # y[assign[i]] = x[i]


@pytest.mark.parametrize("n", [1, 3, 64, 200])
def test_all_points_identical(n, device):
    pairs = ar.emd_pairs(n)
    x = torch.full((pairs, n, 3), 0.375)
    dist, assign, rounds, conv = _run(x, x.clone(), device)
    _costs(x, x, assign)
    assert dist.tolist() == [0.0] * pairs and conv.tolist() == [1] * pairs


def test_round_cap_ends_the_call_with_a_permutation(device):
    x, y, _, _ = ar.solved("gaussian", 5, 64, ar.emd_seed(64))
    dist, assign, rounds, conv = _run(x, y, device, max_rounds=1)
    got = _costs(x, y, assign)
    assert torch.isfinite(dist).all() and conv.tolist() == [0] * 5 and rounds.tolist() == [1] * 5
    np.testing.assert_allclose(dist.double().numpy(), got / 64, rtol=2e-6, atol=0)


@pytest.mark.parametrize("n", [33, 256])
def test_repeatable(n, device):
    x, y, _, _ = ar.solved("gaussian", ar.emd_pairs(n), n, ar.emd_seed(n))
    a, b = _run(x, y, device), _run(x, y, device)
    assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_single_pair_and_other_dtypes(device):
    from si_mamba_amd import earth_movers_distance
    x, y, _, _ = ar.solved("lattice", 5, 32, ar.emd_seed(32))
    eps = ar.lattice_eps(32)
    want = earth_movers_distance(x.to(device), y.to(device), eps=eps)
    one = earth_movers_distance(x[3].to(device), y[3].to(device), eps=eps, return_assignment=True)
    assert one[0].shape == () and one[1].shape == (32,) and one[2].shape == () and one[3].shape == ()
    assert torch.equal(one[0], want[3])
    assert torch.equal(earth_movers_distance(x.double().to(device), y.half().to(device), eps=eps), want)


@pytest.mark.parametrize("n", [32, 65])
def test_gradients_hold_the_matching_fixed(n, device):
    from si_mamba_amd import earth_movers_distance
    pairs = ar.emd_pairs(n)
    x, y, _, _ = ar.solved("gaussian", pairs, n, ar.emd_seed(n))
    xd, yd = x.to(device).requires_grad_(), y.to(device).requires_grad_()
    dout = torch.linspace(0.5, 2.0, pairs)
    dist, assign, _, _ = earth_movers_distance(xd, yd, return_assignment=True)
    (dist * dout.to(device)).sum().backward()
    x64, y64 = x.double().requires_grad_(), y.double().requires_grad_()
    idx = assign.cpu().long()[..., None].expand(-1, -1, 3)
    ref = ((x64 - y64.gather(1, idx)) ** 2).sum(-1).mean(-1)
    (ref * dout.double()).sum().backward()
    for got, want in ((xd.grad, x64.grad), (yd.grad, y64.grad)):
        err = (got.cpu().double() - want).abs().max() / want.abs().max()
        assert err <= 2e-6, err
    # one side only
    xd2 = x.to(device).requires_grad_()
    earth_movers_distance(xd2, y.to(device)).sum().backward()
    assert xd2.grad is not None and torch.isfinite(xd2.grad).all()


def test_captured_in_a_graph(device):
    from si_mamba_amd import earth_movers_distance
    n, pairs = 32, 5
    x, y, _, _ = ar.solved("gaussian", pairs, n, ar.emd_seed(n))
    x2, y2, _, _ = ar.solved("lattice", pairs, n, ar.emd_seed(n))
    sx, sy = x.to(device), y.to(device)
    earth_movers_distance(sx, sy)                                            # loads the library outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = earth_movers_distance(sx, sy, return_assignment=True)
    for a, b in ((x, y), (x2, y2)):
        sx.copy_(a.to(device))
        sy.copy_(b.to(device))
        graph.replay()
        torch.cuda.synchronize()
        eager = earth_movers_distance(a.to(device), b.to(device), return_assignment=True)
        for got, want in zip(out, eager):
            assert torch.equal(got, want)


def test_mae_with_emd_loss(device):
    from si_mamba_amd import earth_movers_distance
    from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
    torch.manual_seed(0)
    cfg = default_mae_config(trans_dim=64, encoder_dims=64, depth=2, decoder_depth=2, num_group=32, group_size=16,
                             knn_graph=6, k_top_eigenvectors=3, drop_path=0., loss="emd")
    m = Point_MAE_Mamba(cfg).to(device).train()
    g = torch.Generator().manual_seed(7)
    pts = torch.randn(3, 256, 3, generator=g).to(device)
    loss, parts = m(pts, return_parts=True)
    loss.backward()
    assert torch.isfinite(loss)
    bad = [k for k, p in m.named_parameters()
           if not k.startswith("decoder_pos_embed.") and (p.grad is None or not torch.isfinite(p.grad).all())]
    assert not bad, bad
    with torch.no_grad():
        dist, _, _, conv = earth_movers_distance(parts["rebuild"], parts["gt"], return_assignment=True)
    assert bool(conv.all())
    assert torch.equal(loss.detach(), dist.mean())
    m.eval()
    mask = parts["mask"]
    with torch.no_grad():
        want = m(pts, mask=mask)
        _, _, loss_patches = m.reconstruct(pts, mask=mask)
    assert loss_patches.shape[0] == 3
    assert abs(float(loss_patches.mean()) - float(want)) <= 1e-6 * abs(float(want))
