"""GPU: dense clouds and many patches end to end -- farthest-point sampling above 4096 points (the 1024-lane kernel of
csrc/fps.hip) and the models at 256 / 512 patches (the large-G spectral kernels)."""
import pytest
import torch

from compose import sast_gather_by_order
from helpers import clouds
from oracle import fps_ref, scan_ref, spectral_ref as sr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(2, 8192, 512), (3, 5000, 256), (1, 4097, 64)])
def test_farthest_point_sampling_dense_matches_oracle(shape, device):
    """Bit-exact against the restatement of pytorch3d's algorithm: start at 0, (dx^2 + dy^2) + dz^2 without FMA,
    first maximum on ties."""
    from si_mamba_amd import grouping
    B, N, K = shape
    pts = clouds(B, N, seed=N + K)
    centers, idx = grouping.sample_farthest_points(pts.to(device), K)
    wc, widx = fps_ref.sample_farthest_points(pts, K)
    assert torch.equal(idx.cpu(), widx)
    assert torch.equal(centers.cpu(), wc)
    assert (idx[:, 0] == 0).all() and all(len(set(r.tolist())) == K for r in idx.cpu())


def _oracle_head(m, x, p, d):
    h, res = x + p, None
    cpu = m.cpu()
    with torch.no_grad():
        for layer in cpu.blocks.layers:
            r = scan_ref.MambaRef(d)
            r.load_state_dict(layer.mixer.state_dict())
            res = h if res is None else h + res
            h = r(layer.norm(res))
        return cpu.cls_head_finetune(cpu.norm(cpu.blocks.norm_f(h + res)).mean(1))


@pytest.mark.parametrize("method", ["SAST", "HLT"])
def test_pointmamba_dense_forward_matches_oracle_composition(method, device):
    """8192 points, 512 patches of 32, small width: same weights, torch for the tokeniser, CPU oracle for the mixers.
    The device's eigenvectors and orders are first held to the oracle's (exact away from near-ties, as in
    tests/test_gpu_spectral_large.py); the oracle composition then runs on the device's ordering, so that a legitimate
    near-tie swap among 512 patches does not masquerade as a model error."""
    from si_mamba_amd import spectral
    from si_mamba_amd.point_mamba import PointMamba, default_config
    from test_gpu_spectral import align_sign
    from test_gpu_spectral_large import assert_order_matches_oracle
    torch.manual_seed(0)
    k = 4 if method == "SAST" else 3
    cfg = default_config(trans_dim=64, encoder_dims=64, depth=2, num_group=512, group_size=32, drop_path=0.,
                         method=method, k_top_eigenvectors=k)
    m = PointMamba(cfg).to(device).eval()
    m.hlt_rand = False
    pts = clouds(2, 8192, 3)
    with torch.no_grad():
        got = m(pts.to(device)).cpu()
        nb, center_d, _ = m.group_divider(pts.to(device))
        tokens, pos = m.encoder(nb).cpu(), m.pos_embed(center_d).cpu()
        center = center_d.cpu()
    assert center.shape == (2, 512, 3)
    if method == "SAST":
        adj = sr.create_graph_from_feature_space(center, cfg.knn_graph, cfg.alpha, True, False, True)
        _, dvecs, dorder = m.spectral_eigs(center_d)
    else:
        adj = sr.create_graph_from_centers(center, cfg.knn_graph, cfg.alpha, True, False, True)
        dadj = spectral.create_graph_from_centers(center_d, cfg.knn_graph, cfg.alpha, True, False, True)
        _, dvecs, _, _, dorder = spectral._eig(dadj, k, True, False, want_all=False, want_order=True)
    _, wvecs, all_vals, _ = sr.calc_top_k_eigenvalues_eigenvectors(adj, k, True)
    gv, sgn = align_sign(dvecs.cpu(), wvecs)
    err = (gv - wvecs).abs().amax(dim=1)
    gap = torch.minimum((all_vals[:, 1:k + 1] - all_vals[:, :k]).abs(),
                        torch.cat([torch.ones(2, 1), (all_vals[:, 1:k] - all_vals[:, :k - 1]).abs()], 1))
    assert (err * gap).max() < 8e-5
    worder = torch.sort(wvecs.transpose(1, 2), dim=2, stable=True)[1]
    assert_order_matches_oracle(dorder.cpu(), sgn, wvecs, worder, err, method)
    if method == "SAST":
        x, p = sast_gather_by_order(tokens, pos, dorder.cpu(), reverse=True)
        assert x.shape == (2, 4096, 64)
    else:
        x, p, _, _ = sr.hlt_order_and_assemble(tokens, pos, center, dvecs.cpu(), k)
    want = _oracle_head(m, x, p, 64)
    assert (got - want).abs().max() < 2e-3 * max(1.0, want.abs().max().item())


def test_pointmamba_train_step_512_patches(device):
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    m = PointMamba(default_config(trans_dim=128, encoder_dims=128, depth=2, num_group=512, group_size=32))
    m = m.to(device).train()
    pts = clouds(4, 8192, 1).to(device)
    gt = torch.randint(0, 15, (4,), device=device)
    loss, _ = m.get_loss_acc(m(pts), gt)
    loss.backward()
    assert torch.isfinite(loss)
    bad = [k for k, p in m.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not bad, bad


def test_mae_train_step_256_patches(device):
    from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
    torch.manual_seed(0)
    cfg = default_mae_config(trans_dim=128, encoder_dims=128, depth=2, decoder_depth=1, num_group=256)
    m = Point_MAE_Mamba(cfg).to(device).train()
    loss = m(clouds(2, 4096, 2).to(device))
    loss.backward()
    assert torch.isfinite(loss)
    bad = [k for k, p in m.named_parameters()
           if not k.startswith("decoder_pos_embed.") and (p.grad is None or not torch.isfinite(p.grad).all())]
    assert not bad, bad


@pytest.mark.parametrize("method", ["HLT", "SAST"])
def test_partseg_train_step_256_patches(method, device):
    from si_mamba_amd.seg import PartSegMamba, default_seg_config, get_loss
    torch.manual_seed(0)
    cfg = default_seg_config(num_group=256, method=method)
    m = PartSegMamba(50, cfg).to(device).train()
    B, N = 2, 4096
    pts = clouds(B, N, 5).transpose(1, 2).contiguous().to(device)
    label = torch.nn.functional.one_hot(torch.tensor([0, 3]), 16).float().to(device)
    target = torch.randint(0, 50, (B, N), device=device)
    out = m(pts, label)
    assert out.shape == (B, N, 50)
    loss = get_loss()(out.reshape(-1, 50), target.view(-1))
    loss.backward()
    assert torch.isfinite(loss)
    bad = [k for k, p in m.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not bad, bad
