"""GPU parity of the part-segmentation path (BASELINE config 5): the 3-NN interpolation
kernels against the oracle's restatement of pointnet2_utils.py:262-305, and the whole PartSegMamba forward against
the oracle composition (CPU mixers + reference-layout head) on the same weights.  Tolerance 1e-3 (fp32)."""
import pytest
import torch

from helpers import clouds, nerr, peak_err
from oracle import scan_ref, seg_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,N,S,C,dtype", [(2, 512, 64, 64, torch.float32), (3, 300, 37, 1152, torch.float32),
                                           (1, 2048, 256, 128, torch.float32), (2, 256, 3, 8, torch.float32),
                                           (2, 512, 64, 64, torch.bfloat16)])
def test_three_nn_interpolate_matches_oracle(B, N, S, C, dtype, device):
    from si_mamba_amd.interp import three_interpolate, three_nn
    pts = clouds(B, N, N + S)
    g = torch.Generator().manual_seed(C)
    centres = pts[:, torch.randperm(N, generator=g)[:S]].clone()       # centres coincide with points (as after FPS)
    if S >= 8:
        centres[:, S // 2:S // 2 + 2] = centres[:, :2]                  # exact duplicates: ties go to the lower index
    feats = torch.randn(B, S, C, generator=g)
    dout = torch.randn(B, N, C, generator=g)
    want, widx, ww = seg_ref.three_nn_interpolate(pts, centres, feats.to(dtype).float())
    idx, w = three_nn(pts.to(device), centres.to(device))
    if S >= 3:
        # the neighbour SETS agree wherever the third and fourth distances are separated; weights within 1e-4
        d = seg_ref.square_distance(pts, centres).sort(dim=-1, stable=True)[0]
        clear = ((d[:, :, 3] - d[:, :, 2]) > 1e-5) if S > 3 else torch.ones(B, N, dtype=torch.bool)
        same = (idx.cpu().long().sort(-1)[0] == widx.sort(-1)[0]).all(-1)
        assert bool(same[clear].all())
    f = feats.to(device).to(dtype).requires_grad_(True)
    out = three_interpolate(f, idx, w)
    assert peak_err(out, want) < (2e-4 if dtype == torch.float32 else 2e-2)
    out.backward(dout.to(device).to(dtype))
    fr = feats.to(dtype).float().clone().requires_grad_(True)
    (seg_ref.index_points(fr, idx.cpu().long()) * w.cpu().view(B, N, 3, 1)).sum(2).backward(dout.to(dtype).float())
    assert peak_err(f.grad, fr.grad) < (2e-4 if dtype == torch.float32 else 2e-2)


def test_interp_golden_fixture(device):
    import os
    import numpy as np
    from si_mamba_amd.interp import three_interpolate, three_nn
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "interp_seg.npz"))
    idx, w = three_nn(torch.from_numpy(z["xyz1"]).to(device), torch.from_numpy(z["xyz2"]).to(device))
    out = three_interpolate(torch.from_numpy(z["feats"]).to(device), idx, w)
    assert peak_err(out, torch.from_numpy(z["out"])) < 2e-4
    assert float((idx.cpu().sort(-1)[0] == torch.from_numpy(z["idx"]).sort(-1)[0]).float().mean()) > 0.99


@pytest.mark.parametrize("method", ["HLT", "SAST", "Point_MAMBA"])
def test_partseg_forward_matches_oracle_composition(method, device):
    from si_mamba_amd.seg import PartSegMamba, default_seg_config
    torch.manual_seed(0)
    cfg = default_seg_config(trans_dim=64, depth=4, fetch_idx=(1, 2, 3), num_group=32, group_size=16, drop_path=0.,
                             drop_path_rate=0., knn_graph=6, method=method, k_top_eigenvectors=3)
    m = PartSegMamba(50, cfg).to(device).eval()
    m.hlt_rand = False
    B, N = 2, 512
    pts = clouds(B, N, 3).transpose(1, 2).contiguous()                 # (B, 3, N)
    label = torch.zeros(B, 16); label[0, 3] = 1; label[1, 7] = 1
    with torch.no_grad():
        got = m(pts.to(device), label.to(device)).cpu()
        # the ordering itself is covered by tests/test_gpu_spectral.py: take the device's tokens in sequence order
        nb, center, _ = m.group_divider(pts.transpose(1, 2).contiguous().to(device))
        x, spos, scenter = m.order_tokens(m.encoder(nb), m.pos_embed(center), center)
        x, spos, scenter = x.cpu(), spos.cpu(), scenter.cpu()
    cpu = m.cpu()
    mixers = []
    for layer in cpu.blocks.layers:
        r = scan_ref.MambaRef(cfg.trans_dim)
        r.load_state_dict(layer.mixer.state_dict())
        mixers.append(r.eval())
    with torch.no_grad():
        feats = seg_ref.mixer_taps(cpu.blocks, mixers, x, spos)
        want = seg_ref.seg_head(cpu, pts, label, scenter, feats)
    assert got.shape == (B, N, 50)
    assert (got - want).abs().max() < 2e-3 * max(1.0, float(want.abs().max()))


def test_partseg_train_step_reference_sizes(device):
    """BASELINE config 5 architecture (12 blocks, d=384, 128 patches, HLT -> L=256, 2048 points): fwd+bwd."""
    from si_mamba_amd.seg import PartSegMamba, get_loss
    torch.manual_seed(0)
    m = PartSegMamba(50).to(device).train()
    B, N = 4, 2048
    pts = clouds(B, N, 5).transpose(1, 2).contiguous().to(device)
    label = torch.nn.functional.one_hot(torch.tensor([0, 3, 7, 15]), 16).float().to(device)
    target = torch.randint(0, 50, (B, N), device=device)
    out = m(pts, label)
    assert out.shape == (B, N, 50)
    loss = get_loss()(out.reshape(-1, 50), target.view(-1))
    loss.backward()
    assert torch.isfinite(loss)
    missing = [k for k, p in m.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not missing, missing


@pytest.mark.parametrize("method,npts", [("HLT", 2048), ("SAST", 2048)])
def test_partseg_full_depth_bf16_matches_oracle(method, npts, device):
    """BASELINE config 5: the ShapeNetPart architecture (12 blocks, d = 384, taps after layers 3 / 7 / 11, 128 patches
    of 32; HLT -> L = 256, SAST -> L = 1024) on 2048 points under bf16 autocast, against the oracle restated with the
    autocast roundings (tests/compose.py, oracle/seg_ref.py).  1e-2 on the normalised error of the per-point
    log-probabilities (north_star's bf16 tolerance)."""
    from compose import oracle_stack
    from si_mamba_amd.seg import PartSegMamba, default_seg_config
    torch.manual_seed(0)
    cfg = default_seg_config(drop_path=0., drop_path_rate=0., method=method)
    m = PartSegMamba(50, cfg).to(device).eval()
    m.hlt_rand = False
    B, N = 2, npts
    pts = clouds(B, N, 3).transpose(1, 2).contiguous()                 # (B, 3, N)
    label = torch.zeros(B, 16); label[0, 3] = 1; label[1, 7] = 1
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        got = m(pts.to(device), label.to(device)).float().cpu()
        nb, center, _ = m.group_divider(pts.transpose(1, 2).contiguous().to(device))
        x, spos, scenter = m.order_tokens(m.encoder(nb), m.pos_embed(center), center)
        x, spos, scenter = x.cpu(), spos.cpu(), scenter.cpu()
    assert x.shape == (B, 256 if method == "HLT" else 1024, 384)
    cpu = m.cpu()
    with torch.no_grad():
        feats = oracle_stack(cpu.blocks, 384, torch.bfloat16, taps=cpu.blocks.fetch_idx)(x, spos)
        want = seg_ref.seg_head(cpu, pts, label, scenter.float(), feats, io_dtype=torch.bfloat16)
    assert got.shape == (B, N, 50)
    assert nerr(got, want) < 1e-2
    # and the class decisions agree wherever the oracle's top-2 margin is not a near-tie
    top2 = want.topk(2, dim=-1)[0]
    clear = (top2[..., 0] - top2[..., 1]) > 0.1
    assert (got.argmax(-1) == want.argmax(-1))[clear].all()


@pytest.mark.parametrize("method", ["SAST", "HLT"])
def test_config5_full_batch_step(method, device):
    """BASELINE config 5 as a whole step at the reference's batch: B = 16 clouds of 2048 points -> 128 patches, 12 blocks
    (taps 3 / 7 / 11), SAST (L = 1024) and HLT (L = 256), fp32 and bf16 autocast (part_segmentation/main.py:59, :226).
    The same size-independent properties as configs 3 and 4: sub-batch log-probabilities equal those of the small run,
    gradient additivity over the batch with frozen statistics, finite training-mode bf16 step; 1e-3 in fp32, 3e-2
    between two bf16 runs through different library GEMM kernels (test_config4_full_batch_step explains)."""
    from si_mamba_amd.seg import PartSegMamba, default_seg_config, get_loss
    torch.manual_seed(0)
    cfg = default_seg_config(method=method)
    m = PartSegMamba(50, cfg).to(device).eval()
    m.hlt_rand = False                                   # the reference's torch.rand tie-break: off for comparisons
    B, N = 16, 2048
    pts = clouds(B, N, 9).transpose(1, 2).contiguous().to(device)
    label = torch.nn.functional.one_hot(torch.arange(B) % 16, 16).float().to(device)
    target = torch.randint(0, 50, (B, N), generator=torch.Generator().manual_seed(3)).to(device)
    for on, tol in ((False, 1e-3), (True, 3e-2)):
        amp = torch.autocast("cuda", dtype=torch.bfloat16, enabled=on)
        with torch.no_grad(), amp:
            full = m(pts, label)
            two = m(pts[:2], label[:2])
        assert full.shape == (B, N, 50)
        assert nerr(full[:2].float(), two.float()) < tol, on

        def grads(sl):
            m.zero_grad(set_to_none=True)
            with amp:
                out = m(pts[sl], label[sl])
            torch.nn.functional.nll_loss(out.reshape(-1, 50), target[sl].reshape(-1), reduction="sum").backward()
            return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

        g_all, g_a, g_b = grads(slice(0, 16)), grads(slice(0, 8)), grads(slice(8, 16))
        assert set(g_all) == set(g_a) == set(g_b) and len(g_all) > 100
        for k in g_all:
            assert nerr(g_all[k], g_a[k] + g_b[k]) < tol, (on, k)
    m.train()
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(pts, label)
    loss = get_loss()(out.reshape(-1, 50), target.view(-1))
    loss.backward()
    assert torch.isfinite(loss)
    bad = [k for k, p in m.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not bad, bad
