"""GPU parity of the MAE pre-training path (BASELINE config 4): Chamfer kernels against the
oracle's restatement of pytorch3d's published semantics, and the whole Point_MAE_Mamba data flow (mask selection,
token restore, decoder, masked-token selection, loss) against the oracle's restatement of the reference's
boolean-mask / loop code on the same weights, mask and orders."""
import pytest
import torch

from helpers import clouds, nerr, peak_err
from oracle import mae_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pairs,n,m", [(1000, 32, 32), (7, 64, 17), (33, 5, 64), (1, 1, 1)])
def test_chamfer_matches_oracle(pairs, n, m, device):
    from si_mamba_amd.mae import chamfer_distance
    g = torch.Generator().manual_seed(pairs)
    x = torch.randn(pairs, n, 3, generator=g)
    y = torch.randn(pairs, m, 3, generator=g)
    w = torch.rand(pairs, generator=g)
    xa = x.to(device).requires_grad_(True)
    da = chamfer_distance(xa, y.to(device))
    (da * w.to(device)).sum().backward()
    xb = x.clone().requires_grad_(True)
    db = mae_ref.chamfer_distance(xb, y)
    (db * w).sum().backward()
    assert peak_err(da, db) < 1e-5
    assert peak_err(xa.grad, xb.grad) < 1e-5


def test_chamfer_golden_fixture(device):
    import os
    import numpy as np
    from si_mamba_amd.mae import chamfer_distance
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "chamfer_mae.npz"))
    x = torch.from_numpy(z["pred"]).to(device).requires_grad_(True)
    d = chamfer_distance(x, torch.from_numpy(z["gt"]).to(device))
    (d * torch.from_numpy(z["wsum"]).to(device)).sum().backward()
    assert peak_err(d, torch.from_numpy(z["dist"])) < 1e-5
    assert peak_err(x.grad, torch.from_numpy(z["grad_pred"])) < 1e-5


@pytest.mark.parametrize("full,dtype", [(False, torch.float32), (True, torch.float32), (True, torch.bfloat16)])
def test_mae_forward_matches_oracle_flow(full, dtype, device):
    """Small fp32 model, and BASELINE config 4's architecture (12 + 4 blocks, d = 384, 64 patches, mask 0.6: encoder
    L = 208, decoder L = 512) in fp32 and under bf16 autocast as tools/runner_pretrain.py:243 runs it.  Tolerances on
    the normalised error: 2e-3 fp32 (two stacked models), 1e-2 bf16 against the oracle restated with the autocast
    roundings (tests/compose.py)."""
    from compose import oracle_stack
    from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
    torch.manual_seed(0)
    if full:
        cfg = default_mae_config(drop_path=0.)
        B, G, N, d = 2, 64, 1024, 384
    else:
        cfg = default_mae_config(trans_dim=64, encoder_dims=64, depth=2, decoder_depth=2, num_group=32, group_size=16,
                                 knn_graph=6, k_top_eigenvectors=3, drop_path=0.)
        B, G, N, d = 3, 32, 256, 64
    bf16 = dtype == torch.bfloat16
    io = torch.bfloat16 if bf16 else None
    tol = 1e-2 if bf16 else 2e-3
    m = Point_MAE_Mamba(cfg).to(device).eval()
    with torch.no_grad():
        m.mask_token.normal_(std=0.5)
    pts = clouds(B, N, 7)
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        nb, center, _ = m.group_divider(pts.to(device))
        mask = m.MAE_encoder._mask_center_rand(center, generator=gen)
        assert int(mask.sum()) == B * int(0.6 * G)
        loss, parts = m(pts.to(device), mask=mask, return_parts=True)
        tokens = m.MAE_encoder.encoder(nb).cpu()
        pos = m.MAE_encoder.pos_embed(center).cpu()
    if full:
        assert parts["x_vis"].shape == (B, 208, 384) and parts["x_full"].shape == (B, 512, 384)
    orders = parts["orders"].cpu()
    nb, center, mask = nb.cpu(), center.cpu(), mask.cpu()
    cpu = m.cpu()
    P = mae_ref.permutation_matrices(orders, G)
    r = (lambda t: t.to(torch.bfloat16).float()) if bf16 else (lambda t: t)
    w = cpu.increase_dim[0]
    # increase_dim is a 1x1 Conv1d: a bf16 GEMM with fp32 accumulation under autocast
    inc = lambda t: r(torch.nn.functional.conv1d(r(t), r(w.weight), r(w.bias)))
    with torch.no_grad():
        enc_blocks = oracle_stack(cpu.MAE_encoder.blocks, d, io)
        enc = mae_ref.encoder_flow(tokens.float(), pos.float(), nb, center, mask, P, True,
                                   lambda x, p: enc_blocks(x.to(tokens.dtype), p.to(pos.dtype)), cpu.MAE_encoder.norm)
        x_vis, masks, pos_mask, pos_full, mask_tensor, snb = enc
        dec_blocks = oracle_stack(cpu.MAE_decoder.blocks, d, io)
        want_loss, rebuild, gt, x_full = mae_ref.decoder_flow(
            x_vis, cpu.mask_token, masks, mask_tensor, pos_full, snb, cfg.transformer_config.mask_ratio, G,
            lambda x, p: cpu.MAE_decoder.norm(dec_blocks(x, p.to(pos.dtype))), inc)
    scale = lambda a, b: nerr(a.float(), b.float())
    assert scale(parts["x_vis"], x_vis) < tol
    assert torch.equal(parts["pos_full"].float().cpu(), pos_full) and torch.equal(parts["pos_mask"].float().cpu(), pos_mask)
    assert scale(parts["x_full"], x_full) < tol
    assert torch.equal(parts["gt"].cpu(), gt)
    assert scale(parts["rebuild"], rebuild) < tol
    assert abs(float(loss) - float(want_loss)) < tol * max(1.0, abs(float(want_loss)))


def test_mae_train_step_reference_sizes(device):
    """BASELINE config 4 architecture (12 + 4 blocks, d=384, 64 patches, mask 0.6: encoder L=208, decoder L=512),
    bf16 autocast like tools/runner_pretrain.py:243: fwd + bwd."""
    from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
    torch.manual_seed(0)
    m = Point_MAE_Mamba(default_mae_config()).to(device).train()
    pts = clouds(8, 1024, 2).to(device)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss, parts = m(pts, return_parts=True)
    assert parts["x_vis"].shape == (8, 208, 384) and parts["x_full"].shape == (8, 512, 384)
    loss.backward()
    assert torch.isfinite(loss)
    # decoder_pos_embed is dead in the reference's spectral branch too (it reuses the encoder's pos_embed, :3192;
    # the reason for find_unused_parameters=True at tools/runner_pretrain.py:116); kept for state-dict parity
    bad = [k for k, p in m.named_parameters()
           if not k.startswith("decoder_pos_embed.") and (p.grad is None or not torch.isfinite(p.grad).all())]
    assert not bad, bad
    assert all(p.grad is None for k, p in m.named_parameters() if k.startswith("decoder_pos_embed."))


def test_config4_full_batch_step(device):
    """BASELINE config 4 as a whole step at the per-GPU batch the metric names: B = 64 clouds of 1024 points -> 64
    patches, mask 0.6, encoder L = 208 over 12 blocks, decoder L = 512 over 4 (cfgs/pretrain.yaml:37-68), in fp32 and
    under bf16 autocast (tools/runner_pretrain.py:243).  Size-independent properties tie the full batch to the small
    cases checked against the oracle (the ones config 3 uses, tests/test_gpu_model.py):
      * eval-mode reconstructions of samples 0-1 inside the batch of 64 equal those of the model run on just those two
        (same mask rows);
      * with frozen statistics the summed Chamfer loss is additive over samples, so every parameter gradient of the
        batch of 64 equals grad(first 32) + grad(last 32): the backward's batch reductions at two grid sizes -- at
        these row counts (64 x 768 = 49 152) both scan directions run the lanes-per-channel kernels;
      * the training-mode bf16 step (batch statistics, DropPath, random masks) gives a finite loss and gradients.
    Tolerances: 1e-3 in fp32.  Under autocast the two sides of each comparison run DIFFERENT library GEMM kernels (the
    batch size selects them) and every block rounds its activations to bf16, so they are held to 3e-2 -- the bf16
    arithmetic itself is held to the oracle at 1e-2 by test_mae_forward_matches_oracle_flow."""
    from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
    torch.manual_seed(0)
    cfg = default_mae_config()                      # DropPath / dropout at the config's rates: off in eval mode
    m = Point_MAE_Mamba(cfg).to(device).eval()
    B, G = 64, cfg.num_group
    pts = clouds(B, 1024, 41).to(device)
    nm = int(cfg.transformer_config.mask_ratio * G)
    gen = torch.Generator().manual_seed(6)
    mask = (torch.rand(B, G, generator=gen).argsort(dim=1).argsort(dim=1) < nm).to(device)      # nm True per row
    for on, tol in ((False, 1e-3), (True, 3e-2)):
        amp = torch.autocast("cuda", dtype=torch.bfloat16, enabled=on)
        with torch.no_grad(), amp:
            _, full = m(pts, mask=mask, return_parts=True)
            _, two = m(pts[:2], mask=mask[:2], return_parts=True)
        assert full["x_vis"].shape == (B, 208, 384) and full["x_full"].shape == (B, 512, 384)
        per = full["rebuild"].shape[0] // B
        assert nerr(full["rebuild"][:2 * per].float(), two["rebuild"].float()) < tol, on

        def grads(sl):
            m.zero_grad(set_to_none=True)
            with amp:
                loss, parts = m(pts[sl], mask=mask[sl], return_parts=True)
            (loss * parts["rebuild"].shape[0]).backward()            # mean over (samples x masked patches) -> sum
            return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

        g_all, g_a, g_b = grads(slice(0, 64)), grads(slice(0, 32)), grads(slice(32, 64))
        assert set(g_all) == set(g_a) == set(g_b) and len(g_all) > 100
        for k in g_all:
            assert nerr(g_all[k], g_a[k] + g_b[k]) < tol, (on, k)
    m.train()
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = m(pts)
    loss.backward()
    assert torch.isfinite(loss)
    bad = [k for k, p in m.named_parameters()
           if not k.startswith("decoder_pos_embed.") and (p.grad is None or not torch.isfinite(p.grad).all())]
    assert not bad, bad
