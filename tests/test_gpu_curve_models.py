"""GPU: the models on space-filling-curve orders (method "CURVE", transformer_config.ordering "curve").  The orders are
a second producer for the (B, k, G) interface the SAST machinery consumes, so what is checked is that the models hand
exactly curve_order's orders (tests/curve_ref.py) to that machinery and that every SAST route still applies."""
import numpy as np
import pytest
import torch

import curve_ref as cr
from helpers import clouds, nerr

pytestmark = pytest.mark.gpu

SMALL = dict(trans_dim=64, encoder_dims=64, depth=2, num_group=32, group_size=16)


def test_order_tokens_curve_is_the_sast_assembly_of_the_reference_order(device):
    from si_mamba_amd import spectral
    g = torch.Generator().manual_seed(3)
    B, G, C = 3, 50, 16
    center = clouds(B, G, 5)
    x, pos = torch.randn(B, G, C, generator=g), torch.randn(B, G, C, generator=g)
    ref = torch.from_numpy(cr.order(center.numpy())[0]).to(device)
    order = spectral.curve_order(center.to(device))
    assert torch.equal(order, ref)
    for reverse in (True, False):
        got = spectral.order_tokens("CURVE", (x.to(device), pos.to(device), center.to(device)), center.to(device), order,
                                    4, reverse)
        idx = spectral.sast_index_map(ref, reverse)
        assert idx.shape == (B, spectral.sast_len(4, G, reverse))
        for t, src in zip(got, (x, pos, center)):
            assert torch.equal(t, spectral.take(src.to(device), idx))


def test_pointmamba_curve_routes_agree_and_train(device):
    from si_mamba_amd import seq_expand, spectral
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    cfg = default_config(method="CURVE", curves=("hilbert", "z", "hilbert-trans"), curve_bits=8, cls_dim=5, **SMALL)
    m = PointMamba(cfg).to(device).eval()
    pts = clouds(4, 256, 9).to(device)
    assert m.n_orders() == 3 and m.seq_len() == 2 * 3 * 32 and m._on_tokens()
    # the model's orders are curve_order's with the configured curves and bits
    with torch.no_grad():
        _, center, _ = m.group_divider(pts)
        want = cr.order(center.cpu().numpy(), cfg.curves, 8)[0]
        np.testing.assert_array_equal(m.spectral_order(center).cpu().numpy(), want)
        np.testing.assert_array_equal(m.token_index(center).cpu().numpy(),
                                      spectral.sast_index_map(torch.from_numpy(want)).numpy())
    # on the distinct tokens (the default) and handed the assembled sequence: the same logits.  1e-5 on the normalised
    # error, the bound tests/test_gpu_model.py holds the two routes of the stack to: the same fp32 arithmetic on the same
    # values, block 0's head once per token instead of once per position
    calls = []
    real = seq_expand.seq_gather_last
    seq_expand.seq_gather_last = lambda *a: (calls.append(1), real(*a))[1]
    try:
        with torch.no_grad():
            on_tokens = m(pts)
    finally:
        seq_expand.seq_gather_last = real
    assert calls, "the distinct-token route was not taken"
    m._on_tokens = lambda: False
    try:
        with torch.no_grad():
            assembled = m(pts)
    finally:
        del m._on_tokens
    assert on_tokens.shape == (4, 5) and nerr(on_tokens, assembled) < 1e-5
    # a training step: finite, and a gradient for every parameter
    m.train()
    logits = m(pts)
    loss, _ = m.get_loss_acc(logits, torch.tensor([0, 1, 2, 3], device=device))
    loss.backward()
    assert torch.isfinite(logits).all() and torch.isfinite(loss)
    bad = [k for k, p in m.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not bad, bad


def test_pointmamba_curve_keeps_sast_state_and_refusals(device):
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    curve = PointMamba(default_config(method="CURVE", **SMALL)).to(device).eval()
    sast = PointMamba(default_config(method="SAST", knn_graph=6, **SMALL)).to(device).eval()
    assert list(curve.state_dict()) == list(sast.state_dict())
    assert [tuple(v.shape) for v in curve.state_dict().values()] == [tuple(v.shape) for v in sast.state_dict().values()]
    sast.load_state_dict(curve.state_dict())
    with pytest.raises(ValueError, match="add_after_layer"):
        PointMamba(default_config(method="CURVE", add_after_layer=True, **SMALL))
    pts = clouds(2, 256, 1).to(device)
    with pytest.raises(NotImplementedError, match="SAST route only"):
        curve(pts, gt=torch.zeros(2, dtype=torch.long, device=device))
    with torch.no_grad():                                                   # SAST itself is as it was
        logits, policy = sast(pts, gt=torch.zeros(2, dtype=torch.long, device=device))
    assert logits.shape == (2, 15) and policy.shape == (2,)


def test_pointmamba_curve_forward_captured_as_one_graph(device):
    """The CURVE forward, its order on the side stream included, as one hipGraph replayed on other clouds: the bound of
    tests/test_gpu_model.py::test_graphed_inference_matches_eager for the SAST forward."""
    from si_mamba_amd.graphed import GraphedForward
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    m = PointMamba(default_config(method="CURVE", drop_path=0., **SMALL)).to(device).eval()
    a, b = clouds(4, 256, 2).to(device), clouds(4, 256, 3).to(device)
    with torch.no_grad():
        ea, eb = m(a).clone(), m(b).clone()
    g = GraphedForward(m, a)
    ga = g(a).clone()
    gb = g(b).clone()
    assert (ga - ea).abs().max() < 1e-4 and (gb - eb).abs().max() < 1e-4
    assert not torch.equal(ea, eb)               # the two inputs really give different outputs


def test_partseg_curve_step(device):
    from si_mamba_amd.seg import PartSegMamba, default_seg_config, get_loss
    torch.manual_seed(0)
    cfg = default_seg_config(trans_dim=64, depth=4, fetch_idx=(1, 2, 3), num_group=32, group_size=16, method="CURVE",
                             curves=("hilbert", "z-trans"), curve_box=(-1, 1))
    m = PartSegMamba(50, cfg).to(device).train()
    B, N = 2, 512
    pts = clouds(B, N, 5).transpose(1, 2).contiguous().to(device)
    label = torch.nn.functional.one_hot(torch.tensor([3, 7]), 16).float().to(device)
    with torch.no_grad():
        _, center, _ = m.group_divider(pts.transpose(1, 2).contiguous())
        np.testing.assert_array_equal(m._spectral(center).cpu().numpy(),
                                      cr.order(center.cpu().numpy(), cfg.curves, 10, (-1, 1))[0])
    out = m(pts, label)
    assert out.shape == (B, N, 50)
    loss = get_loss()(out.reshape(-1, 50), torch.randint(0, 50, (B * N,), device=device))
    loss.backward()
    assert torch.isfinite(loss)
    bad = [k for k, p in m.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not bad, bad


def test_mae_curve_step_and_orders_by_hand(device):
    from si_mamba_amd import spectral
    from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
    torch.manual_seed(0)
    cfg = default_mae_config(trans_dim=64, encoder_dims=64, depth=2, decoder_depth=2, num_group=32, group_size=16,
                             drop_path=0., ordering="curve", curves=("hilbert", "hilbert-trans", "z"))
    m = Point_MAE_Mamba(cfg).to(device).eval()
    pts = clouds(3, 256, 7).to(device)
    with torch.no_grad():
        _, center, _ = m.group_divider(pts)
        mask = m.MAE_encoder._mask_center_rand(center, generator=torch.Generator().manual_seed(11))
        loss, parts = m(pts, mask=mask, return_parts=True)
        by_hand = m(pts, mask=mask, orders=spectral.curve_order(center, cfg.transformer_config.curves))
    np.testing.assert_array_equal(parts["orders"].cpu().numpy(),
                                  cr.order(center.cpu().numpy(), cfg.transformer_config.curves)[0])
    assert parts["orders"].shape == (3, 3, 32) and parts["x_full"].shape[1] == 2 * 3 * 32
    assert torch.isfinite(loss) and loss.view(1).view(torch.int32).item() == by_hand.view(1).view(torch.int32).item()
    # a training step on the curve orders
    m.train()
    step = m(pts)
    step.backward()
    assert torch.isfinite(step)
    bad = [k for k, p in m.named_parameters()
           if not k.startswith("decoder_pos_embed.") and (p.grad is None or not torch.isfinite(p.grad).all())]
    assert not bad, bad
