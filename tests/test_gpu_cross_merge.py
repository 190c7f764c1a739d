"""GPU: add_after_layer=True -- the gather-sum-scatter kernel (csrc/cross_merge.hip) against the reference's own
sequence of torch ops bit for bit, its backward against float64 autograd within the bound of its 2k - 1 fp32 additions,
and PointMamba with the option on against a CPU composition, against the composed ops, and through a hipGraph."""
import pytest
import torch

from helpers import clouds, nerr
from oracle import scan_ref
from test_cross_merge_abi import eigvecs_and_order, restated_merge_expand

pytestmark = pytest.mark.gpu


def _raw(x, gather_idx, scatter_idx):
    """The C entry point on a y prefilled with NaN: every row has to be written."""
    from si_mamba_amd import _lib
    lib = _lib.load()
    B, L, C = x.shape
    M, G = gather_idx.shape[1:]
    y = torch.full_like(x, float("nan"))
    with torch.cuda.device(x.device):
        rc = lib.simamba_gather_sum_scatter(x.data_ptr(), gather_idx.data_ptr(), scatter_idx.data_ptr(), y.data_ptr(),
                                            B, L, G, M, C, _lib.dtype_code(x.dtype), _lib.stream_ptr(x.device))
    assert rc == 0, rc
    return y


def _case(B, G, k, C, device, seed=0):
    from si_mamba_amd.cross_merge import cross_merge_maps
    vecs, order = eigvecs_and_order(B, G, k, seed=seed + G + k)
    x = torch.randn(B, 2 * k * G, C, generator=torch.Generator().manual_seed(seed + C))
    order = order.to(device)
    return vecs, order, cross_merge_maps(order), x


@pytest.mark.parametrize("B,G,k,C", [(2, 8, 1, 4), (3, 37, 3, 36), (2, 64, 4, 384), (2, 128, 4, 384),
                                     (1, 512, 4, 384)])
def test_kernel_equals_composed_ops_fp32(B, G, k, C, device):
    from si_mamba_amd.cross_merge import cross_merge, cross_merge_composed
    _, order, (src, dst), x = _case(B, G, k, C, device)
    x = x.to(device)
    want = cross_merge_composed(x, order)
    got = _raw(x, src, dst)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
    assert torch.equal(_raw(x, src, dst), got)
    assert torch.equal(cross_merge(x, (src, dst)), want)


def test_kernel_bf16_is_the_fp32_sum_rounded_once(device):
    B, G, k, C = 2, 64, 4, 384
    _, order, (src, dst), x = _case(B, G, k, C, device)
    x = x.to(device).to(torch.bfloat16)
    got = _raw(x, src, dst)
    assert torch.isfinite(got.float()).all()
    flat = lambda m: m.flatten(1).long().unsqueeze(-1).expand(-1, -1, C)
    rows = torch.gather(x.float(), 1, flat(src)).view(B, 2 * k, G, C)
    acc = rows[:, 0] + rows[:, k]
    for i in range(1, k):
        acc = acc + (rows[:, i] + rows[:, k + i])
    want = torch.empty_like(x)
    want.scatter_(1, flat(dst), acc.to(torch.bfloat16).repeat(1, 2 * k, 1))
    assert torch.equal(got, want)


@pytest.mark.parametrize("B,G,k,C", [(3, 37, 3, 36), (2, 128, 4, 384)])
def test_backward_within_the_bound_of_its_additions(B, G, k, C, device):
    """dh is a sum of 2k dout rows in fp32, 2k - 1 additions: |got - want| <= 2k * 2^-24 * sum |terms| elementwise,
    want and the sum of the absolute terms from float64 autograd of the restatement."""
    from si_mamba_amd.cross_merge import cross_merge
    vecs, _, maps, x = _case(B, G, k, C, device)
    dout = torch.randn(x.shape, generator=torch.Generator().manual_seed(7))
    h = x.to(device).requires_grad_(True)
    cross_merge(h, maps).backward(dout.to(device))
    h64 = x.double().requires_grad_(True)
    seq = restated_merge_expand(h64, vecs, k)[1]
    want, = torch.autograd.grad(seq, h64, dout.double(), retain_graph=True)
    terms, = torch.autograd.grad(seq, h64, dout.double().abs())
    err = (h.grad.cpu().double() - want).abs()
    bound = 2 * k * 2.0 ** -24 * terms
    print(f"backward ({B}, {G}, {k}, {C}): max err {float(err.max()):.3e}, max err / bound "
          f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())


# ---- the model ----------------------------------------------------------------------------------------------------
K, DEPTH, DIM = 3, 3, 64


def _config(**over):
    from si_mamba_amd.point_mamba import default_config
    return default_config(trans_dim=DIM, encoder_dims=DIM, depth=DEPTH, num_group=16, group_size=8,
                          k_top_eigenvectors=K, knn_graph=6, drop_path=0., drop_out=0., drop_out_in_block=0., **over)


@pytest.fixture(scope="module")
def small(device):
    from si_mamba_amd.point_mamba import PointMamba
    torch.manual_seed(0)
    return PointMamba(_config(add_after_layer=True)).to(device), clouds(2, 128, 3).to(device)


def test_model_matches_cpu_composition(small, device):
    m, pts = small
    m.eval()
    with torch.no_grad():
        got = m(pts).cpu()
        # the ordering itself is covered by tests/test_gpu_spectral.py: take the device's tokens in sequence order
        nb, center, _ = m.group_divider(pts)
        order = m.spectral_order(center)
        x, spos = m.order_tokens(m.encoder(nb), m.pos_embed(center), center, order)
        x, spos, order = x.cpu(), spos.cpu(), order.cpu()
    # stand-in eigenvectors whose sort is the device's order: patch order[i][r] gets the value r
    B, k, G = order.shape
    vecs = torch.empty(B, G, k).scatter_(1, order.transpose(1, 2), torch.arange(G).float().view(1, G, 1).expand(B, G, k))
    state = {n: v.detach().cpu() for n, v in m.state_dict().items()}
    from si_mamba_amd.point_mamba import PointMamba
    cpu = PointMamba(_config(add_after_layer=True)).eval()
    cpu.load_state_dict(state)
    mixers = []
    for layer in cpu.blocks.layers:
        r = scan_ref.MambaRef(DIM)
        r.load_state_dict(layer.mixer.state_dict())
        mixers.append(r.eval())
    with torch.no_grad():
        hidden, residual = x + spos, None
        for i, layer in enumerate(cpu.blocks.layers):
            residual = hidden if residual is None else hidden + residual
            hidden = mixers[i](layer.norm(residual))
            hidden = restated_merge_expand(hidden, vecs, k)[1]
        out = cpu.norm(cpu.blocks.norm_f(hidden + residual))
        want = cpu.cls_head_finetune(out.mean(1))
    assert got.shape == want.shape == (2, 15)
    err = float((got - want).abs().max())
    print(f"model parity: max err {err:.3e}, |want|max {float(want.abs().max()):.3e}")
    assert err < 2e-3 * max(1.0, float(want.abs().max()))


def _train_step(m, pts, autocast=False):
    m.train()
    m.zero_grad(set_to_none=True)
    torch.manual_seed(11)                                   # the head's Dropout(0.5) draws the same masks every time
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        logits = m(pts)
    loss = logits.float().square().sum()
    loss.backward()
    return logits.detach().clone(), {n: p.grad.clone() if p.grad is not None else None for n, p in m.named_parameters()}


def test_kernel_against_composed_in_training(small, device):
    from si_mamba_amd.block import MixerModel_add
    m, pts = small
    assert type(m.blocks) is MixerModel_add and m.blocks.composed is False
    logits, grads = _train_step(m, pts)
    try:
        m.blocks.composed = True
        want_logits, want = _train_step(m, pts)
    finally:
        del m.blocks.composed
    assert m.blocks.composed is False
    assert torch.equal(logits, want_logits)
    missing = [n for n, g in grads.items() if g is None or not torch.isfinite(g).all()]
    assert not missing, missing
    errs = {n: nerr(grads[n], want[n]) for n in grads}
    worst = max(errs, key=errs.get)
    print(f"gradients, kernel against composed: worst {worst} {errs[worst]:.3e}; largest gradient "
          f"{max(float(g.abs().max()) for g in want.values()):.3e}")
    assert errs[worst] < 1e-3, (worst, errs[worst])
    logits, grads = _train_step(m, pts, autocast=True)
    assert torch.isfinite(logits).all()
    assert all(g is not None and torch.isfinite(g).all() for g in grads.values())


def test_no_effect_when_off(device):
    from si_mamba_amd import _lib
    from si_mamba_amd.block import MixerModel
    from si_mamba_amd.point_mamba import PointMamba
    torch.manual_seed(0)
    pts = clouds(2, 128, 3).to(device)
    m = PointMamba(_config(add_after_layer=False)).to(device).eval()
    assert type(m.blocks) is MixerModel
    before = _lib.counters.get("cross_merge", 0)
    with torch.no_grad():
        m(pts)
    assert _lib.counters.get("cross_merge", 0) == before


def test_graphed_forward_replays_the_eager_result(small, device):
    from si_mamba_amd import _lib
    from si_mamba_amd.graphed import GraphedForward
    m, pts = small
    m.eval()
    other = clouds(2, 128, 4).to(device)
    with torch.no_grad():
        before = _lib.counters.get("cross_merge", 0)
        ea, eb = m(pts).clone(), m(other).clone()
        assert _lib.counters["cross_merge"] == before + 2 * DEPTH
    g = GraphedForward(m, pts)
    ga = g(pts).clone()
    gb = g(other).clone()
    assert torch.equal(ga, ea) and torch.equal(gb, eb)
    assert not torch.equal(ea, eb)
