"""GPU parity of the fused out_proj -> (+ residual) -> LayerNorm kernel (csrc/out_norm_bf16.hip) against
float64 products of the bf16 operands with the reference's roundings (the out_proj output is a bf16 tensor under autocast:
models/block.py:72 then :56-58), and against this package's unfused route (library GEMM + add_layer_norm kernel)."""
import pytest
import torch

from helpers import nerr

pytestmark = pytest.mark.gpu


def _case(B, C, L, device, seed, residual=True, rowscale=False, beta=True):
    g = torch.Generator().manual_seed(seed)
    K = 2 * C
    y = torch.randn(B, K, L, generator=g).bfloat16()
    w = (torch.randn(C, K, generator=g) * K ** -0.5)
    res = torch.randn(B, L, C, generator=g) if residual else None
    rs = (torch.rand(B, generator=g) > 0.3).float() / 0.7 if rowscale else None
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    bt = 0.1 * torch.randn(C, generator=g) if beta else None
    dn = torch.randn(B, L, C, generator=g)
    dr = torch.randn(B, L, C, generator=g)
    mv = lambda t: None if t is None else t.to(device)
    return dict(y=mv(y), w=mv(w), res=mv(res), rs=mv(rs), gamma=mv(gamma), beta=mv(bt), dn=mv(dn), dr=mv(dr))


def _want(c, out_dtype):
    """float64 restatement with the roundings: bf16 operands, out_proj result rounded to bf16, fp32 residual stream."""
    y, w = c["y"].double().cpu(), c["w"].bfloat16().double().cpu()
    hid = torch.einsum("bkl,ck->blc", y, w).float().bfloat16().double()
    if c["res"] is not None:
        if c["rs"] is not None:
            hid = hid * c["rs"].double().cpu()[:, None, None]
        hid = hid + c["res"].double().cpu()
    res_out = hid.float()
    x = res_out.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    n = (x - mean) / torch.sqrt(var + 1e-5) * c["gamma"].double().cpu()
    if c["beta"] is not None:
        n = n + c["beta"].double().cpu()
    return n.to(out_dtype), res_out


@pytest.mark.parametrize("B,C,L", [(2, 128, 64), (1, 256, 200), (2, 384, 128), (1, 384, 1024), (3, 384, 72), (2, 256, 136)])
@pytest.mark.parametrize("flags", [(True, False, True), (False, False, True), (True, True, False)])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
def test_out_proj_add_ln_forward(B, C, L, flags, out_dtype, device):
    from si_mamba_amd.out_norm import out_proj_add_ln_fn
    residual, rowscale, beta = flags
    c = _case(B, C, L, device, seed=C + L, residual=residual, rowscale=rowscale, beta=beta)
    normed, res_out = out_proj_add_ln_fn(c["y"], c["w"], c["res"], c["gamma"], c["beta"], 1e-5, c["rs"], out_dtype)
    wn, wr = _want(c, out_dtype)
    assert normed.dtype == out_dtype and res_out.dtype == torch.float32
    # the residual stream: exact up to the rare bf16 rounding flip of an out_proj value (fp32 accumulation order)
    assert nerr(res_out, wr) < 1e-2
    assert ((res_out.cpu() - wr).abs() > 1e-6).float().mean() < 2e-2
    assert nerr(normed, wn) < (1e-2 if out_dtype == torch.bfloat16 else 5e-3)


@pytest.mark.parametrize("B,C,L", [(2, 384, 128), (1, 128, 64)])
def test_out_proj_add_ln_matches_unfused_route_and_backward(B, C, L, device):
    """Against out_proj by the library GEMM + the add_layer_norm kernel (what MixerModel runs when the fused kernel does
    not apply): forward within bf16 rounding flips, every gradient at 1e-2 (bf16)."""
    from si_mamba_amd.add_norm import add_layer_norm_fn
    from si_mamba_amd.out_norm import out_proj_add_ln_fn
    c = _case(B, C, L, device, seed=7, residual=True, rowscale=True, beta=True)
    outs = {}
    for fused in (True, False):
        y = c["y"].clone().requires_grad_(True)
        w = c["w"].clone().requires_grad_(True)
        res = c["res"].clone().requires_grad_(True)
        gamma = c["gamma"].clone().requires_grad_(True)
        beta = c["beta"].clone().requires_grad_(True)
        if fused:
            normed, res_out = out_proj_add_ln_fn(y, w, res, gamma, beta, 1e-5, c["rs"], torch.bfloat16)
        else:
            hid = torch.bmm(y.transpose(1, 2), w.bfloat16().t().unsqueeze(0).expand(B, -1, -1))
            normed, res_out = add_layer_norm_fn(hid, res, gamma, beta, 1e-5, rowscale=c["rs"], out_dtype=torch.bfloat16)
        ((normed.float() * c["dn"]).sum() + (res_out * c["dr"]).sum()).backward()
        outs[fused] = (normed.detach(), res_out.detach(), y.grad, w.grad, res.grad, gamma.grad, beta.grad)
    names = ("normed", "res_out", "dy", "dw", "dres", "dgamma", "dbeta")
    for n, a, b_ in zip(names, outs[True], outs[False]):
        assert nerr(a, b_) < 1e-2, n


@pytest.mark.parametrize("mode", ["expanded", "plain"])
@pytest.mark.parametrize("train", [True, False])
def test_mixer_model_fused_boundaries_match_op_by_op_route(mode, train, device):
    """MixerModel.forward under bf16 autocast: every block boundary (out_proj, DropPath-scaled add, LayerNorm --
    models/block.py:72, :56-58; the stack's norm_f, models/point_mamba.py:257-258) through the fused kernel against the
    same stack op by op (library out_proj GEMM + add_layer_norm kernel).  Same seed, so the same DropPath draws.
    Output, input gradients and every parameter gradient at bf16 tolerance; the counter shows the route was taken."""
    from si_mamba_amd import _lib
    from si_mamba_amd.block import MixerModel
    torch.manual_seed(3)
    B, G, d, n = 3, 32, 128, 3
    model = MixerModel(d, n, ssm_cfg={}, drop_path=0.2 if train else 0.0).to(device).train(train)
    g = torch.Generator().manual_seed(11)
    tok = torch.randn(B, G, d, generator=g).to(device)
    pos = torch.randn(B, G, d, generator=g).to(device)
    if mode == "expanded":
        idx = torch.stack([torch.cat([torch.randperm(G, generator=g) for _ in range(4)]) for _ in range(B)]).to(device)
        kw = dict(token_index=idx, balanced_index=True)
        dout = torch.randn(B, 4 * G, d, generator=g).to(device)
    else:
        kw = {}
        dout = torch.randn(B, G, d, generator=g).to(device)
    res = {}
    for fused in (True, False):
        model.zero_grad(set_to_none=True)
        t, p = tok.clone().requires_grad_(True), pos.clone().requires_grad_(True)
        _lib.counters.pop("out_proj_add_ln", None)
        torch.manual_seed(5)
        with _lib.fuse_out_norm(fused), torch.autocast("cuda", dtype=torch.bfloat16):
            out = model(t, p, **kw)
        assert _lib.counters.get("out_proj_add_ln", 0) == (n if fused else 0)
        assert out.dtype == torch.float32
        (out * dout).sum().backward()
        res[fused] = (out.detach(), t.grad, p.grad, {k: v.grad for k, v in model.named_parameters()})
    assert nerr(res[True][0], res[False][0]) < 2e-2
    assert nerr(res[True][1], res[False][1]) < 3e-2
    assert nerr(res[True][2], res[False][2]) < 3e-2
    for k, ga in res[True][3].items():
        gb = res[False][3][k]
        assert (ga is None) == (gb is None), k
        if ga is not None:
            assert nerr(ga, gb) < 4e-2, k
