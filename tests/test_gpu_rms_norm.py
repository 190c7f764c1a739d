"""GPU parity of rms_norm=True: the add + RMSNorm kernels (csrc/add_norm.hip, csrc/out_norm_bf16.hip with
SIMAMBA_NORM_RMS) forward and every gradient against a float64 restatement of mamba-ssm's rms_norm_ref; the *_ex
entry points with flags 0 against the plain ones (bitwise); MixerModel(rms_norm=True) against a float64 composition of
the reference's Block / MixerModel math, in fp32 and under bf16 autocast (route counters prove the fused RMS chain ran);
PointMamba, MAE and segmentation train steps with rms_norm=True, finite, and bitwise repeatable in deterministic mode."""
import copy

import pytest
import torch
import torch.nn.functional as F

from helpers import clouds, nerr
from oracle.scan_ref import selective_scan_ref
from si_mamba_amd import _lib

pytestmark = pytest.mark.gpu


def rms_norm_ref(x, weight, residual=None, eps=1e-6, prenorm=False):
    """mamba-ssm's rms_norm_ref (mamba_ssm/ops/triton/layernorm.py), in float64."""
    x = x.double()
    if residual is not None:
        x = x + residual.double()
    rstd = 1 / torch.sqrt(x.square().mean(dim=-1, keepdim=True) + eps)
    out = x * rstd * weight.double()
    return (out, x) if prenorm else out


# ---- add + RMSNorm kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 1024, 384), (3, 50, 128), (2, 7, 2048), (5, 1, 36), (1, 300, 512)])
@pytest.mark.parametrize("has_res,has_scale", [(True, True), (True, False), (False, False)])
@pytest.mark.parametrize("hdtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("odtype", [torch.float32, torch.bfloat16])
def test_add_rms_norm_matches_float64(shape, has_res, has_scale, hdtype, odtype, device):
    from si_mamba_amd.add_norm import add_rms_norm_fn
    B, L, d = shape
    g = torch.Generator().manual_seed(B * 1000 + d)
    hidden = torch.randn(B, L, d, generator=g).to(hdtype)
    residual = torch.randn(B, L, d, generator=g) if has_res else None
    w = 1.0 + 0.1 * torch.randn(d, generator=g)
    scale = (torch.rand(B, generator=g) > 0.3).float() / 0.7 if has_scale else None
    dn = torch.randn(B, L, d, generator=g)
    dr = torch.randn(B, L, d, generator=g)

    ref = [t.double().requires_grad_(True) if t is not None else None for t in (hidden, residual, w)]
    h = ref[0] if scale is None else ref[0] * scale.double()[:, None, None]
    wn, wr = rms_norm_ref(h, ref[2], ref[1], eps=1e-5, prenorm=True)
    ((wn * dn.double()).sum() + (wr * dr.double()).sum()).backward()

    dev = [t.to(device).clone().requires_grad_(True) if t is not None else None for t in (hidden, residual, w)]
    c0 = _lib.counters.get("add_rms_norm", 0)
    gn, gr = add_rms_norm_fn(dev[0], dev[1], dev[2], 1e-5, rowscale=None if scale is None else scale.to(device),
                             out_dtype=odtype)
    assert gn.dtype == odtype and gr.dtype == torch.float32
    ((gn.float() * dn.to(device)).sum() + (gr * dr.to(device)).sum()).backward()
    tol = 1e-3 if (hdtype == torch.float32 and odtype == torch.float32) else 1e-2
    assert nerr(gn, wn) < tol and nerr(gr, wr) < tol
    assert nerr(dev[0].grad, ref[0].grad) < tol
    if has_res:
        assert nerr(dev[1].grad, ref[1].grad) < tol
    assert nerr(dev[2].grad, ref[2].grad) < tol * 4
    assert _lib.counters.get("add_rms_norm", 0) == c0           # the op itself counts nothing; the model routes do


def _ln_case(B, L, d, hdtype, odtype, device, seed):
    g = torch.Generator().manual_seed(seed)
    t = dict(h=torch.randn(B, L, d, generator=g).to(hdtype), r=torch.randn(B, L, d, generator=g),
             s=(torch.rand(B, generator=g) > 0.3).float() / 0.7, w=1 + 0.1 * torch.randn(d, generator=g),
             b=0.1 * torch.randn(d, generator=g), dn=torch.randn(B, L, d, generator=g).to(odtype),
             dr=torch.randn(B, L, d, generator=g))
    return {k: v.to(device) for k, v in t.items()}


@pytest.mark.parametrize("hdtype,odtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                           (torch.float32, torch.bfloat16)])
def test_ex_with_flags_zero_is_bitwise_the_plain_entry_point(hdtype, odtype, device):
    lib = _lib.load()
    B, L, d = 4, 100, 384
    c = _ln_case(B, L, d, hdtype, odtype, device, seed=1)
    hc, oc = _lib.dtype_code(hdtype), _lib.dtype_code(odtype)
    st = _lib.stream_ptr(device)
    grid = lib.simamba_add_layer_norm_grid(B, L)
    outs = []
    for ex in (False, True):
        ro = torch.empty(B, L, d, device=device)
        nm = torch.empty(B, L, d, device=device, dtype=odtype)
        mean = torch.empty(B * L, device=device)
        rstd = torch.empty(B * L, device=device)
        dres = torch.empty(B, L, d, device=device)
        dhid = torch.empty(B, L, d, device=device, dtype=hdtype)
        part = torch.zeros(grid, 2, d, device=device)
        a = (c["h"].data_ptr(), c["r"].data_ptr(), c["s"].data_ptr(), c["w"].data_ptr(), c["b"].data_ptr(),
             ro.data_ptr(), nm.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, L, d, 1e-5, hc, oc)
        rc = lib.simamba_add_layer_norm_fwd_ex(*a, 0, st) if ex else lib.simamba_add_layer_norm_fwd(*a, st)
        assert rc == 0
        a = (c["dn"].data_ptr(), c["dr"].data_ptr(), ro.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
             c["w"].data_ptr(), c["s"].data_ptr(), dres.data_ptr(), dhid.data_ptr(), part.data_ptr(), B, L, d, hc, oc)
        rc = lib.simamba_add_layer_norm_bwd_ex(*a, 0, st) if ex else lib.simamba_add_layer_norm_bwd(*a, st)
        assert rc == 0
        torch.cuda.synchronize()
        outs.append((ro, nm, mean, rstd, dres, dhid, part))
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_out_proj_ex_with_flags_zero_is_bitwise_the_plain_entry_point(device):
    lib = _lib.load()
    B, C, L = 2, 384, 200
    c = _op_case(B, C, L, device, seed=3, residual=True, rowscale=True)
    beta = (0.1 * torch.randn(C, generator=torch.Generator().manual_seed(9))).to(device)
    wb = c["w"].bfloat16().contiguous()
    outs = []
    for ex in (False, True):
        ro = torch.empty(B, L, C, device=device)
        nm = torch.empty(B, L, C, device=device, dtype=torch.bfloat16)
        mean, rstd = torch.empty(B * L, device=device), torch.empty(B * L, device=device)
        a = (c["y"].data_ptr(), wb.data_ptr(), c["res"].data_ptr(), c["rs"].data_ptr(), c["gamma"].data_ptr(),
             beta.data_ptr(), ro.data_ptr(), nm.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, 2 * C, L, C, 1e-5,
             _lib.BF16)
        st = _lib.stream_ptr(device)
        rc = lib.simamba_out_proj_add_ln_fwd_ex(*a, 0, st) if ex else lib.simamba_out_proj_add_ln_fwd(*a, st)
        assert rc == 0
        torch.cuda.synchronize()
        outs.append((ro, nm, mean, rstd))
    for x, y in zip(*outs):
        assert torch.equal(x, y)


# ---- out_proj + add + RMSNorm kernel ---------------------------------------------------------------------------------
def _op_case(B, C, L, device, seed, residual=True, rowscale=False):
    g = torch.Generator().manual_seed(seed)
    K = 2 * C
    y = torch.randn(B, K, L, generator=g).bfloat16()
    w = torch.randn(C, K, generator=g) * K ** -0.5
    res = torch.randn(B, L, C, generator=g) if residual else None
    rs = (torch.rand(B, generator=g) > 0.3).float() / 0.7 if rowscale else None
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    dn = torch.randn(B, L, C, generator=g)
    dr = torch.randn(B, L, C, generator=g)
    mv = lambda t: None if t is None else t.to(device)
    return dict(y=mv(y), w=mv(w), res=mv(res), rs=mv(rs), gamma=mv(gamma), dn=mv(dn), dr=mv(dr))


def _op_want(c, out_dtype):
    """float64 with the roundings: bf16 operands, out_proj result rounded to bf16, fp32 residual stream."""
    y, w = c["y"].double().cpu(), c["w"].bfloat16().double().cpu()
    hid = torch.einsum("bkl,ck->blc", y, w).float().bfloat16().double()
    if c["res"] is not None:
        if c["rs"] is not None:
            hid = hid * c["rs"].double().cpu()[:, None, None]
        hid = hid + c["res"].double().cpu()
    res_out = hid.float()
    return rms_norm_ref(res_out, c["gamma"].cpu(), eps=1e-5).to(out_dtype), res_out


@pytest.mark.parametrize("B,C,L", [(2, 128, 64), (1, 256, 200), (2, 384, 128), (1, 384, 1024), (3, 384, 72), (2, 256, 136)])
@pytest.mark.parametrize("flags", [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
def test_out_proj_add_rms_forward(B, C, L, flags, out_dtype, device):
    from si_mamba_amd.out_norm import out_proj_add_ln_fn
    residual, rowscale = flags
    c = _op_case(B, C, L, device, seed=C + L, residual=residual, rowscale=rowscale)
    normed, res_out = out_proj_add_ln_fn(c["y"], c["w"], c["res"], c["gamma"], None, 1e-5, c["rs"], out_dtype, rms=True)
    wn, wr = _op_want(c, out_dtype)
    assert normed.dtype == out_dtype and res_out.dtype == torch.float32
    assert nerr(res_out, wr) < 1e-2
    assert ((res_out.cpu() - wr).abs() > 1e-6).float().mean() < 2e-2
    assert nerr(normed, wn) < (1e-2 if out_dtype == torch.bfloat16 else 5e-3)


@pytest.mark.parametrize("B,C,L", [(2, 384, 128), (1, 128, 64)])
def test_out_proj_add_rms_matches_unfused_route_and_backward(B, C, L, device):
    from si_mamba_amd.add_norm import add_rms_norm_fn
    from si_mamba_amd.out_norm import out_proj_add_ln_fn
    c = _op_case(B, C, L, device, seed=7, residual=True, rowscale=True)
    outs = {}
    for fused in (True, False):
        y = c["y"].clone().requires_grad_(True)
        w = c["w"].clone().requires_grad_(True)
        res = c["res"].clone().requires_grad_(True)
        gamma = c["gamma"].clone().requires_grad_(True)
        if fused:
            normed, res_out = out_proj_add_ln_fn(y, w, res, gamma, None, 1e-5, c["rs"], torch.bfloat16, rms=True)
        else:
            hid = torch.bmm(y.transpose(1, 2), w.bfloat16().t().unsqueeze(0).expand(B, -1, -1))
            normed, res_out = add_rms_norm_fn(hid, res, gamma, 1e-5, rowscale=c["rs"], out_dtype=torch.bfloat16)
        ((normed.float() * c["dn"]).sum() + (res_out * c["dr"]).sum()).backward()
        outs[fused] = (normed.detach(), res_out.detach(), y.grad, w.grad, res.grad, gamma.grad)
    for n, a, b_ in zip(("normed", "res_out", "dy", "dw", "dres", "dgamma"), outs[True], outs[False]):
        assert nerr(a, b_) < 1e-2, n
    # the fused backward against float64 as well (gradient of the RMS part w.r.t. the residual stream and gamma)
    wn, wr = _op_want(c, torch.float64)
    assert nerr(outs[True][0], wn) < 1e-2


# ---- MixerModel(rms_norm=True) against a float64 composition -----------------------------------------------------------
def _mixer64(p, h):
    """Upstream Mamba.forward (mamba_inner_ref order of ops) in float64; p: the mixer's parameters as float64 leaves."""
    Bsz, L, _ = h.shape
    xz = (h @ p["in_proj.weight"].t()).transpose(1, 2)
    x, z = xz.chunk(2, dim=1)
    D = x.shape[1]
    x = F.silu(F.conv1d(x, p["conv1d.weight"], p["conv1d.bias"], padding=3, groups=D)[..., :L])
    xdbl = x.transpose(1, 2) @ p["x_proj.weight"].t()
    R = p["dt_proj.weight"].shape[1]
    N = (xdbl.shape[-1] - R) // 2
    dt, Bm, Cm = torch.split(xdbl, [R, N, N], dim=-1)
    delta = (dt @ p["dt_proj.weight"].t()).transpose(1, 2)
    y = selective_scan_ref(x, delta, -torch.exp(p["A_log"]), Bm.transpose(1, 2), Cm.transpose(1, 2), p["D"], z=z,
                           delta_bias=p["dt_proj.bias"], delta_softplus=True, acc_dtype=torch.float64)
    return y.transpose(1, 2) @ p["out_proj.weight"].t()


def _stack64(model, x, pos):
    """reference MixerModel.forward / Block.forward (no DropPath) with rms_norm_ref norms, float64 leaves for every
    parameter: -> (out, leaves {name: tensor})."""
    leaves = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.named_parameters()}
    h, res = x + pos, None
    for i, layer in enumerate(model.layers):
        res = h if res is None else h + res
        hn = rms_norm_ref(res, leaves[f"layers.{i}.norm.weight"], eps=layer.norm.eps)
        p = {k[len(f"layers.{i}.mixer."):]: v for k, v in leaves.items() if k.startswith(f"layers.{i}.mixer.")}
        h = _mixer64(p, hn)
    return rms_norm_ref(h + res, leaves["norm_f.weight"], eps=model.norm_f.eps), leaves


@pytest.mark.parametrize("amp", [False, True])
def test_mixer_model_rms_matches_float64_composition(amp, device):
    from si_mamba_amd import RMSNorm
    from si_mamba_amd.block import MixerModel
    torch.manual_seed(3)
    B, L, d, n = 2, 64, 128, 3
    model = MixerModel(d, n, rms_norm=True, drop_path=0.).to(device).train()
    assert type(model.norm_f) is RMSNorm
    with torch.no_grad():                               # weights away from 1 so that dweight is exercised
        for layer in model.layers:
            layer.norm.weight.add_(0.1 * torch.randn(d, device=device))
        model.norm_f.weight.add_(0.1 * torch.randn(d, device=device))
    g = torch.Generator().manual_seed(11)
    x, pos = torch.randn(B, L, d, generator=g), torch.randn(B, L, d, generator=g)
    dout = torch.randn(B, L, d, generator=g)
    xd, pd = x.to(device).requires_grad_(True), pos.to(device).requires_grad_(True)
    c0 = dict(_lib.counters)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        out = model(xd, pd)
    (out.float() * dout.to(device)).sum().backward()
    dc = {k: _lib.counters.get(k, 0) - c0.get(k, 0) for k in ("add_rms_norm", "out_proj_add_rms", "out_proj_add_ln")}
    if amp:                                             # the fused bf16 chain: add + RMS, then n fused boundaries
        assert dc == {"add_rms_norm": 1, "out_proj_add_rms": n, "out_proj_add_ln": 0}, dc
    else:                                               # op by op: n block norms + norm_f through the add + RMS kernel
        assert dc == {"add_rms_norm": n + 1, "out_proj_add_rms": 0, "out_proj_add_ln": 0}, dc
    assert out.dtype == torch.float32
    x64, p64 = x.double().requires_grad_(True), pos.double().requires_grad_(True)
    want, leaves = _stack64(model, x64, p64)
    (want * dout.double()).sum().backward()
    # bf16 autocast: every block rounds its activations to bf16 on the way through, the restatement does not
    tol_o, tol_g, tol_p = (1e-3, 2e-3, 2e-3) if not amp else (3e-2, 5e-2, 8e-2)
    assert nerr(out, want) < tol_o
    assert nerr(xd.grad, x64.grad) < tol_g and nerr(pd.grad, p64.grad) < tol_g
    for k, v in model.named_parameters():
        assert v.grad is not None, k
        assert nerr(v.grad, leaves[k].grad) < tol_p, (k, nerr(v.grad, leaves[k].grad))


# ---- train steps with rms_norm=True --------------------------------------------------------------------------------------
def _step(which, device):
    """-> (model, loss_fn) at small sizes with rms_norm=True"""
    torch.manual_seed(0)
    if which == "pointmamba":
        from si_mamba_amd.point_mamba import PointMamba, default_config
        m = PointMamba(default_config(rms_norm=True, depth=4, num_group=64)).to(device).train()
        pts = clouds(8, 1024, 1).to(device)
        gt = torch.randint(0, 15, (8,), generator=torch.Generator().manual_seed(2)).to(device)
        return m, lambda: m.get_loss_acc(m(pts), gt)[0]
    if which == "mae":
        from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
        m = Point_MAE_Mamba(default_mae_config(rms_norm=True, trans_dim=128, encoder_dims=128, depth=2,
                                               decoder_depth=1)).to(device).train()
        pts = clouds(4, 1024, 2).to(device)
        return m, lambda: m(pts)
    from si_mamba_amd.seg import PartSegMamba, default_seg_config, get_loss
    m = PartSegMamba(50, default_seg_config(rms_norm=True, trans_dim=128, depth=4, fetch_idx=(1, 2, 3))).to(device)
    m.train()
    B, N = 2, 2048
    pts = clouds(B, N, 5).transpose(1, 2).contiguous().to(device)
    label = F.one_hot(torch.tensor([0, 3]), 16).float().to(device)
    target = torch.randint(0, 50, (B, N), generator=torch.Generator().manual_seed(3)).to(device)
    crit = get_loss()
    return m, lambda: crit(m(pts, label).reshape(-1, 50), target.view(-1))


def _grads(m):
    return [None if p.grad is None else p.grad.clone() for p in m.parameters()]


@pytest.mark.parametrize("which", ["pointmamba", "mae", "partseg"])
@pytest.mark.parametrize("amp", [False, True])
def test_rms_train_step_finite(which, amp, device):
    from si_mamba_amd import RMSNorm
    m, loss_fn = _step(which, device)
    assert any(type(mod) is RMSNorm for mod in m.modules())
    c0 = _lib.counters.get("add_rms_norm", 0)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        loss = loss_fn()
    loss.backward()
    assert torch.isfinite(loss)
    assert _lib.counters.get("add_rms_norm", 0) > c0
    bad = [k for k, p in m.named_parameters()
           if not k.startswith("decoder_pos_embed.") and (p.grad is None or not torch.isfinite(p.grad).all())]
    assert not bad, bad
    for mod in m.modules():
        if type(mod) is RMSNorm:
            assert mod.bias is None and mod.weight.grad is not None


@pytest.mark.parametrize("which,amp", [("pointmamba", False), ("pointmamba", True), ("mae", True), ("partseg", False)])
def test_rms_train_step_bitwise_repeatable_in_deterministic_mode(which, amp, device):
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        m, loss_fn = _step(which, device)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.05)
        s0 = (copy.deepcopy(m.state_dict()), copy.deepcopy(opt.state_dict()))
        res = []
        with _lib.deterministic(True):
            for _ in range(2):
                m.load_state_dict(s0[0])
                opt.load_state_dict(s0[1])
                opt.zero_grad(set_to_none=True)
                torch.manual_seed(1234)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                    loss = loss_fn()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(m.parameters(), 10.0)
                opt.step()
                torch.cuda.synchronize()
                res.append((loss.detach().clone(), _grads(m), [p.detach().clone() for p in m.parameters()]))
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=prev_warn)
    (l0, g0, p0), (l1, g1, p1) = res
    assert torch.equal(l0, l1)
    for i, (a, b) in enumerate(zip(g0 + p0, g1 + p1)):
        assert (a is None) == (b is None), i
        if a is not None:
            assert torch.equal(a, b), i
