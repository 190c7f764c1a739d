"""GPU: the deterministic backward (SIMAMBA_BWD_DETERMINISTIC; _lib.deterministic / torch.use_deterministic_algorithms).

Every repeat-run comparison is bitwise (torch.equal).  Against the atomic route and the float64 oracle the tolerances
of test_gpu_scan.py / test_gpu_conv.py apply.  Tests that switch torch's global flag restore it (fixture below)."""
import copy

import pytest
import torch

from helpers import clouds, nerr
from oracle import scan_ref
from si_mamba_amd import _lib

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2}
GRADS = ("u", "delta", "A", "B", "C", "D", "z", "delta_bias")


@pytest.fixture
def torch_deterministic():
    """torch.use_deterministic_algorithms(True) for one test, restored afterwards whatever happens."""
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=prev_warn)
        _lib.set_deterministic(None)


def _scan_inputs(B, D, L, N, dtype, device, z=True, Dp=True, bias=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = dict(u=torch.randn(B, D, L, generator=g), delta=0.5 * torch.randn(B, D, L, generator=g),
             A=-torch.rand(D, N, generator=g) - 0.5, B=torch.randn(B, N, L, generator=g),
             C=torch.randn(B, N, L, generator=g), D=torch.randn(D, generator=g) if Dp else None,
             z=torch.randn(B, D, L, generator=g) if z else None,
             delta_bias=0.1 * torch.randn(D, generator=g) if bias else None)
    dout = torch.randn(B, D, L, generator=g)
    act = ("u", "delta", "z", "B", "C")
    dev = {k: None if v is None else v.to(device).to(dtype if k in act else torch.float32).requires_grad_(True)
           for k, v in t.items()}
    return t, dev, dout.to(device).to(dtype)


def _scan_grads(t, dout, ckpt, runs):
    """forward once, then `runs` backwards of the same graph: a list of {name: grad}"""
    from si_mamba_amd import selective_scan_fn
    with _lib.scan_ckpt(ckpt):
        out = selective_scan_fn(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["delta_bias"],
                                delta_softplus=True)
    names = [k for k in GRADS if t[k] is not None]
    res = []
    for _ in range(runs):
        gs = torch.autograd.grad(out, [t[k] for k in names], dout, retain_graph=True)
        res.append(dict(zip(names, gs)))
    torch.cuda.synchronize()
    return res


def _assert_bitwise(runs):
    for r in runs[1:]:
        for k in runs[0]:
            assert torch.equal(runs[0][k], r[k]), k


SCAN_CASES = [
    # sequential kernel (16-step checkpoints) at the model shape
    (64, 768, 1024, 16, torch.float32, _lib.CKPT_SEQ, (True, True, True)),
    (64, 768, 1024, 16, torch.bfloat16, _lib.CKPT_SEQ, (True, True, True)),
    (64, 768, 1024, 16, torch.float32, _lib.CKPT_SEQ, (False, False, False)),
    # row scan (128-step chunks): configs 4 / 5 and small batches, a ragged shape
    (16, 768, 1024, 16, torch.float32, _lib.CKPT_ROW, (True, True, True)),
    (16, 768, 1024, 16, torch.bfloat16, _lib.CKPT_ROW, (False, True, False)),
    (3, 200, 301, 8, torch.float32, _lib.CKPT_ROW, (True, True, True)),
    (3, 200, 301, 8, torch.float32, _lib.CKPT_ROW, (False, False, False)),
]


@pytest.mark.parametrize("B,D,L,N,dtype,ckpt,opt", SCAN_CASES)
def test_scan_bwd_bitwise_repeatable_and_close_to_atomic(B, D, L, N, dtype, ckpt, opt, device):
    _, t, dout = _scan_inputs(B, D, L, N, dtype, device, *opt)
    c0 = dict(_lib.counters)
    with _lib.deterministic(True):
        det = _scan_grads(t, dout, ckpt, 3)
    assert _lib.counters.get("scan_bwd_det", 0) - c0.get("scan_bwd_det", 0) == 3
    assert _lib.counters.get("scan_bwd_atomic", 0) == c0.get("scan_bwd_atomic", 0)
    _assert_bitwise(det)
    with _lib.deterministic(False):
        ato = _scan_grads(t, dout, ckpt, 1)[0]
    assert _lib.counters.get("scan_bwd_atomic", 0) - c0.get("scan_bwd_atomic", 0) == 1
    for k in det[0]:
        assert nerr(det[0][k], ato[k]) < TOL[dtype], k


@pytest.mark.parametrize("ckpt", [_lib.CKPT_SEQ, _lib.CKPT_ROW])
def test_scan_bwd_deterministic_matches_float64_oracle(ckpt, device):
    cpu, t, dout = _scan_inputs(2, 64, 80, 16, torch.float32, device, seed=3)
    with _lib.deterministic(True):
        got = _scan_grads(t, dout, ckpt, 1)[0]
    c = {k: None if v is None else v.double().requires_grad_(True) for k, v in cpu.items()}
    out = scan_ref.selective_scan_ref(c["u"], c["delta"], c["A"], c["B"], c["C"], c["D"], c["z"], c["delta_bias"],
                                      delta_softplus=True)
    out.backward(dout.double().cpu())
    for k in got:
        assert nerr(got[k], c[k].grad) < 1e-3, k


def test_dt_scan_bwd_bitwise_repeatable(device):
    """The bf16 mixer's form (delta formed inside the scans, simamba_selective_scan_dt_bwd_ex) at the model shape:
    the whole mixer backward, three times."""
    from si_mamba_amd.mamba_inner import mamba_inner_fn
    torch.manual_seed(0)
    B, D, L, N, R = 64, 768, 1024, 16, 24
    xz = torch.randn(B, 2 * D, L, device=device).to(torch.bfloat16).requires_grad_(True)
    p = dict(cw=0.3 * torch.randn(D, 4, device=device), cb=0.1 * torch.randn(D, device=device),
             xw=0.05 * torch.randn(R + 2 * N, D, device=device), dtw=0.2 * torch.randn(D, R, device=device),
             A=-torch.rand(D, N, device=device) - 0.5, Dp=torch.randn(D, device=device),
             bias=0.1 * torch.randn(D, device=device))
    p = {k: v.requires_grad_(True) for k, v in p.items()}
    c0 = dict(_lib.counters)
    with _lib.deterministic(True):
        y = mamba_inner_fn(xz, p["cw"], p["cb"], p["xw"], p["dtw"], None, None, p["A"], p["Dp"], p["bias"])
        assert _lib.counters.get("scan_dt_fwd", 0) > c0.get("scan_dt_fwd", 0)
        dy = torch.randn_like(y)
        ins = [xz] + list(p.values())
        runs = [dict(enumerate(torch.autograd.grad(y, ins, dy, retain_graph=True))) for _ in range(3)]
    assert _lib.counters.get("scan_bwd_atomic", 0) == c0.get("scan_bwd_atomic", 0)
    assert _lib.counters.get("conv1d_bwd_atomic", 0) == c0.get("conv1d_bwd_atomic", 0)
    _assert_bitwise(runs)
    with _lib.deterministic(False):
        ato = dict(enumerate(torch.autograd.grad(y, ins, dy)))
    for k in ato:
        assert nerr(runs[0][k], ato[k]) < 4 * TOL[torch.bfloat16], k


@pytest.mark.parametrize("width", [2, 3, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,D,L", [(8, 96, 1024), (3, 40, 301)])      # the fast (aligned) and the general kernel
def test_conv1d_bwd_bitwise_repeatable_and_close_to_atomic(B, D, L, width, dtype, device):
    from si_mamba_amd import causal_conv1d_fn
    g = torch.Generator().manual_seed(width)
    x = torch.randn(B, D, L, generator=g).to(device).to(dtype).requires_grad_(True)
    w = (0.3 * torch.randn(D, width, generator=g)).to(device).requires_grad_(True)
    b = (0.1 * torch.randn(D, generator=g)).to(device).requires_grad_(True)
    dout = torch.randn(B, D, L, generator=g).to(device).to(dtype)
    out = causal_conv1d_fn(x, w, b, "silu")
    c0 = dict(_lib.counters)
    with _lib.deterministic(True):
        runs = [dict(zip("xwb", torch.autograd.grad(out, [x, w, b], dout, retain_graph=True))) for _ in range(3)]
    assert _lib.counters.get("conv1d_bwd_det", 0) - c0.get("conv1d_bwd_det", 0) == 3
    _assert_bitwise(runs)
    with _lib.deterministic(False):
        ato = dict(zip("xwb", torch.autograd.grad(out, [x, w, b], dout)))
    assert _lib.counters.get("conv1d_bwd_atomic", 0) - c0.get("conv1d_bwd_atomic", 0) == 1
    tol = 1e-3 if dtype == torch.float32 else 1e-2
    assert torch.equal(runs[0]["x"], ato["x"])                     # dx never went through an atomic
    assert nerr(runs[0]["w"], ato["w"]) < tol and nerr(runs[0]["b"], ato["b"]) < tol


def test_switch_follows_torch_unless_overridden():
    prev = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        assert not _lib.deterministic_enabled()
        torch.use_deterministic_algorithms(True)
        assert _lib.deterministic_enabled()
        with _lib.deterministic(False):
            assert not _lib.deterministic_enabled()
        _lib.set_deterministic(True)
        torch.use_deterministic_algorithms(False)
        assert _lib.deterministic_enabled()
        _lib.set_deterministic(None)
        assert not _lib.deterministic_enabled()
        torch.backends.cudnn.deterministic, was = True, torch.backends.cudnn.deterministic
        try:
            assert not _lib.deterministic_enabled()                # not keyed on cuDNN's flag
        finally:
            torch.backends.cudnn.deterministic = was
    finally:
        torch.use_deterministic_algorithms(prev)
        _lib.set_deterministic(None)
    import si_mamba_amd
    assert si_mamba_amd.deterministic is _lib.deterministic and si_mamba_amd.set_deterministic is _lib.set_deterministic


def _grads(m):
    return [None if p.grad is None else p.grad.clone() for p in m.parameters()]


def _equal_lists(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), i
        if x is not None:
            assert torch.equal(x, y), i


@pytest.mark.parametrize("stack", [False, True])
def test_mamba_and_mixer_under_torch_flag(stack, torch_deterministic, device):
    from si_mamba_amd import Mamba
    from si_mamba_amd.block import MixerModel
    torch.manual_seed(0)
    m = (MixerModel(d_model=128, n_layer=3, drop_path=0.) if stack else Mamba(128)).to(device).train()
    x = torch.randn(16, 256, 128, device=device)
    pos = torch.randn(16, 256, 128, device=device)
    c0 = dict(_lib.counters)
    out = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        y = m(x, pos) if stack else m(x)
        (y.float() ** 2).mean().backward()
        out.append(_grads(m))
    torch.cuda.synchronize()
    _equal_lists(out[0], out[1])
    assert _lib.counters.get("scan_bwd_det", 0) > c0.get("scan_bwd_det", 0)
    assert _lib.counters.get("scan_bwd_atomic", 0) == c0.get("scan_bwd_atomic", 0)
    assert _lib.counters.get("conv1d_bwd_atomic", 0) == c0.get("conv1d_bwd_atomic", 0)


def test_default_route_unchanged(device):
    """Mode off (torch's flag off, no override): the atomic routes run."""
    from si_mamba_amd import Mamba
    assert not torch.are_deterministic_algorithms_enabled() and not _lib.deterministic_enabled()
    torch.manual_seed(0)
    m = Mamba(128).to(device)
    c0 = dict(_lib.counters)
    m(torch.randn(4, 64, 128, device=device)).sum().backward()
    assert _lib.counters.get("scan_bwd_atomic", 0) > c0.get("scan_bwd_atomic", 0)
    assert _lib.counters.get("conv1d_bwd_atomic", 0) > c0.get("conv1d_bwd_atomic", 0)
    assert _lib.counters.get("scan_bwd_det", 0) == c0.get("scan_bwd_det", 0)


# ---- end to end: one seeded training step, twice from the same state ---------------------------------------------
def _state(m, opt):
    return copy.deepcopy(m.state_dict()), copy.deepcopy(opt.state_dict())


def _twice(m, opt, loss_fn, amp):
    """run the seeded step twice from the same state; return (grads, params, buffers) of each run"""
    s0 = _state(m, opt)
    res = []
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
        res.append((_grads(m), [p.detach().clone() for p in m.parameters()],
                    [b.detach().clone() for b in m.buffers()], loss.detach().clone()))
    return res


def _assert_same_step(res):
    (g0, p0, b0, l0), (g1, p1, b1, l1) = res
    assert torch.equal(l0, l1)
    _equal_lists(g0, g1)
    _equal_lists(p0, p1)
    _equal_lists(b0, b1)


@pytest.mark.parametrize("amp", [False, True])
def test_pointmamba_finetune_step_bitwise(amp, torch_deterministic, device):
    """The bench step (B = 64, 1024 points, 12 blocks, AdamW, clip): forward, loss, backward, clip, update."""
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    m = PointMamba(default_config()).to(device).train()
    opt = torch.optim.AdamW(m.parameters(), lr=5e-4, weight_decay=0.05)
    pts = clouds(64, 1024, 1).to(device)
    gt = torch.randint(0, 15, (64,), generator=torch.Generator().manual_seed(2)).to(device)
    c0 = dict(_lib.counters)
    res = _twice(m, opt, lambda: m.get_loss_acc(m(pts), gt)[0], amp)
    _assert_same_step(res)
    assert _lib.counters.get("scan_bwd_det", 0) - c0.get("scan_bwd_det", 0) >= 2 * 12
    assert _lib.counters.get("scan_bwd_atomic", 0) == c0.get("scan_bwd_atomic", 0)


def test_mae_step_bitwise(torch_deterministic, device):
    from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
    torch.manual_seed(0)
    m = Point_MAE_Mamba(default_mae_config(trans_dim=96, encoder_dims=96, depth=2, decoder_depth=1)).to(device).train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.05)
    pts = clouds(4, 1024, 2).to(device)
    _assert_same_step(_twice(m, opt, lambda: m(pts), True))


def test_partseg_step_bitwise(torch_deterministic, device):
    from si_mamba_amd.seg import PartSegMamba, get_loss
    torch.manual_seed(0)
    m = PartSegMamba(50).to(device).train()
    B, N = 2, 2048
    pts = clouds(B, N, 5).transpose(1, 2).contiguous().to(device)
    label = torch.nn.functional.one_hot(torch.tensor([0, 3]), 16).float().to(device)
    target = torch.randint(0, 50, (B, N), generator=torch.Generator().manual_seed(3)).to(device)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.05)
    crit = get_loss()
    _assert_same_step(_twice(m, opt, lambda: crit(m(pts, label).reshape(-1, 50), target.view(-1)), False))


def test_graphed_train_step_deterministic(torch_deterministic, device):
    """GraphedTrainStep under torch's switch (the library GEMMs need it too; the library's own mode alone leaves their
    last bits free): two replays from the same restored state are bitwise equal."""
    from si_mamba_amd.graphed import GraphedTrainStep
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    cfg = default_config(trans_dim=64, encoder_dims=64, depth=2, num_group=32, group_size=16, cls_dim=5,
                         drop_path=0., knn_graph=8)
    m = PointMamba(cfg).to(device).train()
    for mod in m.modules():             # every replay draws fresh Philox offsets: a dropout mask would differ by design
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, capturable=True)
    pts = clouds(8, 256, 20).to(device)
    gt = torch.randint(0, 5, (8,), generator=torch.Generator().manual_seed(0)).to(device)
    c0 = dict(_lib.counters)
    step = GraphedTrainStep(lambda p, y: m.get_loss_acc(m(p), y)[0], opt, (pts, gt), clip=10.0, warmup=3)
    assert _lib.counters.get("scan_bwd_det", 0) > c0.get("scan_bwd_det", 0)
    assert _lib.counters.get("scan_bwd_atomic", 0) == c0.get("scan_bwd_atomic", 0)
    params, bufs = list(m.parameters()), list(m.buffers())
    snap_p = [p.detach().clone() for p in params]
    snap_b = [b.detach().clone() for b in bufs]                  # BatchNorm running stats and batch counters
    snap_s = {id(p): {k: v.clone() for k, v in opt.state[p].items() if torch.is_tensor(v)} for p in params}
    res = []
    for _ in range(2):
        with torch.no_grad():
            for p, s in zip(params, snap_p):
                p.copy_(s)
            for b, s in zip(bufs, snap_b):
                b.copy_(s)
            for p in params:
                for k, v in snap_s[id(p)].items():
                    opt.state[p][k].copy_(v)
        loss = step(pts, gt).clone()
        torch.cuda.synchronize()
        res.append((_grads(m), [p.detach().clone() for p in params], [b.detach().clone() for b in m.buffers()], loss))
    _assert_same_step(res)
