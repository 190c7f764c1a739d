"""CPU: rms_norm=True (reference models/point_mamba.py:164, :227; part_segmentation/models/pt_mamba.py:134, :277) --
the RMSNorm module and its state-dict contract, the models built with it at reference sizes, its CPU formula against
a float64 restatement of mamba-ssm's rms_norm_ref, and the C ABI of the norm flags (validation before any launch)."""
import ctypes
import re

import pytest
import torch

from si_mamba_amd import _lib


def rms_norm_ref(x, weight, residual=None, eps=1e-6, prenorm=False):
    """mamba-ssm's rms_norm_ref (mamba_ssm/ops/triton/layernorm.py), restated in float64."""
    x = x.double()
    if residual is not None:
        x = x + residual.double()
    rstd = 1 / torch.sqrt(x.square().mean(dim=-1, keepdim=True) + eps)
    out = x * rstd * weight.double()
    return (out, x) if prenorm else out


def test_rmsnorm_exported_and_state_dict():
    import si_mamba_amd
    from si_mamba_amd import RMSNorm
    assert "RMSNorm" in si_mamba_amd.__all__ and si_mamba_amd.RMSNorm is RMSNorm
    n = RMSNorm(48, eps=1e-6)
    assert n.eps == 1e-6 and n.bias is None and torch.equal(n.weight.detach(), torch.ones(48))
    assert list(n.state_dict()) == ["weight"]


def test_create_block_rms_norm():
    from si_mamba_amd import RMSNorm
    from si_mamba_amd.block import _init_weights, create_block
    blk = create_block(64, rms_norm=True, norm_epsilon=1e-6, layer_idx=0)
    n = blk.norm
    assert type(n) is RMSNorm and n.eps == 1e-6 and n.bias is None
    assert torch.equal(n.weight.detach(), torch.ones(64))
    sd = blk.state_dict()
    assert "norm.weight" in sd and "norm.bias" not in sd
    with torch.no_grad():
        n.weight.fill_(3.0)
    blk.apply(lambda m: _init_weights(m, n_layer=4))
    assert torch.equal(n.weight.detach(), torch.full((64,), 3.0))          # _init_weights leaves it alone
    assert type(create_block(64, layer_idx=0).norm) is torch.nn.LayerNorm     # the default is unchanged


def test_mixer_model_norm_f_follows_rms_norm():
    from si_mamba_amd import RMSNorm
    from si_mamba_amd.block import MixerModel
    mm = MixerModel(d_model=64, n_layer=2, rms_norm=True, norm_epsilon=1e-6, drop_path=0.)
    assert type(mm.norm_f) is RMSNorm and mm.norm_f.eps == 1e-6
    assert all(type(layer.norm) is RMSNorm for layer in mm.layers)
    assert type(MixerModel(d_model=64, n_layer=2, drop_path=0.).norm_f) is torch.nn.LayerNorm


@pytest.mark.parametrize("rms_norm", [False, True])
def test_segmentation_stack_is_the_mixer_models_construction(rms_norm):
    """After the same seed the two stacks hold the same state dict: same keys in the same order, equal tensors (one
    constructor, one order of draws from the generator)."""
    from si_mamba_amd.block import MixerModel
    from si_mamba_amd.seg import MixerModelForSegmentation
    torch.manual_seed(0)
    a = MixerModel(64, 3, drop_path=0.1, rms_norm=rms_norm).state_dict()
    torch.manual_seed(0)
    b = MixerModelForSegmentation(64, 3, drop_path=0.1, rms_norm=rms_norm).state_dict()
    assert list(a) == list(b)
    assert all(k.startswith(("layers.", "norm_f.")) for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), k


_NORM_BIAS = re.compile(r"(^|\.)blocks\.(layers\.\d+\.norm|norm_f)\.bias$")


def _key_sets(build):
    torch.manual_seed(0)
    ln = set(build(False).state_dict())
    torch.manual_seed(0)
    rms = set(build(True).state_dict())
    return ln, rms


@pytest.mark.parametrize("which", ["pointmamba", "mae", "partseg"])
def test_models_at_reference_sizes_drop_only_the_norm_biases(which):
    if which == "pointmamba":
        from si_mamba_amd.point_mamba import PointMamba, default_config
        build = lambda rms: PointMamba(default_config(rms_norm=rms))
        n_blocks = 12
    elif which == "mae":
        from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
        build = lambda rms: Point_MAE_Mamba(default_mae_config(rms_norm=rms))
        n_blocks = 12 + 4
    else:
        from si_mamba_amd.seg import PartSegMamba, default_seg_config
        build = lambda rms: PartSegMamba(50, default_seg_config(rms_norm=rms))
        n_blocks = 12
    ln, rms = _key_sets(build)
    dropped = {k for k in ln if _NORM_BIAS.search(k)}
    n_stacks = 2 if which == "mae" else 1
    assert len(dropped) == n_blocks + n_stacks
    assert rms == ln - dropped
    # the head norms stay nn.LayerNorm, as in the reference
    assert any(k.endswith("norm.bias") and not _NORM_BIAS.search(k) for k in rms)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("prenorm", [False, True])
def test_rmsnorm_cpu_matches_float64(dtype, with_res, prenorm):
    from si_mamba_amd import RMSNorm
    g = torch.Generator().manual_seed(5)
    n = RMSNorm(40, eps=1e-6)
    with torch.no_grad():
        n.weight.copy_(1 + 0.1 * torch.randn(40, generator=g))
    x = (3 * torch.randn(2, 7, 40, generator=g)).to(dtype)
    res = torch.randn(2, 7, 40, generator=g) if with_res else None
    got = n(x, residual=res, prenorm=prenorm)
    want = rms_norm_ref(x, n.weight.detach(), res, eps=1e-6, prenorm=prenorm)
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    if prenorm:
        (got, got_res), (want, want_res) = got, want
        assert got_res.dtype == (torch.float32 if with_res else dtype)
        assert (got_res.double() - want_res).abs().max() <= tol * want_res.abs().max()
    assert got.dtype == dtype and got.shape == x.shape
    assert (got.double() - want).abs().max() <= tol * want.abs().max()
    # residual_in_fp32: the residual stream comes back in fp32 whatever the input dtype
    _, r32 = n(x, residual=res, prenorm=True, residual_in_fp32=True)
    assert r32.dtype == torch.float32


def test_rmsnorm_cpu_gradients_match_float64():
    from si_mamba_amd import RMSNorm
    g = torch.Generator().manual_seed(6)
    n = RMSNorm(32)
    with torch.no_grad():
        n.weight.copy_(1 + 0.1 * torch.randn(32, generator=g))
    x = torch.randn(3, 5, 32, generator=g).requires_grad_(True)
    r = torch.randn(3, 5, 32, generator=g).requires_grad_(True)
    dy = torch.randn(3, 5, 32, generator=g)
    (n(x, residual=r) * dy).sum().backward()
    x64, r64 = x.detach().double().requires_grad_(True), r.detach().double().requires_grad_(True)
    w64 = n.weight.detach().double().requires_grad_(True)
    (rms_norm_ref(x64, w64, r64, eps=1e-5) * dy.double()).sum().backward()
    for got, want in ((x.grad, x64.grad), (r.grad, r64.grad), (n.weight.grad, w64.grad)):
        assert (got.double() - want).abs().max() <= 1e-5 * max(1.0, want.abs().max().item())


def test_ex_symbols_flags_and_error_codes():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("simamba_add_layer_norm_fwd_ex", "simamba_add_layer_norm_bwd_ex", "simamba_out_proj_add_ln_fwd_ex"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.NORM_RMS == 1
    lib = _lib.load()
    assert lib.simamba_abi_version() == 9
    assert b"bias" in lib.simamba_strerror(-10)
    assert b"flag" in lib.simamba_strerror(-9) and b"variant" in lib.simamba_strerror(-9)
    one = ctypes.c_void_p(16)               # never dereferenced: every call below fails validation first
    n = None
    RMS = _lib.NORM_RMS

    def fwd(flags, bias, mean=one, batch=2):
        return lib.simamba_add_layer_norm_fwd_ex(one, n, n, one, bias, one, one, mean, one, batch, 8, 64, 1e-5, 0, 0,
                                                 flags, n)

    def bwd(flags, mean=one):
        return lib.simamba_add_layer_norm_bwd_ex(one, n, one, mean, one, one, n, one, n, one, 2, 8, 64, 0, 0, flags, n)

    def onp(flags, beta, mean=one):
        return lib.simamba_out_proj_add_ln_fwd_ex(one, one, n, n, one, beta, one, one, mean, one, 2, 256, 64, 128,
                                                  1e-5, 0, flags, n)

    assert fwd(2, n) == -9 and fwd(RMS | 4, n) == -9 and fwd(-1, n) == -9          # unknown flag bits
    assert fwd(RMS, one) == -10                                                      # RMSNorm has no bias
    assert bwd(2) == -9 and bwd(RMS | 2) == -9
    assert onp(2, n) == -9 and onp(RMS, one) == -10
    # flag checks come first; the plain errors keep their codes
    assert lib.simamba_add_layer_norm_fwd_ex(one, n, n, one, n, one, one, one, one, 2, 8, 66, 1e-5, 0, 0, RMS, n) == -2
    assert fwd(0, n, mean=n) == -1                                                   # LayerNorm needs mean
    assert bwd(0, mean=n) == -1
    assert onp(0, n, mean=n) == -1
    assert fwd(RMS, n, mean=n, batch=0) == 0                                         # RMS: mean may be NULL
    # the plain entry points are the flags == 0 forms
    assert lib.simamba_add_layer_norm_fwd(one, n, n, one, n, one, one, n, one, 2, 8, 64, 1e-5, 0, 0, n) == -1


def test_add_norm_functions_refuse_a_bias_with_rms():
    from si_mamba_amd.add_norm import add_layer_norm_fn
    from si_mamba_amd.out_norm import out_proj_add_ln_fn
    t = torch.zeros(1, 4, 8)
    with pytest.raises(ValueError, match="no bias"):
        add_layer_norm_fn(t, None, torch.ones(8), torch.zeros(8), rms=True)
    with pytest.raises(ValueError, match="no bias"):
        out_proj_add_ln_fn(torch.zeros(1, 64, 8), torch.zeros(128, 64), None, torch.ones(128), torch.zeros(128),
                           rms=True)
