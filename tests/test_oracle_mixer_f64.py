"""CPU: the float64 statement of the whole mixer (oracle.scan_ref.MambaRef with acc_dtype=float64) checks itself.

It is what tests/test_gpu_mixer_routes.py measures the device AND the fp32 / bf16 oracles against, so it has to be
right on its own evidence: (1) its forward against a composition written out here stage by stage with the O(L^2)
closed form in place of the sequential scan, (2) its autograd gradients -- input and all nine parameters -- against
central differences in float64, (3) the default fp32 path is untouched by the new argument."""
import pytest
import torch
import torch.nn.functional as F

from oracle import scan_ref

CASES = [  # (d_model, d_state, d_conv, conv_bias)
    (8, 16, 4, True), (8, 8, 3, True), (8, 8, 2, False), (12, 16, 4, False)]


def _ref64(d_model, d_state, d_conv, conv_bias, seed):
    torch.manual_seed(seed)
    ref = scan_ref.MambaRef(d_model, d_state=d_state, d_conv=d_conv, conv_bias=conv_bias)
    with torch.no_grad():                           # off the init's special values (A_log rows equal, D = 1)
        ref.A_log.add_(0.1 * torch.randn_like(ref.A_log))
        ref.D.add_(0.1 * torch.randn_like(ref.D))
    return ref, scan_ref.mamba_ref_f64(ref)


@pytest.mark.parametrize("d_model,d_state,d_conv,conv_bias", CASES)
def test_f64_mixer_matches_stagewise_closed_form(d_model, d_state, d_conv, conv_bias):
    """in_proj, conv (an explicit tap loop) + SiLU, x_proj, dt_proj, the scan + D + gate as the closed form, out_proj:
    each stage restated independently in float64."""
    _, r = _ref64(d_model, d_state, d_conv, conv_bias, seed=0)
    Bsz, L, D, R, N = 2, 12, r.d_inner, r.dt_rank, d_state
    h = torch.randn(Bsz, L, d_model, dtype=torch.float64)
    got = r(h, acc_dtype=torch.float64)
    assert got.dtype == torch.float64
    xz = torch.einsum("jc,blc->bjl", r.in_proj.weight, h)
    x, z = xz[:, :D], xz[:, D:]
    w = r.conv1d.weight[:, 0]
    xc = torch.zeros_like(x)
    for t in range(L):
        for k in range(d_conv):
            s = t - (d_conv - 1) + k
            if s >= 0:
                xc[:, :, t] += w[:, k] * x[:, :, s]
    if conv_bias:
        xc = xc + r.conv1d.bias[None, :, None]
    xc = xc * torch.sigmoid(xc)
    x_dbl = torch.einsum("sd,bdl->bls", r.x_proj.weight, xc)
    delta = torch.einsum("dr,blr->bdl", r.dt_proj.weight, x_dbl[:, :, :R])
    y = scan_ref.selective_scan_closed_form(xc, delta, -torch.exp(r.A_log), x_dbl[:, :, R:R + N].transpose(1, 2),
                                            x_dbl[:, :, R + N:].transpose(1, 2), r.D, z=z,
                                            delta_bias=r.dt_proj.bias, delta_softplus=True)
    want = torch.einsum("cd,bdl->blc", r.out_proj.weight, y)
    # float64 sums of < 100 terms of order 1: 1e-12 is ~1e4 ulp, a wrong term is >= 1e-6
    assert (got - want).abs().max().item() < 1e-12 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("d_model,d_state,d_conv,conv_bias", CASES)
def test_f64_mixer_gradients_match_central_differences(d_model, d_state, d_conv, conv_bias):
    """torch.autograd.gradcheck (central differences, float64) over the input and every parameter.  eps = 1e-6: the
    truncation error is ~eps^2 |f'''| ~ 1e-12 and the rounding error ~2^-53 |f| / eps ~ 1e-10, so analytic and numeric
    Jacobians have to agree to ~1e-9; asserted at atol 1e-8 + rtol 1e-7."""
    _, r = _ref64(d_model, d_state, d_conv, conv_bias, seed=1)
    names = [k for k, _ in r.named_parameters()]
    assert len(names) == (9 if conv_bias else 8)
    h = torch.randn(1, 5, d_model, dtype=torch.float64, requires_grad=True)
    params = [p.detach().clone().requires_grad_(True) for _, p in r.named_parameters()]

    def f(hh, *ps):
        return torch.func.functional_call(r, dict(zip(names, ps)), (hh,), {"acc_dtype": torch.float64})
    assert torch.autograd.gradcheck(f, (h, *params), eps=1e-6, atol=1e-8, rtol=1e-7)


def test_f64_gradients_are_float64_and_close_to_fp32():
    """mamba_ref_f64 leaves float64 gradients holding what the fp32 oracle computes, to fp32 rounding."""
    ref, r64 = _ref64(16, 16, 4, True, seed=2)
    h = torch.randn(2, 20, 16)
    dout = torch.randn(2, 20, 16)
    h32, h64 = h.clone().requires_grad_(True), h.double().requires_grad_(True)
    ref(h32).backward(dout)
    r64(h64, acc_dtype=torch.float64).backward(dout.double())
    assert h64.grad.dtype == torch.float64
    for (k, p), (_, q) in zip(ref.named_parameters(), r64.named_parameters()):
        assert q.grad.dtype == torch.float64 and torch.equal(q.detach().float(), p.detach()), k
        scale = q.grad.abs().max().item()
        assert (p.grad.double() - q.grad).abs().max().item() < 1e-5 * scale, k


def test_default_path_unchanged_by_acc_dtype_argument():
    """acc_dtype defaults to float32 and then adds no op: same bits as spelling it out, fp32 and autocast forms."""
    ref, _ = _ref64(16, 16, 4, True, seed=3)
    h = torch.randn(2, 20, 16)
    assert torch.equal(ref(h), ref(h, acc_dtype=torch.float32))
    assert ref(h).dtype == torch.float32
    x = torch.randn(2, 6, 9)
    w = torch.randn(6, 4)
    want = F.silu(F.conv1d(x.float(), w.float()[:, None, :], None, padding=3, groups=6)[..., :9])
    assert torch.equal(scan_ref.causal_conv1d_ref(x, w, None, "silu"), want)
    with pytest.raises(ValueError):
        ref(h, io_dtype=torch.bfloat16, acc_dtype=torch.float64)
