"""CPU: the regime inputs of tests/scan_regimes.py and the float64 reference the device rows are judged by.

For every regime: the float64 reference (selective_scan_ref, acc_dtype=float64, double leaves) agrees with the O(L^2)
closed form at a small L; every reference tensor is finite; the promised share of delta + delta_bias lies in each
softplus band; no channel of any per-channel comparison has a zero or denormal scale; E_ref -- the error of the fp32 and
bf16 CPU oracles against float64, the only thing the GPU bounds are made from -- is computed and printed here, before any
device runs.  And the defect the small_dt regime exists for is shown from the reference side alone: a float32
restatement of log2(1 + e) * ln 2 misses the small_dt bound, torch's softplus does not.
"""
import pytest
import torch

import scan_regimes as sr
from oracle import scan_ref

EPS32 = 2.0 ** -23
FACTOR_F32 = 16.0
SHAPE = (2, 128, 136, 16)


@pytest.fixture(scope="module")
def cases():
    res = {}
    for name, fn in sr.REGIMES.items():
        L = 1024 if name == "long_memory" else SHAPE[2]
        inp = fn(SHAPE[0], SHAPE[1], L, SHAPE[3], seed=11)
        res[name] = (inp, sr.run_ref(inp, "f64"))
    return res


@pytest.mark.parametrize("name", list(sr.REGIMES))
def test_activations_are_bf16_values_and_layout_matches_scan_inputs(name):
    inp = sr.REGIMES[name](2, 16, 24, 16, seed=3)
    assert set(inp) == {"u", "delta", "A", "B", "C", "D", "z", "delta_bias", "dout"}
    for k in sr.ACT:
        assert inp[k].dtype == torch.float32 and torch.equal(inp[k], inp[k].bfloat16().float()), k
    for k in ("A", "D", "delta_bias"):
        assert inp[k].dtype == torch.float32
    assert (inp["A"] < 0).all()


@pytest.mark.parametrize("name", list(sr.REGIMES))
def test_reference_matches_closed_form(name):
    inp = sr.REGIMES[name](2, 12, 24, 16, seed=5)
    want = sr.run_ref(inp, "f64")["out"]
    closed = scan_ref.selective_scan_closed_form(inp["u"], inp["delta"], inp["A"], inp["B"], inp["C"], inp["D"],
                                                 inp["z"], inp["delta_bias"], delta_softplus=True)
    other = (0, 2)
    err = ((want - closed).abs().amax(other) / closed.abs().amax(other)).max().item()     # per channel
    assert err < 1e-11, err


@pytest.mark.parametrize("name", list(sr.REGIMES))
def test_reference_is_finite_and_leaves_no_channel_out(name, cases):
    inp, want = cases[name]
    assert set(want) == set(sr.TENSORS)
    for k, v in want.items():
        assert v.dtype == torch.float64 and torch.isfinite(v).all(), k
    floor = sr.channel_floor(want)
    print(name, {k: f"{v:.2e}" for k, v in floor.items()})
    assert set(floor) == set(sr.CHANNEL_DIM)
    for k, v in floor.items():
        assert v > 1e-30, (k, v)
    for k in ("dB", "dC", "dD", "ddelta_bias"):
        assert want[k].abs().max().item() > 1e-30, k


def _frac(x, lo, hi):
    return ((x >= lo) & (x < hi)).double().mean().item()


def test_softplus_bands(cases):
    x = sr.x_of(cases["small_dt"][0])
    assert x.min() >= -15.0 and x.max() <= -5.0
    assert _frac(x, -15.0, -12.0) >= 0.2 and _frac(x, -12.0, -9.0) >= 0.2 and _frac(x, -9.0, -4.999) >= 0.2

    # series_branch: everything below -15 except the upper seam elements (x = -15 + 1 ulp exactly), which the regime
    # must also have; the lower seam elements sit at -15 - 1 ulp
    x = sr.x_of(cases["series_branch"][0])
    up, lo = -15.0 + sr.ULP15, -15.0 - sr.ULP15
    assert x.min() >= -30.0
    assert ((x < -15.0) | (x == up)).all()
    assert (x == up).sum() >= 64 and (x == lo).sum() >= 64
    assert _frac(x, -30.0, -15.0) >= 0.99
    assert (x[:, 2:] < -15.0).all()                        # 100 % below -15 outside the two seam channels

    x = sr.x_of(cases["large_dt"][0])
    assert x.min() >= 15.0 and x.max() <= 100.0
    assert _frac(x, 15.0, 20.0) >= 0.05 and _frac(x, 20.0, 25.0) >= 0.05 and _frac(x, 88.0, 101.0) >= 0.2

    inp = cases["long_memory"][0]
    step = torch.nn.functional.softplus(sr.x_of(inp))
    assert inp["delta"].shape[2] == 1024
    assert step.min() >= 0.01 and step.max() <= 0.1 and inp["A"].min() >= -1e-2 and inp["A"].max() <= -1e-4

    inp = cases["fast_decay"][0]
    da = torch.nn.functional.softplus(sr.x_of(inp))[..., None] * inp["A"].double()[None, :, None, :]   # (B, D, L, N)
    assert da.min() >= -100.0 and da.max() <= -20.0
    assert (da.amax(-1) > -40.0).all()                      # every channel, every step: one state above -40
    assert _frac(da, -100.0, -87.34) >= 0.01                # and some where exp underflows the fp32 normal range

    z = cases["gate_ends"][0]["z"]
    assert z.min() < -29.0 and z.max() > 29.0 and z[:, 0::4].max() <= -15.0 and z[:, 1::4].min() >= 15.0


def test_mixed_changes_regime_between_adjacent_channels_and_successive_packs(cases):
    x = sr.x_of(cases["mixed"][0])                          # (B, D, L)

    def regime(v):      # 0 init-like, 1 small step, 2 series branch, 3 large step
        return torch.where(v > 15.0, 3, torch.where(v < -15.0, 2, torch.where(v < -6.0, 1, 0)))
    packs = x[:, :, :x.shape[2] // 4 * 4].reshape(x.shape[0], x.shape[1], -1, 4)
    for r, (lo, hi) in enumerate(((-6.5, -1.5), (-15.0, -5.0), (-30.0, -15.0), (15.0, 100.0))):
        sel = (torch.arange(x.shape[1])[:, None] + torch.arange(packs.shape[2])[None]) % 4 == r
        v = packs[:, sel]
        assert v.min() >= lo and v.max() <= hi, (r, v.min().item(), v.max().item())
    # one wave's 16 / 32 adjacent channels hold all four, and so do any four successive packs of a row
    centre = regime(packs.mean(-1))
    assert all(len(set(centre[0, d:d + 4, 0].tolist())) == 4 for d in range(0, 64))
    assert all(len(set(centre[0, 5, p:p + 4].tolist())) >= 3 for p in range(0, packs.shape[2] - 4))
    A = cases["mixed"][0]["A"]
    assert A[1::3].min() >= -1e-2 and A[2::3].max() <= -0.1


@pytest.mark.parametrize("name", list(sr.REGIMES))
def test_e_ref_exists_before_any_device_runs(name, cases):
    """E_ref of the fp32 and bf16 oracles, printed; the tensors that stay fp32 in a bf16 run (last_state and the parameter
    gradients dA, dD, ddelta_bias) have the SAME E_ref in both -- the inputs are bf16 values, so the two oracles compute
    them identically -- which is why the GPU test bounds them with the fp32 factor in bf16 rows too."""
    inp, want = cases[name]
    e32, e16 = sr.errors(sr.run_ref(inp, "f32"), want), sr.errors(sr.run_ref(inp, "bf16"), want)
    for k in sr.TENSORS:
        print(f"{name} {k}: E_ref fp32 chan {e32[k]['chan']:.3e} max {e32[k]['max']:.3e} rms {e32[k]['rms']:.3e} | "
              f"bf16 chan {e16[k]['chan']:.3e} max {e16[k]['max']:.3e} rms {e16[k]['rms']:.3e}")
        assert e32[k]["chan"] < 1e-3 and e16[k]["chan"] < 2e-2, k          # the oracles themselves are sound here
    for k in ("last_state", "dA", "dD", "ddelta_bias"):
        assert e32[k] == e16[k], k


def _run_with_softplus(inp, softplus, mode="f32"):
    """The fp32 oracle with its softplus replaced: delta handed over as the step itself (delta_softplus off).  The
    gradient of the step with respect to x is not part of this check: forward tensors and the step's own gradient."""
    step = softplus(inp["delta"] + inp["delta_bias"][None, :, None])
    sub = dict(inp, delta=step, delta_bias=None)
    return sr.run_ref(sub, mode, delta_softplus=False)


def test_old_softplus_form_violates_the_small_dt_bound_and_torch_does_not(cases):
    inp, want = cases["small_dt"]
    e_ref = sr.errors(sr.run_ref(inp, "f32"), want)
    old = sr.errors(_run_with_softplus(inp, sr.softplus_log2_form_f32), want)
    new = sr.errors(_run_with_softplus(inp, sr.softplus_torch_f32), want)
    for k in ("out", "last_state", "du", "dz"):
        bound = FACTOR_F32 * max(e_ref[k]["chan"], EPS32)
        print(f"small_dt {k}: bound {bound:.3e}  log2(1 + e) form {old[k]['chan']:.3e}  F.softplus {new[k]['chan']:.3e}")
        assert old[k]["chan"] > 10 * bound, k
        assert new[k]["chan"] <= bound, k
    # the formula itself, per band of x, on the regime's own x (relative error of the step)
    x = (inp["delta"] + inp["delta_bias"][None, :, None]).flatten()
    ref = torch.nn.functional.softplus(x.double())
    rel_old = ((sr.softplus_log2_form_f32(x).double() - ref).abs() / ref)
    rel_new = ((sr.softplus_torch_f32(x).double() - ref).abs() / ref)
    for lo, hi, least in ((-15.0, -12.0, 1e-2), (-12.0, -9.0, 1e-3), (-9.0, -7.0, 1e-4), (-7.0, -5.0, 1e-5)):
        m = (x >= lo) & (x < hi)
        print(f"x in [{lo}, {hi}): log2(1 + e) form {rel_old[m].max():.2e}  F.softplus {rel_new[m].max():.2e}")
        assert rel_old[m].max() > least and rel_new[m].max() < 2.5e-7
