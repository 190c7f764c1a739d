"""GPU: every scan kernel against float64, across softplus, decay and gate regimes (tests/scan_regimes.py).

The other scan tests draw from one distribution (x = delta + delta_bias in [-8, -1], A ~ -(1..16), z ~ N(0,1)) and
normalise by max(1, max |want|) over the whole tensor.  Here each regime moves one range (small steps down to x = -15,
the series branch below, the linear branch above 20 and past exp's overflow, hardly-decaying and immediately-decaying
states, the ends of the gate, and all of them inside one launch), and the error is taken PER CHANNEL on the channel's
own scale (scan_regimes.channel_err): a channel whose step is 1e-6 is not hidden behind one whose step is 0.1.

Metric, per tensor: out, last_state, du, ddelta, dz -- max over channels of max |got - want| / max |want| of that
channel; dA -- the same per row; dD, ddelta_bias -- per element on the tensor's maximum (the worst single-element
relative error is recorded too); dB, dC -- the tensor's own scale (they are sums over channels).  helpers.scaled_err
(max and RMS over the whole tensor) is bounded the same way, and the suite's nerr bars (1e-3 fp32, 1e-2 bf16) hold too.

Bound, from the reference side only: E_dev <= F * max(E_ref, 2^-23), E_ref being the same metric for the CPU oracle of
that dtype (selective_scan_ref in fp32; for bf16 rows the same with bf16 outputs) against the float64 reference.  F is
the factor of tests/test_gpu_mixer_routes.py, with its reasoning: 16 for fp32, 4 for bf16.  One named override,
FACTOR_TENSOR: last_state, dA, dD and ddelta_bias are fp32 tensors in a bf16 run too, and because every activation of a
regime is a bf16 value the bf16 oracle computes them exactly as the fp32 oracle does (test_oracle_scan_regimes.py asserts
the two E_ref equal) -- no bf16 rounding enters on either side, so the fp32 reasoning and its factor 16 apply to them.

With SIMAMBA_SCAN_REGIMES_JSON=<path> set, every row's E_ref, E_dev and counters are written there
(profiles/scan_regimes.json is such a run).
"""
import functools
import json
import os

import pytest
import torch

import scan_regimes as sr
from helpers import nerr
from si_mamba_amd import _lib

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
FACTOR = {F32: 16.0, BF16: 4.0}
FACTOR_TENSOR = {(BF16, k): 16.0 for k in ("last_state", "dA", "dD", "ddelta_bias")}      # fp32 tensors: see docstring
NERR = {F32: 1e-3, BF16: 1e-2}
EPS32 = 2.0 ** -23
SHAPE = (2, 128, 16)                                   # batch, dim, N
# (forward variant, checkpoint layout = backward kernel, deterministic)
ROUTES = [("row", _lib.SCAN_ROWSCAN, _lib.CKPT_ROW, False), ("lpc2", _lib.SCAN_LPC2, _lib.CKPT_SEQ, False),
          ("lpc4", _lib.SCAN_LPC4, _lib.CKPT_SEQ, True), ("auto", _lib.SCAN_AUTO, _lib.CKPT_ROW, True)]
_RESULTS = {}


@pytest.fixture(scope="module", autouse=True)
def _record_results():
    yield
    path = os.environ.get("SIMAMBA_SCAN_REGIMES_JSON")
    if path and _RESULTS:
        with open(path, "w") as fh:
            fh.write(_dump(_RESULTS))


def _dump(rows):
    """One line per row, three significant digits: {row: {counters, E_ref, E_dev}}, each error as [chan, max, rms] (+ elem
    for dD and ddelta_bias)."""
    def short(errs):
        return {k: [float(f"{e[w]:.3g}") for w in ("chan", "max", "rms", "elem") if w in e] for k, e in errs.items()}
    head = {"metric": "[chan, max, rms(, elem)] per tensor.  chan: max over channels of max |got - want| / max |want| of "
                      "the channel (dD, ddelta_bias, dB, dC: on the tensor's maximum); max / rms: helpers.scaled_err; elem: "
                      "worst single-element relative error; all against the float64 selective_scan_ref.  E_ref: the fp32 "
                      "/ bf16 CPU oracle, E_dev: the device"}
    lines = [json.dumps(tag) + ": " + json.dumps({"counters": r["counters"], "E_ref": short(r["E_ref"]),
                                                  "E_dev": short(r["E_dev"])}) for tag, r in rows.items()]
    return "{" + json.dumps("metric") + ": " + json.dumps(head["metric"]) + ",\n" + json.dumps("rows") + ": {\n" + \
        ",\n".join(lines) + "\n}}\n"


def _cases():
    rows = []
    for name in sr.REGIMES:
        Ls = [136, 264] + ([1024] if name in ("long_memory", "mixed") else [])
        rows += [(name, L) for L in Ls]
    return rows


@functools.lru_cache(maxsize=2)
def _reference(name, batch, dim, L, N, drop=()):
    inp = sr.REGIMES[name](batch, dim, L, N, seed=1000 + L)
    for k in drop:
        inp[k] = None
    want = sr.run_ref(inp, "f64")
    return inp, want, {}


def _e_ref(key, dtype):
    inp, want, cache = _reference(*key)
    if dtype not in cache:
        cache[dtype] = sr.errors(sr.run_ref(inp, "f32" if dtype == F32 else "bf16"), want)
    return cache[dtype]


def _device_run(inp, dtype, device, variant, ckpt, delta_softplus=True):
    from si_mamba_amd import selective_scan_fn
    leaf = {}
    for k in sr.LEAVES:
        if inp.get(k) is not None:
            v = inp[k].to(device)
            leaf[k] = (v.to(dtype) if k in sr.ACT else v).requires_grad_(True)
    _lib.counters.clear()
    with _lib.scan_variant(variant), _lib.scan_ckpt(ckpt):
        out, last = selective_scan_fn(leaf["u"], leaf["delta"], leaf["A"], leaf["B"], leaf["C"], leaf.get("D"),
                                      leaf.get("z"), leaf.get("delta_bias"), delta_softplus, True)
    assert out.dtype == dtype and last.dtype == F32
    out.backward(inp["dout"].to(device).to(dtype))
    torch.cuda.synchronize()
    res = {"out": out.detach().float().cpu(), "last_state": last.cpu()}
    res.update({sr._GRAD_NAME[k]: v.grad.float().cpu() for k, v in leaf.items()})
    return res, dict(_lib.counters)


def _violations(tag, got, want, e_ref, dtype):
    e_dev = sr.errors(got, want)
    bad = []
    for k in want:
        f = FACTOR_TENSOR.get((dtype, k), FACTOR[dtype])
        ne = nerr(got[k], want[k])
        print(f"{tag} {k}: E_ref chan {e_ref[k]['chan']:.3e} max {e_ref[k]['max']:.3e} rms {e_ref[k]['rms']:.3e}  "
              f"E_dev chan {e_dev[k]['chan']:.3e} max {e_dev[k]['max']:.3e} rms {e_dev[k]['rms']:.3e}  nerr {ne:.3e}"
              + (f"  elem {e_dev[k]['elem']:.3e}" if "elem" in e_dev[k] else ""))
        if not torch.isfinite(got[k]).all():
            bad.append((k, "non-finite"))
        for what in ("chan", "max", "rms"):
            if not e_dev[k][what] <= f * max(e_ref[k][what], EPS32):
                bad.append((k, what, e_dev[k][what], e_ref[k][what]))
        if not ne < NERR[dtype]:
            bad.append((k, "nerr", ne))
    return e_dev, bad


def test_table_covers_every_regime_and_route():
    """Review aid: a regime, a length or a route cannot quietly go."""
    cases = _cases()
    assert {n for n, _ in cases} == {"init", "small_dt", "series_branch", "large_dt", "long_memory", "fast_decay",
                                     "gate_ends", "mixed"}
    assert all({(n, 136), (n, 264)} <= set(cases) for n in sr.REGIMES)
    assert ("long_memory", 1024) in cases and ("mixed", 1024) in cases
    assert {r[1] for r in ROUTES} == {_lib.SCAN_ROWSCAN, _lib.SCAN_LPC2, _lib.SCAN_LPC4, _lib.SCAN_AUTO}
    assert {(r[2], r[3]) for r in ROUTES} == {(c, d) for c in (_lib.CKPT_ROW, _lib.CKPT_SEQ) for d in (False, True)}
    assert FACTOR == {F32: 16.0, BF16: 4.0}


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,L", _cases(), ids=[f"{n}-L{L}" for n, L in _cases()])
def test_scan_regime(name, L, dtype, route, device):
    rname, variant, ckpt, det = route
    key = (name, SHAPE[0], SHAPE[1], L, SHAPE[2])
    inp, want, _ = _reference(*key)
    e_ref = _e_ref(key, dtype)
    _lib.set_deterministic(det)
    try:
        got, counters = _device_run(inp, dtype, device, variant, ckpt)      # a forced variant runs or refuses by name
        again = _device_run(inp, dtype, device, variant, ckpt)[0] if det else None
    finally:
        _lib.set_deterministic(None)
    # the route: the checkpoint layout (= which backward kernel) and the deterministic / atomic form that ran
    assert counters == {"scan_ckpt_seq" if ckpt == _lib.CKPT_SEQ else "scan_ckpt_row": 1,
                        "scan_bwd_det" if det else "scan_bwd_atomic": 1}, counters
    if variant == _lib.SCAN_AUTO:       # the library's own choice at 256 rows is the row scan
        assert _lib.load().simamba_scan_fwd_auto_variant(SHAPE[0], SHAPE[1]) == _lib.SCAN_ROWSCAN
    if again is not None:
        for k in got:
            assert torch.equal(got[k], again[k]), k
    tag = f"{name}-L{L}-{'f32' if dtype == F32 else 'bf16'}-{rname}"
    e_dev, bad = _violations(tag, got, want, e_ref, dtype)
    _RESULTS[tag] = {"counters": counters, "E_ref": e_ref, "E_dev": e_dev}
    assert not bad, bad


@pytest.mark.parametrize("name", ["mixed", "small_dt", "large_dt"])
def test_scan_regime_mixed_launch(name, device):
    """SCAN_MIX (two and four lanes per channel in one launch) at (64, 768, 160), a shape of test_scan_mixed_launch: out,
    last_state and the per-element gradients of a channel subset on both sides of the seam (channel 512), two samples."""
    from si_mamba_amd import selective_scan_fn
    B, D, L, N = 64, 768, 160, 16
    inp = sr.REGIMES[name](B, D, L, N, seed=64 + L)
    t = {k: v.to(device) for k, v in inp.items()}
    leaf = {k: t[k].clone().requires_grad_(True) for k in ("u", "delta", "z")}
    _lib.counters.clear()
    with _lib.scan_variant(_lib.SCAN_MIX):                                # refused by name where it does not apply
        out, last = selective_scan_fn(leaf["u"], leaf["delta"], t["A"], t["B"], t["C"], t["D"], leaf["z"],
                                      t["delta_bias"], True, True)
    out.backward(t["dout"])
    ds = torch.tensor([0, 1, 31, 32, D // 2, D - 257, D - 256, D - 255, D - 17, D - 16, D - 1])
    bs = torch.tensor([0, B - 1])
    sub = {k: (v[bs][:, ds] if k in ("u", "delta", "z", "dout") else v[bs] if k in ("B", "C") else v[ds])
           for k, v in inp.items()}
    want = sr.run_ref(sub, "f64")
    e_ref = sr.errors(sr.run_ref(sub, "f32"), want)
    pick = lambda v: v.detach().cpu()[bs][:, ds]                      # noqa: E731
    got = {"out": pick(out), "last_state": pick(last), "du": pick(leaf["u"].grad), "ddelta": pick(leaf["delta"].grad),
           "dz": pick(leaf["z"].grad)}
    want = {k: want[k] for k in got}
    e_dev, bad = _violations(f"{name}-mix", got, want, e_ref, F32)
    _RESULTS[f"{name}-B64-D768-L160-f32-mix"] = {"counters": dict(_lib.counters), "E_ref": {k: e_ref[k] for k in got},
                                                 "E_dev": e_dev}
    assert not bad, bad


@pytest.mark.parametrize("name", list(sr.REGIMES))
@pytest.mark.parametrize("N", [7, 16])
def test_scan_regime_row_scan_without_softplus(name, N, device):
    """Row scan only (the other kernels require softplus and 16 states): delta_softplus off, the regime's own positive
    steps handed over as delta; 7 and 16 states."""
    inp = dict(sr.REGIMES[name](2, 40, 136, N, seed=70 + N))
    step = torch.nn.functional.softplus(sr.x_of(inp)).float().bfloat16().float()
    step = torch.where(step > 0, step, torch.full_like(step, 2.0 ** -126))      # a bf16 value; steps stay positive
    inp.update(delta=step, delta_bias=None)
    want = sr.run_ref(inp, "f64", delta_softplus=False)
    e_ref = sr.errors(sr.run_ref(inp, "f32", delta_softplus=False), want)
    got, counters = _device_run(inp, F32, device, _lib.SCAN_ROWSCAN, _lib.CKPT_ROW, delta_softplus=False)
    assert counters == {"scan_ckpt_row": 1, "scan_bwd_atomic": 1}
    e_dev, bad = _violations(f"{name}-N{N}-nosoftplus", got, want, e_ref, F32)
    _RESULTS[f"{name}-L136-N{N}-f32-row-nosoftplus"] = {"counters": counters, "E_ref": e_ref, "E_dev": e_dev}
    assert not bad, bad


@pytest.mark.parametrize("name", ["small_dt", "large_dt", "mixed"])
def test_scan_regime_row_scan_without_optional_operands(name, device):
    """z, D and delta_bias absent (the regime's bias folded into delta, rounded to bf16 once)."""
    inp = dict(sr.REGIMES[name](2, 40, 136, 16, seed=91))
    inp.update(delta=sr.x_of(inp).float().bfloat16().float(), delta_bias=None, z=None, D=None)
    want = sr.run_ref(inp, "f64")
    e_ref = sr.errors(sr.run_ref(inp, "f32"), want)
    got, counters = _device_run(inp, F32, device, _lib.SCAN_ROWSCAN, _lib.CKPT_ROW)
    assert set(got) == set(want) and "dz" not in got and "dD" not in got and "ddelta_bias" not in got
    e_dev, bad = _violations(f"{name}-bare", got, want, e_ref, F32)
    _RESULTS[f"{name}-L136-f32-row-bare"] = {"counters": counters, "E_ref": e_ref, "E_dev": e_dev}
    assert not bad, bad


# ---- the kernels that form delta themselves --------------------------------------------------------------------------
def _dt_operands(name, B, D, L, R, dtype, device):
    """Operands of simamba_selective_scan_dt_fwd / _bwd in a regime: the regime's bias, and dt columns / dt_proj weights
    scaled so that delta = wdt @ dt reproduces the regime's own delta range (all operands bf16 values)."""
    inp = sr.REGIMES[name](B, D, L, 16, seed=300 + L + R)
    g = torch.Generator().manual_seed(R + L)
    spread = min(inp["delta"].abs().max().item(), 1.0)      # the regime's delta range; delta itself is re-formed
    dt = (torch.randn(B, L, R, generator=g) * 0.5).clamp(-1.0, 1.0)
    wdt = (torch.rand(D, R, generator=g) * 2 - 1) * spread / R
    xdbl = torch.cat([dt, inp["B"].transpose(1, 2), inp["C"].transpose(1, 2)], dim=2).bfloat16().float()
    wdt = wdt.bfloat16().float()
    delta = torch.einsum("dr,blr->bdl", wdt.double(), xdbl[:, :, :R].double())
    if dtype == BF16:                                       # rounded once, where the materialised tensor would be
        delta = delta.float().bfloat16().double()
    t = dict(u=inp["u"].to(dtype), z=inp["z"].to(dtype), xdbl=xdbl.to(dtype), wdt=wdt.to(dtype),
             dout=inp["dout"].to(dtype))
    t = {k: v.to(device).contiguous() for k, v in t.items()}
    t.update(A=inp["A"].contiguous().to(device), D=inp["D"].to(device), bias=inp["delta_bias"].to(device))
    return inp, delta, t


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["init", "small_dt", "series_branch", "large_dt"])
def test_scan_regime_dt_kernels(name, dtype, device):
    """simamba_selective_scan_dt_fwd / _bwd (delta formed in the kernel from the dt columns) against float64 on the delta
    the kernel is specified to form: the exact product in fp32 rows, rounded to bf16 once in bf16 rows."""
    from test_gpu_scan_dt import _run
    B, D, L, R = 2, 128, 136, 8
    inp, delta, t = _dt_operands(name, B, D, L, R, dtype, device)

    def oracle(mode):
        f64 = mode == "f64"
        cast = (lambda v: v.detach().double().clone()) if f64 else (lambda v: v.detach().float().clone())
        leaf = {k: cast(inp[k]).requires_grad_(True) for k in ("u", "z", "A", "D", "delta_bias", "B", "C")}
        dl = cast(delta).requires_grad_(True)
        out = sr.scan_ref.selective_scan_ref(leaf["u"], dl, leaf["A"], leaf["B"], leaf["C"], leaf["D"], leaf["z"],
                                             leaf["delta_bias"], delta_softplus=True,
                                             acc_dtype=torch.float64 if f64 else torch.float32)
        out.backward(cast(inp["dout"]))
        res = {"out": out.detach(), "du": leaf["u"].grad, "ddelta": dl.grad, "dz": leaf["z"].grad, "dA": leaf["A"].grad,
               "dB": leaf["B"].grad, "dC": leaf["C"].grad, "dD": leaf["D"].grad, "ddelta_bias": leaf["delta_bias"].grad}
        if mode == "bf16":
            for k in ("out", "du", "ddelta", "dz"):
                res[k] = res[k].bfloat16().float()
        return res
    want = oracle("f64")
    e_ref = sr.errors(oracle("f32" if dtype == F32 else "bf16"), want)
    dev = _run(t, True, 2)
    got = {k: dev["dbias" if k == "ddelta_bias" else k].float().cpu() for k in want}
    e_dev, bad = _violations(f"{name}-dt", got, want, e_ref, dtype)
    _RESULTS[f"{name}-L136-{'f32' if dtype == F32 else 'bf16'}-dt"] = {"counters": {}, "E_ref": e_ref, "E_dev": e_dev}
    assert not bad, bad


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["small_dt", "series_branch", "large_dt"])
def test_mixer_in_kernel_delta_bit_identical_in_regime(name, dtype, device):
    """The mixer with the regime's bias as dt_proj.bias: delta formed in the scan kernels gives bit for bit the output of
    the materialised path (what test_gpu_scan_dt.py requires at initialisation values)."""
    from si_mamba_amd import Mamba
    torch.manual_seed(3)
    m = Mamba(128, layer_idx=0).to(device)
    bias = sr.REGIMES[name](1, m.d_inner, 8, 16, seed=5)["delta_bias"]
    with torch.no_grad():
        m.dt_proj.bias.copy_(bias.to(device))
    h = torch.randn(3, 96, 128, device=device)
    outs = {}
    for fused in (True, False):
        before = _lib.counters.get("scan_dt_fwd", 0)
        x = h.clone().requires_grad_(True)
        with _lib.scan_ckpt(_lib.CKPT_SEQ), _lib.scan_fuse_dt(fused), torch.autocast("cuda", dtype=BF16,
                                                                                    enabled=dtype == BF16):
            out = m(x)
        out.float().sum().backward()
        assert (_lib.counters.get("scan_dt_fwd", 0) - before) == (1 if fused else 0)
        outs[fused] = (out.detach().clone(), x.grad.clone())
    assert torch.isfinite(outs[True][0]).all() and torch.isfinite(outs[True][1]).all()
    assert torch.equal(outs[True][0], outs[False][0])
