"""GPU: si_mamba_amd.Mamba on every dispatch route against a float64 statement of the same mixer.

One mixer forward / backward passes through ~eight routing decisions (_lib.scan_plan, fuse_dt and xdt_proj_fused_ok
in mamba_inner.py, in_proj_hand_enabled, the deterministic switch, and inside the library auto_variant, seq_ok,
scan_fwd_seq_bc_mode, scan_bwd_seq_ok) that depend on batch * d_inner, d_inner % 64, dt_rank % 4 and % 8, L % 4 and
% 8, L <= 16, d_state and d_conv.  Each row of ROWS pins one combination, runs the default fast path forward +
backward on the whole batch, asserts -- through _lib.counters -- that the run took the route the row states (so a
passing row cannot be one that silently fell back), and compares the output, the input gradient and every parameter
gradient with oracle.scan_ref.MambaRef computed in float64 from the same weights and inputs.

Metric and bounds (tests/helpers.scaled_err: max and RMS error on the tensor's OWN scale, no floor of 1 -- three of
the gradients are of order 1e-3 .. 1e-2, where the suite's ``nerr`` passes anything).  The bounds come from the
reference side only, never from what the device returned:

  fp32   E_ref = error of the fp32 CPU oracle (MambaRef, same weights / inputs) against float64.
         E_dev <= 16 * max(E_ref, 2^-23), and nerr < 1e-3 as everywhere in the suite.  16: device and CPU oracle both
         compute in fp32 and differ in summation order (4x4 MFMA blocks, wave reductions, atomics over up to
         B * L ~ 16 k terms) and in exp / softplus being 1-2 ulp off where libm rounds correctly: a small factor each.
         A wrong term of 1e-4 relative still lies 10x outside.
  bf16   E_ref = error of MambaRef(io_dtype=bfloat16) -- the oracle that carries the autocast roundings -- against
         float64.  E_dev <= 4 * E_ref, and nerr < 1e-2.  4: identical roundings on the forward; the device also
         carries bf16 gradients between the ops where the oracle carries fp32 ones (test_mamba_bf16_autocast), a few
         more roundings of 2^-9 on values of the same scale.

With SIMAMBA_MIXER_ROUTES_JSON=<path> set, every row's E_ref, E_dev and route counters are written there
(profiles/mixer_routes.json is such a run).
"""
import functools
import json
import os

import pytest
import torch

from compose import mixer_oracle_run as _oracle
from helpers import nerr, scaled_err
from oracle import scan_ref
from si_mamba_amd import _lib

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SEQ, ROW = "seq", "row"                  # scan checkpoint step: CKPT_SEQ (lanes-per-channel pair) / CKPT_ROW (row scan)
SCAN, MAT = "scan", "mat"                # delta formed inside the scan kernels / materialised
CONV_FUSED, FUSED, GEMM = "xdt_conv_fused", "xdt_fused", "xdt_gemm"   # conv + x_proj + dt_proj route
FACTOR = {F32: 16.0, BF16: 4.0}          # per-tensor overrides would go in FACTOR_TENSOR, each with its evidence
FACTOR_TENSOR = {}
NERR = {F32: 1e-3, BF16: 1e-2}
EPS32 = 2.0 ** -23


def R(B, L, d, dtype, ckpt, delta, xdt, N=16, W=4, det=False, bias=True):
    return dict(B=B, L=L, d=d, N=N, W=W, dtype=dtype, det=det, bias=bias, ckpt=ckpt, delta=delta, xdt=xdt)


# (B, L, d_model, dtype, expected checkpoint step, expected delta route, expected xdt route, ...).  d_inner = 2 d_model,
# dt_rank = ceil(d_model / 16); "above" = batch * d_inner >= 49 152 rows.  Rows of one shape are adjacent: they share
# one float64 reference.
ROWS = [
    # -- the threshold itself, d_model 128 (dt_rank 8): 49 152 rows and 49 152 - d_inner; dt_rank % 8 == 0 fp32 / bf16
    R(192, 64, 128, F32, SEQ, MAT, CONV_FUSED),                # above, dt_rank % 8 == 0, fp32
    R(192, 64, 128, BF16, SEQ, SCAN, CONV_FUSED),              # above, dt_rank % 8 == 0, bf16: scan_dt_fwd
    R(192, 64, 128, F32, SEQ, MAT, CONV_FUSED, det=True),      # deterministic: sequential backward
    R(192, 64, 128, BF16, SEQ, SCAN, CONV_FUSED, det=True),    # deterministic: sequential backward forming delta
    R(191, 64, 128, F32, ROW, MAT, CONV_FUSED),                # one sample below the line: row scan
    R(191, 64, 128, BF16, ROW, MAT, CONV_FUSED),
    # -- the d_model = 384 anchor (the full-batch model steps run this route; compared here against a reference)
    R(64, 64, 384, BF16, SEQ, SCAN, CONV_FUSED),
    # -- dt_rank % 8 == 4 (d_model 64: dt_rank 4; 192: 12): bf16 materialises delta, and the sequential kernels read
    #    token-major B / C packs at 8-byte, not 16-byte, aligned addresses
    R(384, 64, 64, F32, SEQ, MAT, CONV_FUSED),
    R(384, 64, 64, BF16, SEQ, MAT, CONV_FUSED),
    R(128, 64, 192, F32, SEQ, MAT, CONV_FUSED),
    R(128, 64, 192, BF16, SEQ, MAT, CONV_FUSED),
    # -- dt_rank % 4 == 2 (d_model 96: dt_rank 6; 160: 10): B / C off a pack boundary -> row-scan pair, library GEMMs
    #    (at the parent commit: RuntimeError from the refused CKPT_SEQ forward)
    R(256, 64, 96, F32, ROW, MAT, GEMM),
    R(256, 64, 96, BF16, ROW, MAT, GEMM),
    R(256, 64, 96, F32, ROW, MAT, GEMM, det=True),             # deterministic: row-scan backward above the line
    R(256, 64, 96, BF16, ROW, MAT, GEMM, det=True),
    R(154, 64, 160, F32, ROW, MAT, GEMM),
    R(154, 64, 160, BF16, ROW, MAT, GEMM),
    # -- dt_rank % 4 == 2 with S % 4 != 0 at d_inner = 64 (d_model 32: dt_rank 2, S = 34)
    R(768, 64, 32, F32, ROW, MAT, GEMM),
    R(768, 64, 32, BF16, ROW, MAT, GEMM),
    # -- dt_rank > 24, dt_rank % 4 == 0 (d_model 448: dt_rank 28): library GEMMs for x_proj / dt_proj, CKPT_SEQ kept
    R(56, 64, 448, F32, SEQ, MAT, GEMM),
    R(56, 64, 448, BF16, SEQ, MAT, GEMM),
    # -- d_inner > 1024 and S > 64 (d_model 576: d_inner 1152, dt_rank 36, S = 68): the conv cannot be fused
    R(43, 64, 576, F32, SEQ, MAT, GEMM),
    R(43, 64, 576, BF16, SEQ, MAT, GEMM),
    # -- L = 16: CKPT_SEQ without a checkpoint buffer (above), one row-scan chunk (below)
    R(192, 16, 128, F32, SEQ, MAT, CONV_FUSED),
    R(192, 16, 128, BF16, SEQ, SCAN, CONV_FUSED),
    R(4, 16, 128, F32, ROW, MAT, CONV_FUSED),
    # -- L = 20: % 4 == 0 but % 8 != 0 -- fp32 takes the sequential kernels, bf16 must not
    R(192, 20, 128, F32, SEQ, MAT, CONV_FUSED),
    R(192, 20, 128, BF16, ROW, MAT, GEMM),
    R(4, 20, 128, F32, ROW, MAT, CONV_FUSED),
    R(4, 20, 128, BF16, ROW, MAT, GEMM),
    # -- L % 4 == 2 (66): nothing vectorisable -> row scan, library GEMMs
    R(192, 66, 128, F32, ROW, MAT, GEMM),
    R(4, 66, 128, BF16, ROW, MAT, GEMM),
    # -- L = 64 / 68: the single-chunk boundary of the row scan (64 below is the config-1 golden shape)
    R(2, 64, 128, F32, ROW, MAT, CONV_FUSED),
    R(4, 68, 128, F32, ROW, MAT, CONV_FUSED),
    R(192, 68, 128, F32, SEQ, MAT, CONV_FUSED),
    R(192, 68, 128, BF16, ROW, MAT, GEMM),
    # -- L = 132: ragged past one 128-step chunk
    R(384, 132, 64, F32, SEQ, MAT, CONV_FUSED),
    R(4, 132, 128, F32, ROW, MAT, CONV_FUSED),
    R(4, 132, 128, F32, ROW, MAT, CONV_FUSED, det=True),       # deterministic: row-scan backward, two chunks
    # -- L = 208: the MAE length
    R(384, 208, 64, BF16, SEQ, MAT, CONV_FUSED),
    R(4, 208, 128, F32, ROW, MAT, CONV_FUSED),
    R(4, 208, 128, BF16, ROW, MAT, CONV_FUSED),
    # -- shapes the lanes-per-channel kernels must refuse cleanly, above the line
    R(123, 64, 200, F32, ROW, MAT, GEMM),                      # d_inner % 64 != 0 (400), dt_rank 13
    R(123, 64, 200, BF16, ROW, MAT, GEMM),
    R(192, 64, 128, F32, ROW, MAT, CONV_FUSED, N=8),           # d_state 8
    R(192, 64, 128, BF16, ROW, MAT, CONV_FUSED, N=8),
    # -- d_conv 3 / 2 (separate conv kernel, then the fused x_proj + dt_proj) and conv_bias=False
    R(192, 64, 128, F32, SEQ, MAT, FUSED, W=3),
    R(192, 64, 128, BF16, SEQ, MAT, FUSED, W=3),
    R(4, 64, 128, F32, ROW, MAT, FUSED, W=2),
    R(192, 64, 128, F32, SEQ, MAT, CONV_FUSED, bias=False),
    R(192, 64, 128, BF16, SEQ, SCAN, CONV_FUSED, bias=False),
]


def _row_id(r):
    s = f"B{r['B']}-L{r['L']}-d{r['d']}-{'f32' if r['dtype'] == F32 else 'bf16'}"
    s += "" if r["N"] == 16 else f"-N{r['N']}"
    s += "" if r["W"] == 4 else f"-W{r['W']}"
    s += "" if r["bias"] else "-nobias"
    return s + ("-det" if r["det"] else "")


def _problem(B, L, d, N, W, bias):
    """Weights (as an fp32 CPU oracle module), input and output gradient of one shape, from a seed of the shape.  dout
    is exactly representable in bf16, so one float64 reference serves the fp32 and the bf16 rows."""
    torch.manual_seed(1000 * d + 10 * L + N + W + B)
    ref = scan_ref.MambaRef(d, d_state=N, d_conv=W, conv_bias=bias)
    with torch.no_grad():                           # off the init's special values (equal A_log rows, D = 1)
        ref.A_log.add_(0.1 * torch.randn_like(ref.A_log))
        ref.D.add_(0.1 * torch.randn_like(ref.D))
    h = torch.randn(B, L, d)
    dout = torch.randn(B, L, d).to(BF16).float()
    return ref, h, dout


@functools.lru_cache(maxsize=2)
def _reference(B, L, d, N, W, bias):
    """The float64 reference of one shape and, against it, the scaled errors of the fp32 and of the bf16-autocast CPU
    oracles: shared by the fp32, bf16 and deterministic rows of that shape."""
    ref, h, dout = _problem(B, L, d, N, W, bias)
    want = _oracle(ref, h, dout, f64=True)
    return ref, h, dout, want, {}


def _e_ref(B, L, d, N, W, bias, dtype):
    ref, h, dout, want, cache = _reference(B, L, d, N, W, bias)
    if dtype not in cache:
        got = _oracle(ref, h, dout, io_dtype=None if dtype == F32 else BF16)
        cache[dtype] = {k: scaled_err(got[k], want[k]) for k in want}
    return cache[dtype]


def _device_run(r, ref, h, dout, device):
    from si_mamba_amd import Mamba
    m = Mamba(r["d"], d_state=r["N"], d_conv=r["W"], conv_bias=r["bias"]).to(device)
    m.load_state_dict(ref.state_dict())
    hd = h.to(device).requires_grad_(True)
    _lib.counters.clear()
    with torch.autocast("cuda", dtype=BF16, enabled=r["dtype"] == BF16):
        out = m(hd)
    assert out.dtype == r["dtype"]
    out.backward(dout.to(device).to(out.dtype))
    torch.cuda.synchronize()
    res = {"out": out.detach().float().cpu(), "hidden": hd.grad.cpu()}
    res.update({k: p.grad.cpu() for k, p in m.named_parameters()})
    return res, dict(_lib.counters)


def _expected_counters(r):
    want = {"scan_ckpt_seq" if r["ckpt"] == SEQ else "scan_ckpt_row": 1, r["xdt"]: 1,
            "scan_bwd_det" if r["det"] else "scan_bwd_atomic": 1, "conv1d_bwd_det" if r["det"] else "conv1d_bwd_atomic": 1}
    if r["delta"] == SCAN:
        want["scan_dt_fwd"] = 1
    return want


_RESULTS = {}


@pytest.fixture(scope="module", autouse=True)
def _record_results():
    yield
    path = os.environ.get("SIMAMBA_MIXER_ROUTES_JSON")
    if path and _RESULTS:
        with open(path, "w") as fh:
            json.dump({"metric": "[max |got - want| / max |want|, rms(got - want) / rms(want)] against the float64 "
                                 "mixer; E_ref: the fp32 (fp32 rows) / bf16-autocast (bf16 rows) CPU oracle, E_dev: "
                                 "the device", "rows": _RESULTS}, fh, indent=1)
            fh.write("\n")


def test_table_covers_every_row_kind():
    """The table keeps at least one row of every kind it was written for (review aid: a row cannot quietly go)."""
    def has(**kw):
        return any(all(r[k] == v for k, v in kw.items()) for r in ROWS)
    above = [r for r in ROWS if r["B"] * 2 * r["d"] >= 49152]
    assert 25 <= len(ROWS) and all(r["L"] <= 208 for r in above)
    for d in (128, 384, 64, 192, 96, 160, 32, 448, 576, 200):
        assert any(r["d"] == d for r in above), d
    for L in (16, 20, 66, 68, 132, 208):
        assert any(r["L"] == L for r in above) and any(r["L"] == L and r not in above for r in ROWS), L
    assert has(B=191, d=128) and has(B=192, d=128) and has(N=8) and has(W=3) and has(bias=False)
    det = {(r["ckpt"], r["delta"], r["dtype"]) for r in ROWS if r["det"]}
    assert {(SEQ, MAT, F32), (SEQ, SCAN, BF16), (ROW, MAT, F32), (ROW, MAT, BF16)} <= det
    assert all(has(**{**r, "det": False}) for r in ROWS if r["det"] and r["B"] > 8)


@pytest.mark.parametrize("r", ROWS, ids=_row_id)
def test_mixer_route(r, device):
    torch.backends.cuda.matmul.allow_tf32 = False
    key = (r["B"], r["L"], r["d"], r["N"], r["W"], r["bias"])
    ref, h, dout, want, _ = _reference(*key)
    e_ref = _e_ref(*key, r["dtype"])
    _lib.set_deterministic(True if r["det"] else None)
    try:
        got, counters = _device_run(r, ref, h, dout, device)
        again = _device_run(r, ref, h, dout, device)[0] if r["det"] else None
    finally:
        _lib.set_deterministic(None)

    # the route this row is about was the one taken
    seen = {k: v for k, v in counters.items() if k != "in_proj_hand"}
    assert seen == _expected_counters(r), (seen, _expected_counters(r))
    if r["dtype"] == F32:
        assert "in_proj_hand" not in counters

    if again is not None:                         # deterministic: bitwise-equal gradients from two whole runs
        for k in got:
            assert torch.equal(got[k], again[k]), k

    e_dev = {k: scaled_err(got[k], want[k]) for k in want}
    _RESULTS[_row_id(r)] = {"row": {k: (str(v) if k == "dtype" else v) for k, v in r.items()}, "counters": counters,
                            "E_ref": e_ref, "E_dev": e_dev}
    floor = EPS32 if r["dtype"] == F32 else 0.0
    bad = []
    for k in want:
        f = FACTOR_TENSOR.get((r["dtype"], k), FACTOR[r["dtype"]])
        print(f"{_row_id(r)} {k}: E_ref {e_ref[k][0]:.3e} / {e_ref[k][1]:.3e}  E_dev {e_dev[k][0]:.3e} / "
              f"{e_dev[k][1]:.3e}  nerr {nerr(got[k], want[k]):.3e}")
        for i, what in enumerate(("max", "rms")):
            if not e_dev[k][i] <= f * max(e_ref[k][i], floor):
                bad.append((k, what, e_dev[k][i], e_ref[k][i]))
        if not nerr(got[k], want[k]) < NERR[r["dtype"]]:
            bad.append((k, "nerr", nerr(got[k], want[k])))
    assert not bad, bad
