"""GPU: the memory contract of every op, through poisoned, guard-banded buffers (tests/guarded_alloc.py).

Every row of TABLE calls one op through its public Python entry point, forward and backward where it has one, and
returns every tensor its caller can observe.  The test runs a row plain, then twice with every ``torch.empty`` /
``empty_like`` / ``empty_strided`` of the package replaced by a guarded buffer filled with a finite poison (0, then
-12288 / 1) and the inputs copied into guarded buffers as well:

  * the guards of every buffer still hold the poison  -> the call wrote nothing outside what it was handed, and
  * the two poisoned runs and the plain run agree bit for bit -> every element the caller sees was written by the call,
    nothing around an input influenced it, and the op repeats itself.

Rows marked ``bitwise=False`` take a route that accumulates floats with atomics (the row cites the atomic): they run
under the large finite poison 2^100 and are compared with the plain run within the tolerance their own test file uses,
and one more plain run shows the same spread without any poison; the returned tensors no atomic feeds (``exact``) are
held to the same bits there too.

Shapes are the smallest at which the kernels' tails exist: every tiled or packed dimension is no multiple of the tile
and spans more than one.  Where a wrapper refuses such a shape the row takes the nearest one it accepts and says so.
"""
import contextlib
import copy
import glob
import os

import pytest
import torch

import guarded_alloc
from guarded_alloc import LARGE, SENTINEL, ZERO, guarded, place, same_bits
from helpers import nerr
from si_mamba_amd import _lib

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DT = {F32: "f32", BF16: "bf16"}


class Row:
    def __init__(self, name, build, bitwise=True, atomic=None, tol=None, exact=()):
        """``build(device) -> (run, inputs)``.  ``bitwise=False`` goes with ``atomic`` (file:line of the float atomic on
        the row's route), ``tol`` ((quoted test file, nerr bound)) and ``exact``: the positions in the returned tuple of
        the tensors no atomic feeds, which stay bit for bit."""
        assert bitwise or (atomic and tol)
        self.name, self.build, self.bitwise, self.atomic, self.tol = name, build, bitwise, atomic, tol
        self.exact = tuple(exact)


TABLE = []


def row(name, **kw):
    def add(build):
        TABLE.append(Row(name, build, **kw))
        return build
    return add


def _gen(seed):
    return torch.Generator().manual_seed(seed)


_PLACED = [0]       # guarded buffers a row's run made for its module's parameters (inputs, not allocations of the op)


def _place_module(m):
    """Inside a guarded context: ``m``'s parameters and buffers rebound to guarded copies, so that what lies around
    the weights is poison too.  Outside one: ``m`` as it is."""
    if guarded_alloc._active:
        for t in list(m.parameters()) + list(m.buffers()):
            t.data = place(t.data)
            _PLACED[0] += 1
    return m


def _leaf(*ts):
    return [t.requires_grad_(True) for t in ts]


def _grads(*ts):
    return tuple(t.grad for t in ts)


# ---- mixer core ------------------------------------------------------------------------------------------------------
CONV_ATOMIC = "si_mamba_amd/csrc/conv1d.hip: conv_bwd_reduce, the atomicAdd into p.dw and into p.dbias"
CONV_TOL = ("tests/test_gpu_conv.py: nerr < 1e-3 (fp32), 1e-2 (bf16)", {F32: 1e-3, BF16: 1e-2})
# the scan backward the row's checkpoint step selects, and the conv1d backward behind it
SCAN_ATOMIC = {"row": "si_mamba_amd/csrc/scan_bwd.hip:233-235 (dA, dD, ddelta_bias), :270 (dB, dC); "
                      "conv1d.hip: conv_bwd_reduce (dw, dbias)",
               "seq": "si_mamba_amd/csrc/scan_bwd_seq.hip:521 (ddelta_bias), :558 (dB, dC), :575-576 (dA, dD); "
                      "conv1d.hip: conv_bwd_reduce (dw, dbias)"}
MIXER_TOL = ("tests/test_gpu_mixer_routes.py: NERR = 1e-3 (fp32), 1e-2 (bf16)", {F32: 1e-3, BF16: 1e-2})


def _conv_row(b, d, L, W, dtype, det):
    def build(device):
        g = _gen(b * 100 + d + L + W)
        inputs = (torch.randn(b, d, L, generator=g).to(dtype), torch.randn(d, W, generator=g),
                  torch.randn(d, generator=g), torch.randn(b, d, L, generator=g).to(dtype))

        def run(x, w, bias, dout):
            from si_mamba_amd import causal_conv1d_fn
            _leaf(x, w, bias)
            with _lib.deterministic(det):
                out = causal_conv1d_fn(x, w, bias, "silu")
                out.backward(dout)
            return (out.detach(),) + _grads(x, w, bias)
        return run, inputs
    name = f"conv1d-{b}x{d}x{L}-W{W}-{DT[dtype]}" + ("" if det else "-atomic")
    if det:
        TABLE.append(Row(name, build))
    else:
        # out is the forward; dx is one sum per element, in a fixed order: only dw and dbias are accumulated atomically
        TABLE.append(Row(name, build, bitwise=False, atomic=CONV_ATOMIC, tol=(CONV_TOL[0], CONV_TOL[1][dtype]),
                         exact=(0, 1)))


for _dt in (F32, BF16):
    # (2, 8, 8, 4): aligned rows, the pipelined backward
    for _s in ((2, 33, 50, 3), (1, 7, 1, 2), (2, 8, 8, 4)):
        _conv_row(*_s, _dt, True)
    _conv_row(2, 33, 50, 3, _dt, False)

# (name, forward variant, checkpoint step, L per dtype): the row scan takes any L; the lanes-per-channel kernels want
# L % 4 == 0 in fp32 and L % 8 == 0 in bf16 (simamba_scan_seq_applicable), so they get the nearest ragged-chunk lengths:
# 68 / 72 with 16-step checkpoints, 132 / 136 (two 128-step chunks) where a lanes-per-channel forward writes the
# row-scan backward's checkpoints -- the pair the plan picks when the forward's shape rule passes and the backward's
# does not.  SCAN_MIX is never the library's own choice (SCAN_AUTO); as an explicit variant it launches at (2, 128)
# with every channel on four lanes (scan_fwd_seq_mix_c4), and gets a row with either checkpoint layout.
SCAN_ROUTES = [("row", _lib.SCAN_ROWSCAN, _lib.CKPT_ROW, {F32: 50, BF16: 50}),
               ("auto-ckpt-row", _lib.SCAN_AUTO, _lib.CKPT_ROW, {F32: 134, BF16: 134}),
               ("lpc2-ckpt-seq", _lib.SCAN_LPC2, _lib.CKPT_SEQ, {F32: 68, BF16: 72}),
               ("lpc4-ckpt-seq", _lib.SCAN_LPC4, _lib.CKPT_SEQ, {F32: 68, BF16: 72}),
               ("lpc2-ckpt-row", _lib.SCAN_LPC2, _lib.CKPT_ROW, {F32: 132, BF16: 136}),
               ("lpc4-ckpt-row", _lib.SCAN_LPC4, _lib.CKPT_ROW, {F32: 132, BF16: 136}),
               ("mix-ckpt-seq", _lib.SCAN_MIX, _lib.CKPT_SEQ, {F32: 68, BF16: 72}),
               ("mix-ckpt-row", _lib.SCAN_MIX, _lib.CKPT_ROW, {F32: 132, BF16: 136})]


def _scan_row(tag, variant, ckpt, L, dtype):
    B, D, N = 2, 128, 16             # tests/test_gpu_scan_regimes.py's (batch, dim, N)

    def build(device):
        g = _gen(L + N)
        inputs = (torch.randn(B, D, L, generator=g).to(dtype), (0.5 * torch.randn(B, D, L, generator=g)).to(dtype),
                  -torch.rand(D, N, generator=g) - 0.5, torch.randn(B, N, L, generator=g).to(dtype),
                  torch.randn(B, N, L, generator=g).to(dtype), torch.randn(D, generator=g),
                  torch.randn(B, D, L, generator=g).to(dtype), 0.1 * torch.randn(D, generator=g),
                  torch.randn(B, D, L, generator=g).to(dtype))

        def run(u, delta, A, Bm, Cm, Dv, z, bias, dout):
            from si_mamba_amd import selective_scan_fn
            _leaf(u, delta, A, Bm, Cm, Dv, z, bias)
            before = dict(_lib.counters)
            with _lib.deterministic(True), _lib.scan_variant(variant), _lib.scan_ckpt(ckpt):
                out, last = selective_scan_fn(u, delta, A, Bm, Cm, Dv, z=z, delta_bias=bias, delta_softplus=True,
                                              return_last_state=True)
                out.backward(dout)
            key = "scan_ckpt_seq" if ckpt == _lib.CKPT_SEQ else "scan_ckpt_row"
            assert _lib.counters.get(key, 0) == before.get(key, 0) + 1, "the plan did not take the row's route"
            return (out.detach(), last) + _grads(u, delta, A, Bm, Cm, Dv, z, bias)
        return run, inputs
    TABLE.append(Row(f"scan-{tag}-L{L}-{DT[dtype]}", build))


for _dt in (F32, BF16):
    for _tag, _v, _c, _L in SCAN_ROUTES:
        _scan_row(_tag, _v, _c, _L[_dt], _dt)


def _mixer_rows():
    """One row per distinct route of test_gpu_mixer_routes.ROWS, at that table's smallest row for the route."""
    from test_gpu_mixer_routes import ROWS, _row_id
    best = {}
    for r in ROWS:
        key = (r["dtype"], r["ckpt"], r["delta"], r["xdt"], r["det"])
        size = r["B"] * r["L"] * r["d"]
        if key not in best or size < best[key][0]:
            best[key] = (size, r)
    return [(r, _row_id(r)) for _, r in best.values()]


def _mixer_row(r, rid):
    def build(device):
        from si_mamba_amd import Mamba
        torch.manual_seed(r["d"] + r["L"])
        cpu = Mamba(r["d"], d_state=r["N"], d_conv=r["W"], conv_bias=r["bias"])
        g = _gen(r["B"] + r["L"])
        inputs = (torch.randn(r["B"], r["L"], r["d"], generator=g), torch.randn(r["B"], r["L"], r["d"], generator=g))

        def run(h, dout):
            from test_gpu_mixer_routes import _expected_counters
            m = _place_module(copy.deepcopy(cpu).to(device))
            _leaf(h)
            before = dict(_lib.counters)
            with _lib.deterministic(True if r["det"] else None):
                with torch.autocast("cuda", dtype=BF16, enabled=r["dtype"] == BF16):
                    out = m(h)
                out.backward(dout.to(out.dtype))
            took = {k: _lib.counters.get(k, 0) - before.get(k, 0) for k in _expected_counters(r)}
            assert took == _expected_counters(r), f"not the row's route: {took}"
            grads = dict((k, p.grad) for k, p in m.named_parameters())
            return (out.detach(), grads.pop("out_proj.weight"), h.grad) + tuple(grads.values())
        return run, inputs
    if r["det"]:
        TABLE.append(Row("mamba-" + rid, build))
    else:
        # out is the forward, and out_proj's weight gradient the product of dout with the forward's y: no atomic feeds
        # either.  dB / dC (atomic) reach everything upstream of x_proj, the input gradient included.
        TABLE.append(Row("mamba-" + rid, build, bitwise=False, atomic=SCAN_ATOMIC[r["ckpt"]],
                         tol=(MIXER_TOL[0], MIXER_TOL[1][r["dtype"]]), exact=(0, 1)))


for _r, _rid in _mixer_rows():
    _mixer_row(_r, _rid)


def _in_proj_row(B, L, C, M, dtype):
    def build(device):
        g = _gen(L + C)
        inputs = (torch.randn(B, L, C, generator=g).to(dtype), (torch.randn(M, C, generator=g) / C ** 0.5).to(dtype),
                  torch.randn(B, M, L, generator=g).to(dtype))

        def run(h, w, dxz):
            from si_mamba_amd.mamba_inner import in_proj_fn
            _leaf(h, w)
            before = _lib.counters.get("in_proj_hand", 0)
            with _lib.hand_in_proj(True):
                xz = in_proj_fn(h, w)
                xz.backward(dxz)
            assert _lib.counters.get("in_proj_hand", 0) > before, "not the hand route"
            return (xz.detach(),) + _grads(h, w)
        return run, inputs
    TABLE.append(Row(f"in_proj-{B}x{L}x{C}x{M}-{DT[dtype]}", build))


def _xdt_row(B, D, L, dtype, conv):
    R, N = max(4, D // 32), 16

    def build(device):
        g = _gen(D + L)
        inputs = (torch.randn(B, D, L, generator=g).to(dtype),
                  (torch.randn(R + 2 * N, D, generator=g) / D ** 0.5).to(dtype),
                  (torch.randn(D, R, generator=g) / R ** 0.5).to(dtype), torch.randn(D, 4, generator=g),
                  torch.randn(D, generator=g))

        def run(x, wx, wdt, cw, cb):
            from si_mamba_amd.mamba_inner import xdt_proj_fused_ok, xdt_proj_fwd
            assert xdt_proj_fused_ok(x, wx, wdt, conv=conv)
            out = torch.empty(B, D, L, device=x.device, dtype=dtype) if conv else None
            x_dbl, delta = xdt_proj_fwd(x, wx, wdt, conv=(cw, cb, out) if conv else None)
            return (x_dbl, delta) + ((out,) if conv else ())
        return run, inputs
    TABLE.append(Row(f"xdt_proj-{B}x{D}x{L}-{DT[dtype]}" + ("-conv" if conv else ""), build))


for _dt in (F32, BF16):
    _in_proj_row(3, 72, 128, 512, _dt)
    _in_proj_row(2, 264, 64, 64, _dt)             # the hand kernel wants L % 8 == 0 (in_proj_hand_ok): 260 -> 264
    for _conv in (False, True):
        # the bf16 kernels read packs of 8 along L (xdt_proj_fused_ok): (1, 64, 4) -> (1, 64, 8), (3, 256, 68) -> 72
        _xdt_row(1, 64, 4 if _dt == F32 else 8, _dt, _conv)
        _xdt_row(3, 256, 68 if _dt == F32 else 72, _dt, _conv)


def _add_norm_row(shape, dtype, rms, mode):
    def build(device):
        B, d = shape[0], shape[-1]
        g = _gen(d + B + len(mode))
        inputs = (torch.randn(shape, generator=g).to(dtype), torch.randn(shape, generator=g),
                  (torch.rand(B, generator=g) > 0.3).float() / 0.7, 1 + 0.1 * torch.randn(d, generator=g),
                  0.1 * torch.randn(d, generator=g), torch.randn(shape, generator=g).to(dtype),
                  torch.randn(shape, generator=g))

        def run(h, res, rs, w, b, dn, dro):
            from si_mamba_amd.add_norm import add_layer_norm_fn, add_rms_norm_fn
            res = res if mode != "nores" else None
            rs = rs if mode == "res-rowscale" else None
            leaves = _leaf(*[t for t in (h, res, w, None if rms else b) if t is not None])
            if rms:
                normed, ro = add_rms_norm_fn(h, res, w, rowscale=rs, out_dtype=dtype)
            else:
                normed, ro = add_layer_norm_fn(h, res, w, b, rowscale=rs, out_dtype=dtype)
            torch.autograd.backward([normed, ro], [dn, dro])
            return (normed.detach(), ro.detach()) + _grads(*leaves)
        return run, inputs
    TABLE.append(Row(f"add_{'rms' if rms else 'ln'}-{'x'.join(map(str, shape))}-{DT[dtype]}-{mode}", build))


for _shape in ((5, 1, 36), (3, 50, 128)):
    for _dt in (F32, BF16):
        for _rms in (False, True):
            for _mode in ("res-rowscale", "res", "nores"):
                _add_norm_row(_shape, _dt, _rms, _mode)


def _out_norm_row(B, C, L):
    D = 2 * C

    def build(device):
        g = _gen(C + L)
        inputs = (torch.randn(B, D, L, generator=g).to(BF16), (torch.randn(C, D, generator=g) / D ** 0.5),
                  torch.randn(B, L, C, generator=g), (torch.rand(B, generator=g) > 0.3).float() / 0.7,
                  1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g),
                  torch.randn(B, L, C, generator=g).to(BF16), torch.randn(B, L, C, generator=g))

        def run(y, ow, res, rs, lw, lb, dn, dro):
            from si_mamba_amd.out_norm import out_proj_add_ln_fn, out_proj_add_ln_ok
            assert out_proj_add_ln_ok(y, ow, C)
            _leaf(y, ow, res, lw, lb)
            normed, ro = out_proj_add_ln_fn(y, ow, res, lw, lb, rowscale=rs)
            torch.autograd.backward([normed, ro], [dn, dro])
            return (normed.detach(), ro.detach()) + _grads(y, ow, res, lw, lb)
        return run, inputs
    TABLE.append(Row(f"out_proj_add_ln-{B}x{C}x{L}", build))


_out_norm_row(1, 128, 64)
_out_norm_row(2, 256, 136)


def _seq_gather_row(B, C, G, R, dtype):
    def build(device):
        g = _gen(G + R)
        idx = torch.cat([torch.stack([torch.randperm(G, generator=g) for _ in range(B)]) for _ in range(R)], 1)
        inputs = (torch.randn(B, C, G, generator=g).to(dtype), idx.to(torch.int32),
                  torch.randn(B, C, G * R, generator=g).to(dtype))

        def run(x, idx32, dout):
            from si_mamba_amd.seq_expand import expansion_len_ok, inverse_positions, seq_gather_last
            assert expansion_len_ok(x.transpose(1, 2), G * R)
            inv32 = inverse_positions(idx32.long(), G)
            _leaf(x)
            out = seq_gather_last(x, idx32, inv32)
            out.backward(dout)
            return out.detach(), x.grad
        return run, inputs
    TABLE.append(Row(f"seq_gather-{B}x{C}x{G}x{R}-{DT[dtype]}", build))


def _cross_merge_row(B, G, k, C, dtype):
    def build(device):
        g = _gen(G + k)
        order = torch.stack([torch.stack([torch.randperm(G, generator=g) for _ in range(k)]) for _ in range(B)])
        inputs = (torch.randn(B, 2 * k * G, C, generator=g).to(dtype), order,
                  torch.randn(B, 2 * k * G, C, generator=g).to(dtype))

        def run(h, order, dout):
            from si_mamba_amd.cross_merge import cross_merge, cross_merge_maps
            _leaf(h)
            out = cross_merge(h, cross_merge_maps(order))
            out.backward(dout)
            return out.detach(), h.grad
        return run, inputs
    TABLE.append(Row(f"cross_merge-{B}x{G}x{k}x{C}-{DT[dtype]}", build))


for _dt in (F32, BF16):
    _seq_gather_row(2, 5, 12, 3, _dt)
    _seq_gather_row(1, 4, 256, 8, _dt)
    _cross_merge_row(3, 37, 3, 36, _dt)


# ---- encoder ---------------------------------------------------------------------------------------------------------
def _bn_row(rows, C, group, dtype, training):
    def build(device):
        g = _gen(rows + C + group)
        gt = torch.randn(rows // group, C, generator=g) if group else torch.zeros(0)
        inputs = (torch.randn(rows, C, generator=g).to(dtype), gt, 1 + 0.1 * torch.randn(C, generator=g),
                  0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g),
                  0.5 + torch.rand(C, generator=g), torch.randn(rows, C, generator=g).to(dtype))

        def run(x, gt, w, b, rm, rv, dy):
            from si_mamba_amd.encoder_ops import bn_relu_fn
            bn = torch.nn.BatchNorm1d(C).to(x.device)
            bn.train(training)
            # the module's parameters and running buffers ARE the placed tensors: the kernels update them in place
            bn.weight, bn.bias = torch.nn.Parameter(w), torch.nn.Parameter(b)
            bn.running_mean, bn.running_var = rm, rv
            gterm = _leaf(gt)[0] if group else None
            _leaf(x)
            y = bn_relu_fn(x, bn, gterm=gterm, group=group)
            y.backward(dy)
            return (y.detach(), bn.running_mean, bn.running_var, x.grad, bn.weight.grad, bn.bias.grad) + \
                ((gterm.grad,) if group else ())
        return run, inputs
    TABLE.append(Row(f"bn_relu-{rows}x{C}-g{group}-{DT[dtype]}-{'train' if training else 'eval'}", build))


for _dt in (F32, BF16):
    for _train in (True, False):
        for _s in ((1000, 96, 0), (768, 384, 16), (512, 1280, 256)):      # 1280 channels: the two-slice path
            _bn_row(*_s, _dt, _train)


def _group_max_row(dtype):
    def build(device):
        g = _gen(17)
        inputs = (torch.randn(10, 17, 36, generator=g).to(dtype), torch.randn(10, 36, generator=g).to(dtype))

        def run(x, dout):
            from si_mamba_amd.encoder_ops import group_max_fn
            _leaf(x)
            out = group_max_fn(x)
            out.backward(dout)
            return out.detach(), x.grad
        return run, inputs
    TABLE.append(Row(f"group_max-10x17x36-{DT[dtype]}", build))


def _max_linear_row(dtype):
    groups, n, cin, cout = 6, 17, 64, 36

    def build(device):
        g = _gen(cin + cout)
        inputs = (torch.randn(groups * n, cin, generator=g).to(dtype),
                  (torch.randn(cout, cin, generator=g) / 8).to(dtype), (0.1 * torch.randn(cout, generator=g)).to(dtype),
                  torch.randn(groups, cout, generator=g).to(dtype))

        def run(x, w, b, dout):
            from si_mamba_amd.encoder_ops import token_linear_group_max
            _leaf(x, w, b)
            before = _lib.counters.get("max_linear_sparse", 0)
            with _lib.sparse_max_linear(True):
                out = token_linear_group_max(x, w, b, n)
            assert _lib.counters.get("max_linear_sparse", 0) == before + 1, "not the sparse route"
            out.backward(dout)
            return (out.detach(),) + _grads(x, w, b)
        return run, inputs
    TABLE.append(Row(f"max_linear_sparse-6x17x64x36-{DT[dtype]}", build))


for _dt in (F32, BF16):
    _group_max_row(_dt)
    _max_linear_row(_dt)


# ---- geometry and ordering -------------------------------------------------------------------------------------------
def _fps_knn_row(ragged):
    B, N, K = 3, 300, 37

    def build(device):
        g = _gen(N + K)
        inputs = (torch.randn(B, N, 3, generator=g), torch.tensor([300, 123, 20]))

        def run(pts, lengths):
            from si_mamba_amd import grouping
            ln = lengths if ragged else None
            centers, idx = grouping.sample_farthest_points(pts, K, lengths=ln)
            cl = lengths.clamp(max=K) if ragged else None
            nn_idx = grouping.knn_group(centers, pts, 17, lengths=ln, center_lengths=cl)
            return centers, idx, nn_idx
        return run, inputs
    TABLE.append(Row("fps-knn-3x300-K37-k17" + ("-ragged" if ragged else ""), build))


_fps_knn_row(False)
_fps_knn_row(True)


def _interp_row(B, N, S, C, dtype):
    def build(device):
        g = _gen(N + S)
        inputs = (torch.randn(B, N, 3, generator=g), torch.randn(B, S, 3, generator=g),
                  torch.randn(B, S, C, generator=g).to(dtype), torch.randn(B, N, C, generator=g).to(dtype))

        def run(xyz1, xyz2, feats, dout):
            from si_mamba_amd import interp
            idx, w = interp.three_nn(xyz1, xyz2)
            _leaf(feats)
            out = interp.three_interpolate(feats, idx, w)
            out.backward(dout)
            return idx, w, out.detach(), feats.grad
        return run, inputs
    TABLE.append(Row(f"three_nn-interp-{B}x{N}x{S}x{C}-{DT[dtype]}", build))


for _dt in (F32, BF16):
    _interp_row(2, 300, 37, 36, _dt)
    _interp_row(2, 256, 2, 8, _dt)            # fewer than three centres: the last index repeats

GRAPH = dict(k=20, alpha=10.0, symmetric=True, self_loop=False, binary=True)     # the ordering the model runs


def _spectral_rows(G, knn):
    from si_mamba_amd.synthetic import unit_ball_centers
    kw = dict(GRAPH, k=knn)
    k = min(4, G - 1)

    def graph(device):
        def run(c):
            from si_mamba_amd import spectral
            return (spectral.create_graph_from_feature_space_gpu_weighted_adjacency(c, **kw),)
        return run, (unit_ball_centers(2, G, 3),)

    def jacobi(device):
        def run(c):
            from si_mamba_amd import spectral
            adj = spectral.create_graph_from_feature_space_gpu_weighted_adjacency(c, **kw)
            return spectral.calc_top_k_eigenvalues_eigenvectors(adj, k, True)
        return run, (unit_ball_centers(2, G, 3),)

    def tridiag(device):
        def run(c):
            from si_mamba_amd import spectral
            adj = spectral.create_graph_from_feature_space_gpu_weighted_adjacency(c, **kw)
            vals, vecs, _, _, order = spectral._eig(adj, k, True, False, want_all=False, want_order=True)
            return vals, vecs, order
        return run, (unit_ball_centers(2, G, 3),)

    def order(device):
        def run(c):
            from si_mamba_amd import spectral
            return spectral.spectral_order(c, knn, 10.0, k, smallest=True, symmetric=True, self_loop=False, binary=True)
        return run, (unit_ball_centers(2, G, 3),)

    def large(device):
        def run(c):
            from si_mamba_amd import spectral
            adj = spectral.create_graph_from_feature_space_gpu_weighted_adjacency(c, **kw)
            before = _lib.counters.get("spectral_large_g", 0)
            with _lib.spectral_large_g():
                vals, vecs, _, _, order = spectral._eig(adj, k, True, False, want_all=False, want_order=True)
            assert _lib.counters.get("spectral_large_g", 0) == before + 1
            return vals, vecs, order
        return run, (unit_ball_centers(2, G, 3),)
    return dict(graph=graph, jacobi=jacobi, tridiag=tridiag, order=order, large=large)


for _G in (37, 128):
    for _name, _b in _spectral_rows(_G, 20).items():
        if _name != "large":
            TABLE.append(Row(f"spectral-{_name}-G{_G}", _b))
# the large-G kernel forced below 129 patches: G = 3 is the smallest it takes (a single reflector,
# tests/test_gpu_spectral_large.py), G = 37 an odd width with tails
TABLE.append(Row("spectral-large-forced-G3", _spectral_rows(3, 2)["large"]))
TABLE.append(Row("spectral-large-forced-G37", _spectral_rows(37, 20)["large"]))


@row("argsort_rows-5x37")
def _argsort(device):
    def run(v):
        from si_mamba_amd import spectral
        return (spectral.argsort_rows(v),)
    return run, (torch.randn(5, 37, generator=_gen(5)),)


# ---- losses, metrics, data -------------------------------------------------------------------------------------------
def _chamfer_row(name, n, m, **kw):
    pairs = 3

    def build(device):
        g = _gen(n + m)
        # ragged: lengths on both sides of a 1024-target tile, a whole set and a single point
        inputs = (torch.randn(pairs, n, 3, generator=g), torch.randn(pairs, m, 3, generator=g),
                  torch.rand(pairs, generator=g) + 0.5, torch.tensor([n, min(n, 1025), 1]),
                  torch.tensor([min(m, 1023), m, 2]))

        def run(p, q, dd, xl, yl):
            from si_mamba_amd.chamfer import chamfer_distance
            before = dict(_lib.counters)
            extra = dict(x_lengths=xl, y_lengths=yl) if name == "ragged" else {}
            if name == "patch":
                _leaf(p)
            else:
                _leaf(p, q)
            dist = chamfer_distance(p, q, **extra, **kw)
            key = {"patch": "chamfer_small", "whole": "chamfer_large", "ragged": "chamfer_ragged"}[name]
            assert _lib.counters.get(key, 0) == before.get(key, 0) + 1, "not the row's kernel family"
            dist.backward(dd)
            return (dist.detach(), p.grad) + (() if name == "patch" else (q.grad,))
        return run, inputs
    TABLE.append(Row(f"chamfer-{name}-{n}x{m}", build))


_chamfer_row("patch", 32, 27)
# chamfer_large.hip stages kChTile = 1024 targets per LDS tile and a workgroup owns a multiple of 256 queries; each set
# is the other direction's targets, so both cross 1024 with a partial last tile (tests/test_gpu_chamfer_ragged.py's
# boundaries: 64, 256 Q, 1024)
_chamfer_row("whole", 1301, 1030)
_chamfer_row("ragged", 1301, 1030, norm=1, point_reduction="sum")


@row("emd-3x37")          # earth_movers_distance takes equal set sizes only: 37 against 37
def _emd(device):
    g = _gen(37)
    inputs = (torch.randn(3, 37, 3, generator=g), torch.randn(3, 37, 3, generator=g), torch.rand(3, generator=g) + 0.5)

    def run(x, y, dd):
        from si_mamba_amd.emd import earth_movers_distance
        _leaf(x, y)
        dist, assign, rounds, conv = earth_movers_distance(x, y, return_assignment=True)
        dist.backward(dd)
        return (dist.detach(), assign, rounds, conv) + _grads(x, y)
    return run, inputs


def _sinkhorn_row(ragged):
    def build(device):
        g = _gen(58)
        inputs = (torch.randn(3, 37, 3, generator=g), torch.randn(3, 21, 3, generator=g),
                  torch.rand(3, generator=g) + 0.5, torch.tensor([37, 5, 1]), torch.tensor([2, 21, 13]))

        def run(x, y, dd, xl, yl):
            from si_mamba_amd.sinkhorn import sinkhorn_divergence
            _leaf(x, y)
            extra = dict(x_lengths=xl, y_lengths=yl) if ragged else {}
            div, ot, merr = sinkhorn_divergence(x, y, return_info=True, **extra)
            div.backward(dd)
            return (div.detach(), ot, merr) + _grads(x, y)
        return run, inputs
    TABLE.append(Row("sinkhorn-3x37x21" + ("-ragged" if ragged else ""), build))


_sinkhorn_row(False)
_sinkhorn_row(True)


def _part_seg_row(dtype):
    def build(device):
        from si_mamba_amd.seg_metrics import SHAPENETPART
        g = _gen(50)
        B, N, C = 3, 301, SHAPENETPART.num_labels
        cat = torch.tensor([0, 10, 15])
        first = torch.tensor(SHAPENETPART.first)[cat]
        count = torch.tensor(SHAPENETPART.count)[cat]
        target = first[:, None] + (torch.randint(0, 1 << 20, (B, N), generator=g) % count[:, None])
        inputs = (torch.randn(B, N, C, generator=g).to(dtype), target, cat, torch.tensor([301, 130, 1]))

        def run(scores, target, cat, lengths):
            from si_mamba_amd.seg_metrics import part_seg_eval
            return tuple(part_seg_eval(scores, target, cat, lengths=lengths))
        return run, inputs
    TABLE.append(Row(f"part_seg_eval-3x301-ragged-{DT[dtype]}", build))


_part_seg_row(F32)
_part_seg_row(BF16)


@row("svm-ovo-3classes-d37")
def _svm(device):
    g = _gen(37)
    y = torch.arange(90) % 3
    X = torch.randn(90, 37, generator=g) + 1.5 * torch.nn.functional.one_hot(y, 37).float()
    inputs = (X, y, torch.randn(41, 37, generator=g))

    def run(X, y, T):
        from si_mamba_amd.svm import OvOLinearSVC
        clf = OvOLinearSVC(C=0.01).fit(X, y)
        return clf.coef_, clf.intercept_, clf.n_iter_, clf.converged_, clf._alpha, clf.predict(T), clf.predict(X)
    return run, inputs


@row("sample_and_augment-chain-idx-sel")
def _augment(device):
    g = _gen(300)
    inputs = (torch.randn(3, 300, 3, generator=g),
              torch.stack([torch.randperm(300, generator=g)[:101] for _ in range(3)]),
              torch.randperm(101, generator=g)[:37], torch.tensor([37, 20, 1]))

    def run(pts, idx, sel, lengths):
        from si_mamba_amd import transforms as T
        chain = [T.PointcloudRotate(), T.PointcloudScaleAndTranslate(), T.PointcloudJitter(),
                 T.PointcloudRandomInputDropout(), T.RandomHorizontalFlip()]
        state = T.AugmentState(7, pts.device)
        full = T.sample_and_augment(pts, chain, idx=idx, sel=sel, state=state)
        ragged = T.sample_and_augment(pts, chain, idx=idx.to(torch.int32), sel=sel, lengths=lengths, state=state)
        return full, ragged, state.tensor
    return run, inputs


@row("dataset-fetch-and-keyed_perm")
def _dataset(device):
    g = _gen(11)
    inputs = (torch.randn(7, 130, 3, generator=g), torch.arange(7) % 3,
              torch.randint(0, 50, (7, 130), generator=g))

    def run(pts, labels, point_labels):
        from si_mamba_amd import data
        ds = data.DeviceDataset(pts.reshape(-1, 3), None, 130, labels, point_labels.reshape(-1).to(torch.int32))
        loader = data.DeviceLoader(ds, 3, 37, shuffle=True, drop_last=False, subsample="permute",
                                   normalize="unit_sphere", seed=5)
        a, b, c = loader.fetch(), loader.fetch(), loader.fetch()          # the third batch has two empty slots
        perm = torch.from_numpy(data.keyed_perm(7, 5, _lib.DS_STREAM_SHUFFLE))
        return tuple(a) + tuple(b) + tuple(c) + (perm,)
    return run, inputs


# ---- the whole model -------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _torch_deterministic():
    """torch.use_deterministic_algorithms(True) for a block.  The scan and conv1d backward follow it
    (_lib.deterministic_enabled), and so does torch itself: the stack expands the residual of block 0 with torch.gather
    (si_mamba_amd/block.py:372), whose backward is ATen's scatter-add -- float atomics onto 2 k positions per token
    unless this switch is on.  Without it the encoder's and pos_embed's gradients differ in the last bits from one
    plain run to the next."""
    prev = torch.are_deterministic_algorithms_enabled()
    warn_only = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=warn_only)


def _model_row(dtype):
    def build(device):
        from si_mamba_amd.point_mamba import PointMamba, default_config
        from si_mamba_amd.synthetic import surface_clouds
        torch.manual_seed(0)
        cfg = default_config(trans_dim=64, encoder_dims=64, depth=2, num_group=32, group_size=16, cls_dim=5,
                             drop_path=0., knn_graph=8)
        cpu = PointMamba(cfg).train()
        for mod in cpu.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        inputs = (surface_clouds(3, 256, 2), torch.tensor([0, 3, 4]))

        def run(pts, gt):
            m = _place_module(copy.deepcopy(cpu).to(device))
            torch.manual_seed(1)
            with _torch_deterministic():
                with torch.autocast("cuda", dtype=BF16, enabled=dtype == BF16):
                    logits = m(pts)
                    loss = torch.nn.functional.cross_entropy(logits.float(), gt)
                loss.backward()
            grads = tuple(p.grad for p in m.parameters() if p.grad is not None)
            assert grads
            return (logits.detach(),) + grads
        return run, inputs
    TABLE.append(Row(f"point_mamba-train-step-{DT[dtype]}", build))


_model_row(F32)
_model_row(BF16)


# ---- the test --------------------------------------------------------------------------------------------------------
# row name -> (guarded allocations of its least-allocating context, the package's files on their stacks)
_SEEN = {}


def _to_device(inputs, device, guard):
    out = []
    for t in inputs:
        d = t.to(device)
        out.append(place(d) if guard else d.clone())
    return out


def _plain(r, device):
    run, inputs = r.build(device)
    out = run(*_to_device(inputs, device, False))
    torch.cuda.synchronize()
    return run, inputs, out


def _guarded_run(r, run, inputs, device, poison):
    with guarded(poison) as g:
        placed = _to_device(inputs, device, True)
        n_inputs = len(g.records)
        _PLACED[0] = 0
        out = run(*placed)
        g.verify()
        torch.cuda.synchronize()
    made = len(g.records) - n_inputs - _PLACED[0]
    prev = _SEEN.get(r.name)
    _SEEN[r.name] = (made if prev is None else min(made, prev[0]), g.modules | (prev[1] if prev else set()))
    return out


def _finite(name, outs):
    for i, t in enumerate(outs):
        assert isinstance(t, torch.Tensor), (name, i, type(t))
        if t.dtype.is_floating_point:
            assert bool(torch.isfinite(t).all()), f"{name}: returned tensor {i} is not finite"


@pytest.mark.parametrize("r", TABLE, ids=lambda r: r.name)
def test_memory_contract(r, device):
    tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        _contract(r, device)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = tf32


def _contract(r, device):
    run, inputs, plain = _plain(r, device)
    _finite(r.name, plain)
    poisons = (ZERO, SENTINEL) if r.bitwise else (LARGE, LARGE)
    got = [_guarded_run(r, run, inputs, device, p) for p in poisons]
    assert _SEEN[r.name][0] > 0, "the row allocated nothing through the harness: it tests nothing"
    assert len(got[0]) == len(got[1]) == len(plain)
    if r.bitwise:
        for i, (a, b, p) in enumerate(zip(got[0], got[1], plain)):
            assert same_bits(a, b), f"{r.name}: returned tensor {i} differs between the two poisons"
            assert same_bits(a, p), f"{r.name}: returned tensor {i} differs between the poisoned and the plain run"
        return
    # a float-atomic route (r.atomic): within the op's own tolerance (r.tol) of the plain run, poisoned or not
    again = run(*_to_device(inputs, device, False))
    torch.cuda.synchronize()
    for i, (a, b, c, p) in enumerate(zip(got[0], got[1], again, plain)):
        for which, t in (("2^100 poison, first run", a), ("2^100 poison, second run", b), ("plain, second run", c)):
            assert t.shape == p.shape and t.dtype == p.dtype
            if i in r.exact:
                assert same_bits(t, p), f"{r.name}: tensor {i}, which no atomic feeds, differs ({which})"
            elif t.dtype.is_floating_point:
                assert bool(torch.isfinite(t).all()), f"{r.name}: tensor {i} not finite ({which})"
                assert nerr(t, p) < r.tol[1], f"{r.name}: tensor {i} ({which}) against the plain run; {r.tol[0]}"
            else:
                assert torch.equal(t, p), f"{r.name}: tensor {i} ({which})"


def test_the_harness_catches_stand_ins_on_the_device(device):
    """tests/test_guarded_alloc.py's stand-in ops on the device the rows run on: the two-poison comparison flags the
    skipped element and the stray read, verify() the stray write, and a correct op passes all of it."""
    def correct(x, out):
        out.copy_(3 * x)

    def skips_last(x, out):
        out[:-1] = 3 * x[:-1]

    def writes_past(x, out):
        out.as_strided((x.numel() + 1,), (1,), out.storage_offset())[:] = torch.cat([3 * x, x[-1:]])

    def reads_past(x, out):
        out.copy_(3 * x)
        out[-1] += x.as_strided((x.numel() + 1,), (1,), x.storage_offset())[-1]

    def contract(op):
        x = torch.randn(37, generator=_gen(0)).to(device)
        got, guards = [], True
        for poison in (ZERO, SENTINEL):
            with guarded(poison) as g:
                xin, out = place(x), torch.empty(37, device=device)
                assert xin._base is None and out._base is None and out.data_ptr() % 512 == 0 and len(g.records) == 2
                op(xin, out)
                got.append(out)
                try:
                    g.verify()
                except AssertionError:
                    guards = False
        return same_bits(got[0], got[1]), guards
    assert contract(correct) == (True, True)
    assert contract(skips_last) == (False, True)
    assert contract(writes_past) == (True, False)
    assert contract(reads_past) == (False, True)


def _seen(r, device):
    """What the row's guarded contexts saw; a row that has not run yet (a -k selection) runs once, guarded."""
    if r.name not in _SEEN:
        run, inputs = r.build(device)
        _guarded_run(r, run, inputs, device, LARGE if not r.bitwise else SENTINEL)
    return _SEEN[r.name]


def test_every_guarded_context_allocated(device):
    """Non-vacuity: every row's every guarded context handed out at least one buffer besides the placed inputs."""
    empty = [r.name for r in TABLE if _seen(r, device)[0] <= 0]
    assert not empty, empty
    assert len({r.name for r in TABLE}) == len(TABLE)
    assert all((not r.bitwise) == bool(r.atomic) for r in TABLE)


def test_every_module_that_launches_is_reached(device):
    """Every si_mamba_amd/*.py that calls _lib.call had a frame on the stack of a guarded allocation in some row."""
    pkg = os.path.dirname(os.path.abspath(_lib.__file__))
    launching = set()
    for path in glob.glob(os.path.join(pkg, "*.py")):
        with open(path) as fh:
            if "_lib.call(" in fh.read():
                launching.add(os.path.basename(path))
    assert launching
    reached = set()
    for r in TABLE:
        reached |= _seen(r, device)[1]
    assert launching <= reached, sorted(launching - reached)
