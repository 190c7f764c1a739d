"""CPU: the Python scan plan against the library's own accept / refuse logic, swept over what the dispatch depends on.

The sequential (CKPT_SEQ) forward / backward pair refuses operands it cannot read with SIMAMBA_E_VARIANT -- after the
plan has already allocated 16-step checkpoints, so a plan that answers CKPT_SEQ for operands the library refuses is a
RuntimeError on the first training step (Mamba(96) at B = 256: dt_rank = 6 puts B / C off a pack boundary).  That
logic is host code in front of any launch; simamba_scan_seq_applicable states it launch-free, from the predicates the
entry points themselves evaluate.  Nothing here calls an entry point that could launch: addresses are fabricated
integers that only ever meet alignment tests.
"""
import itertools

import pytest
import torch

from si_mamba_amd import _lib

F32, BF16 = torch.float32, torch.bfloat16
BASE = 0x7F0000000000          # a fabricated, 2 MiB-aligned "allocation"
LIM = 1 << 30


def _model(batch, dim, L, N, dtype, softplus, has_z, act_or, a_addr, b_addr, c_addr, z_bs, dz_bs, bc):
    """The preconditions of the sequential pair as include/simamba.h and the comments in csrc/scan_fwd.hip,
    scan_fwd_seq.hip and scan_bwd_seq.hip state them, written out a second time."""
    esz = 4 if dtype == F32 else 2
    z_bs = z_bs or dim * L
    dz_bs = dz_bs or dim * L
    bs, ns, ts = bc if any(bc) else (N * L, L, 1)
    if not (0 < batch <= 65535 and N == 16 and softplus and dim % 64 == 0):
        return False
    if (L * esz) % 16 or act_or % 16 or a_addr % 16:
        return False
    if has_z and ((z_bs * esz) % 16 or (dz_bs * esz) % 16):
        return False
    if batch * dim * L >= LIM or batch * z_bs >= LIM or (has_z and batch * dz_bs >= LIM):
        return False
    pack_bytes = 4 * esz                                    # B / C are read in packs of 4 elements
    if b_addr % pack_bytes or c_addr % pack_bytes or bs % 4:
        return False
    if not ((ts == 1 and ns % 4 == 0) or (ns == 1 and ts % 4 == 0)):
        return False
    return ns >= 0 and ts >= 0 and 15 * ns + (L - 1) * ts < LIM


def _query(batch, dim, L, N, dtype, softplus, has_z, act_or, a_addr, b_addr, c_addr, z_bs, dz_bs, bc):
    return bool(_lib.load().simamba_scan_seq_applicable(batch, dim, L, N, _lib.dtype_code(dtype), int(softplus),
                                                        int(has_z), act_or, a_addr, b_addr, c_addr, z_bs, dz_bs, *bc))


def _mixer_cases():
    """(batch, d_inner, L, dt_rank, N, dtype, xz misalignment, A misalignment, z batch stride): the fused mixer's scan
    at every dt_rank residue mod 8, both dtypes, L around the pack sizes, row counts on both sides of the 49 152-row
    line and of the 2^30 bounds, a padded xz (z_bs > 2 d_inner L), and operands off 16 bytes."""
    shapes = [(B, D, L) for D in (64, 128, 192, 320, 400, 832, 1152) for B in (1, 48, 191, 192, 256, 768, 4096, 65535)
              for L in (8, 16, 20, 64, 66, 68, 128, 132, 208, 1024)]
    for (B, D, L), R, N, dtype in itertools.product(shapes, (2, 4, 6, 8, 10, 12, 13, 16, 24, 28, 36), (16, 8), (F32, BF16)):
        yield B, D, L, R, N, dtype, 0, 0, 2 * D * L
    for B, D, L, R in [(256, 192, 64, 12), (256, 256, 64, 8), (768, 64, 64, 2)]:
        for dtype, xo, ao, pad in itertools.product((F32, BF16), (0, 4, 8), (0, 4, 8), (0, 2, 4, 8)):
            yield B, D, L, R, 16, dtype, xo, ao, 2 * D * L + pad
    # batch * z_bs >= 2^30 while batch * dim * L < 2^30 (z_bs = 2 d_inner L in the mixer), and the exact edges
    for B, D, L in [(4096, 1024, 128), (8192, 512, 128), (2048, 1024, 256), (1024, 1024, 512), (8191, 512, 128),
                    (4095, 1024, 128), (16384, 64, 512), (16383, 64, 512), (16384, 64, 1024)]:
        for R, dtype in itertools.product((4, 8, 64), (F32, BF16)):
            yield B, D, L, R, 16, dtype, 0, 0, 2 * D * L


def _mixer_operands(B, D, L, R, N, dtype, xo, ao, z_bs):
    esz = 4 if dtype == F32 else 2
    return _lib.mixer_scan_operands(BASE + xo, BASE + (1 << 21) + ao, D, L, R, N, esz, z_bs)


def test_plan_seq_implies_library_accepts_mixer_operands():
    """Whenever the plan answers CKPT_SEQ for the mixer's operands, the library would accept a sequential forward and
    backward with them -- and the query agrees with the written-out preconditions everywhere in the sweep."""
    seen = {"seq": 0, "row_above_line": 0, "refused_bc": 0, "refused_zbs": 0}
    bad = []
    for case in _mixer_cases():
        B, D, L, R, N, dtype, xo, ao, z_bs = case
        ops = _mixer_operands(*case)
        q = _query(B, D, L, N, dtype, ops["softplus"], ops["has_z"], ops["act_addr_or"], ops["a_addr"], ops["b_addr"],
                   ops["c_addr"], ops["z_bs"], ops["dz_bs"], ops["bc_strides"])
        m = _model(B, D, L, N, dtype, ops["softplus"], ops["has_z"], ops["act_addr_or"], ops["a_addr"], ops["b_addr"],
                   ops["c_addr"], ops["z_bs"], ops["dz_bs"], ops["bc_strides"])
        assert q == m, ("query and documented preconditions disagree", case)
        step = _lib.scan_plan_step(B, D, L, N, dtype, **ops)
        assert step in (_lib.CKPT_SEQ, _lib.CKPT_ROW)
        if step == _lib.CKPT_SEQ:
            seen["seq"] += 1
            if not q:
                bad.append(case)
        elif B * D >= 48 * 1024:
            seen["row_above_line"] += 1
            esz = 4 if dtype == F32 else 2
            if N == 16 and D % 64 == 0 and (L * esz) % 16 == 0 and not xo and not ao:
                seen["refused_bc" if B * z_bs < LIM and B * D * L < LIM else "refused_zbs"] += 1
    assert not bad, f"{len(bad)} operand sets planned CKPT_SEQ that the library refuses, e.g. {bad[:6]}"
    # the sweep reaches what it is about: accepted plans, and both kinds of refusal above the row threshold
    assert seen["seq"] > 500 and seen["refused_bc"] > 500 and seen["refused_zbs"] > 10, seen


def test_plan_of_known_shapes():
    """Pinned answers: the model shapes keep the sequential pair; the shapes of the two crashes plan the row scan."""
    def plan(B, d_model, L, dtype, **kw):
        D, R = 2 * d_model, -(-d_model // 16)
        return _lib.scan_plan_step(B, D, L, 16, dtype, **_mixer_operands(B, D, L, R, 16, dtype, 0, 0,
                                                                          kw.get("z_bs", 2 * D * L)))
    SEQ, ROW = _lib.CKPT_SEQ, _lib.CKPT_ROW
    assert plan(64, 384, 1024, F32) == SEQ and plan(64, 384, 1024, BF16) == SEQ     # the flagship
    assert plan(256, 384, 128, F32) == SEQ and plan(32, 384, 1024, F32) == ROW      # rows: 196 608 / 24 576
    assert plan(192, 128, 64, F32) == SEQ and plan(191, 128, 64, F32) == ROW        # the 49 152-row line
    assert plan(384, 64, 64, F32) == SEQ and plan(384, 64, 64, BF16) == SEQ         # dt_rank 4: 8-byte packs in bf16
    assert plan(256, 96, 64, F32) == ROW and plan(256, 96, 64, BF16) == ROW         # dt_rank 6 (was: RuntimeError)
    assert plan(154, 160, 64, F32) == ROW and plan(768, 32, 64, BF16) == ROW        # dt_rank 10, 2
    assert plan(256, 128, 20, F32) == SEQ and plan(256, 128, 20, BF16) == ROW       # L % 8 == 4
    assert plan(256, 128, 16, F32) == SEQ and plan(256, 128, 66, F32) == ROW
    assert plan(4096, 512, 128, F32) == ROW        # batch * z_bs = 2^30 with batch * dim * L = 2^29 (was: RuntimeError)
    assert plan(4095, 512, 128, F32) == SEQ
    assert plan(256, 128, 64, F32, z_bs=2 * 256 * 64 + 2) == ROW                    # z rows off 16 bytes


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_plan_seq_implies_library_accepts_standalone_scan_operands(dtype):
    """selective_scan_fn's operands: B / C as (B, N, L) time-major or as token-major column views, at every base
    offset and stride residue; A off 16 bytes; z through a batch stride; softplus off."""
    esz = 4 if dtype == F32 else 2
    bad, n_seq = [], 0
    for (B, D, L), off, S, has_z, softplus, ao, layout in itertools.product(
            [(768, 64, 64), (96, 512, 128), (96, 512, 20), (1024, 1024, 1024), (2048, 512, 1024), (96, 520, 64)],
            (0, 2, 4, 6, 8), (32, 34, 36, 40), (True, False), (True, False), (0, 8), ("time", "token")):
        bc = (16 * L, L, 1) if layout == "time" else (L * S, 1, S)
        if layout == "time" and S != 32:
            continue
        ops = dict(softplus=softplus, has_z=has_z, act_addr_or=BASE, a_addr=BASE + ao, b_addr=BASE + off * esz,
                   c_addr=BASE + (off + (16 if layout == "token" else 16 * L * B)) * esz,
                   z_bs=2 * D * L if has_z else 0, dz_bs=0, bc_strides=bc)
        q = _query(B, D, L, 16, dtype, softplus, has_z, ops["act_addr_or"], ops["a_addr"], ops["b_addr"], ops["c_addr"],
                   ops["z_bs"], 0, bc)
        assert q == _model(B, D, L, 16, dtype, softplus, has_z, ops["act_addr_or"], ops["a_addr"], ops["b_addr"],
                           ops["c_addr"], ops["z_bs"], 0, bc), (B, D, L, off, S, has_z, softplus, ao, layout)
        if _lib.scan_plan_step(B, D, L, 16, dtype, **ops) == _lib.CKPT_SEQ:
            n_seq += 1
            if not q:
                bad.append((B, D, L, off, S, has_z, softplus, ao, layout))
    assert not bad, bad[:6]
    assert n_seq > 20


def test_forced_checkpoint_step_is_still_checked():
    """Parity tests force CKPT_SEQ below the row threshold (_lib.scan_ckpt): operands the library refuses still plan
    the row scan, and a forced row-scan forward never plans 16-step checkpoints."""
    ok = _mixer_operands(2, 128, 64, 4, 16, F32, 0, 0, 2 * 128 * 64)
    off = _mixer_operands(2, 192, 64, 6, 16, F32, 0, 0, 2 * 192 * 64)
    assert _lib.scan_plan_step(2, 128, 64, 16, F32, **ok) == _lib.CKPT_ROW
    with _lib.scan_ckpt(_lib.CKPT_SEQ):
        assert _lib.scan_plan_step(2, 128, 64, 16, F32, **ok) == _lib.CKPT_SEQ
        assert _lib.scan_plan_step(2, 192, 64, 16, F32, **off) == _lib.CKPT_ROW
        with _lib.scan_variant(_lib.SCAN_ROWSCAN):
            assert _lib.scan_plan_step(2, 128, 64, 16, F32, **ok) == _lib.CKPT_ROW
