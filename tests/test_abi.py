"""CPU: the C-ABI library loads, exports every symbol include/simamba.h declares, and validates
arguments before touching the device (no compute calls here)."""
import ctypes
import os
import re

import pytest

import abi_tables
from abi_tables import OFF, P, check_rows, declared_params
from conftest import ROOT
from si_mamba_amd import _lib


def _declared():
    return sorted(set(re.findall(r"\b(simamba_[a-z0-9_]+)\s*\(", abi_tables.header_code())))


def test_header_and_binding_agree():
    assert _declared() == sorted(_lib.SIGNATURES)


def _kind(ctype):
    if ctype in (ctypes.c_void_p, ctypes.c_char_p):
        return "pointer"
    if ctype is ctypes.c_float:
        return "float"
    assert ctype in (ctypes.c_int, ctypes.c_uint, ctypes.c_longlong, ctypes.c_size_t), ctype
    return "integer"


def test_header_and_binding_agree_on_parameters():
    """ctypes accepts surplus arguments silently and converts whatever argtypes says, so a binding that disagrees
    with the header would first show on the device: count and kind (pointer / float / integer) of every parameter."""
    declared = declared_params()
    assert sorted(declared) == sorted(_lib.SIGNATURES)
    for name, params in declared.items():
        argtypes = _lib.SIGNATURES[name][1]
        assert len(params) == len(argtypes), name
        for i, (param, ctype) in enumerate(zip(params, argtypes)):
            want = "pointer" if "*" in param else "float" if re.match(r"(const\s+)?float\b", param) else "integer"
            assert "double" not in param or "*" in param, (name, param)       # no by-value double in the ABI
            assert _kind(ctype) == want, (name, i, param)
    # every entry point _lib.call can launch takes the stream last
    for name, params in declared.items():
        if any("stream" in p for p in params):
            assert re.fullmatch(r"void\s*\*\s*stream", params[-1]), name


# direct calls that expand a sequence into the argument list: their arity is not countable from the source
_STARRED_CALLS = {("_lib.py", "simamba_scan_seq_applicable")}


def test_every_call_site_has_the_right_arity():
    """Every C-ABI call in the package, from its source alone: _lib.call("simamba_x", ...) names a bound symbol with a
    string literal and passes its arguments less the stream; a direct lib.simamba_x(...) call (the host-only queries)
    passes all of them."""
    import ast
    pkg = os.path.join(ROOT, "si_mamba_amd")
    sites, starred = 0, set()
    for dp, _, files in os.walk(pkg):
        for f in sorted(files):
            if not f.endswith(".py"):
                continue
            path = os.path.join(dp, f)
            for node in ast.walk(ast.parse(open(path).read(), path)):
                if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)):
                    continue
                where = f"{os.path.relpath(path, pkg)}:{node.lineno}"
                has_star = any(isinstance(a, ast.Starred) for a in node.args)
                if node.func.attr == "call" and isinstance(node.func.value, ast.Name) and node.func.value.id == "_lib":
                    name = node.args[0]
                    assert isinstance(name, ast.Constant) and isinstance(name.value, str), where
                    assert name.value in _lib.SIGNATURES, (where, name.value)
                    assert not has_star, where
                    assert {k.arg for k in node.keywords} <= {"device", "time_as"}, where
                    assert "device" in {k.arg for k in node.keywords}, where
                    # node.args holds the name and not the stream: positional arguments + 1 == len(argtypes)
                    assert (len(node.args) - 1) + 1 == len(_lib.SIGNATURES[name.value][1]), (where, name.value)
                    sites += 1
                elif node.func.attr.startswith("simamba_"):
                    name = node.func.attr
                    assert name in _lib.SIGNATURES, (where, name)
                    assert not node.keywords, where
                    if has_star:
                        starred.add((os.path.relpath(path, pkg), name))
                    else:
                        assert len(node.args) == len(_lib.SIGNATURES[name][1]), (where, name)
                    sites += 1
    assert starred == _STARRED_CALLS
    assert sites >= 50, sites


def test_library_exports_every_declared_symbol():
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), name


def test_version_strerror_and_chunks():
    lib = _lib.load()
    assert lib.simamba_abi_version() == 9
    assert _lib.ABI_VERSION == 9
    assert lib.simamba_strerror(0) == b"ok"
    assert b"dstate" in lib.simamba_strerror(-4)
    assert lib.simamba_scan_num_chunks(64) == 1
    assert lib.simamba_scan_num_chunks(128) == 1
    assert lib.simamba_scan_num_chunks(129) == 2
    assert lib.simamba_scan_num_chunks(1024) == 8
    # host-side kernel choice: row-scan below 49 152 rows, two lanes per channel from there on
    assert lib.simamba_scan_fwd_auto_variant(32, 768) == 1
    assert lib.simamba_scan_fwd_auto_variant(64, 768) == 2
    assert lib.simamba_scan_fwd_auto_variant(256, 768) == 2
    # checkpoint plan: the sequential backward (16-step checkpoints) from the row count on at which the forward is a
    # lanes-per-channel kernel, for shapes it can take; sizes of both layouts
    assert lib.simamba_scan_ckpt_step(64, 768, 1024, 16, 0) == 16
    assert lib.simamba_scan_ckpt_step(32, 768, 1024, 16, 0) == 128
    assert lib.simamba_scan_ckpt_step(64, 768, 1024, 8, 0) == 128
    assert lib.simamba_scan_ckpt_step(64, 776, 1024, 16, 0) == 128      # dim % 64
    assert lib.simamba_scan_ckpt_step(64, 768, 1022, 16, 0) == 128      # rows not 16-byte aligned
    assert lib.simamba_scan_ckpt_step(64, 768, 1020, 16, 1) == 128      # bf16: 8-element packs
    assert lib.simamba_scan_ckpt_floats(64, 768, 1024, 16, 16) == 64 * 64 * 768 * 16
    assert lib.simamba_scan_ckpt_floats(64, 768, 1024, 16, 128) == 64 * 768 * 8 * 16
    assert lib.simamba_scan_ckpt_floats(64, 768, 16, 16, 16) == 0
    assert lib.simamba_scan_ckpt_floats(64, 768, 128, 16, 128) == 0
    assert lib.simamba_spectral_workspace_bytes(4, 128) == 256 + 4 * 128 * 128 * 4
    assert b"variant" in lib.simamba_strerror(-9)


def test_error_code_literals_equal_the_header():
    """tests/abi_tables.py spells the codes as numbers, which are an ABI promise: each equals its #define, and the
    header defines no code the tables have no name for."""
    defines = {k: int(v) for k, v in re.findall(r"#define\s+SIMAMBA_(OK|E_[A-Z]+)\s+(-?\d+)", abi_tables.header_code())}
    assert defines == {k: getattr(abi_tables, k) for k in defines}
    assert sorted(defines.values()) == list(range(-10, 1))


# The *_ex scan backward, the dt pair and the workspace query.  Every row states what it changes in a call that would
# otherwise be accepted, and the code the library answers; rows with two faults pin the order of the checks.  P is a
# 16-byte aligned address that is never dereferenced: no row gets as far as a memset or a launch.  (An empty backward
# problem that passes validation clears the caller's accumulators, a device call, so it has no row here; the rows with
# batch == 0 show that the checks in front of that still run.)
_BWD_EX = dict(u=P, delta=P, A=P, B=P, C=P, D=None, z=None, delta_bias=None, dout=P, x_ckpt=P, du=P, ddelta=P, dA=P,
               dB=P, dC=P, dD=None, dz=None, ddelta_bias=None, batch=2, dim=64, seqlen=32, dstate=16, io_dtype=0,
               delta_softplus=1, z_bstride=0, dz_bstride=0, bc_bstride=0, bc_nstride=0, bc_tstride=0, ckpt_step=16,
               flags=1, workspace=P, workspace_floats=1 << 40, stream=None)
_DT_FWD = dict(u=P, xdbl=P, wdt=P, A=P, D=None, z=P, delta_bias=None, out=P, x_ckpt=None, last_state=None, batch=2,
               dim=64, seqlen=32, dstate=16, dt_rank=8, io_dtype=0, z_bstride=0, xdbl_bstride=0, xdbl_tstride=0,
               ckpt_step=0, variant=0, stream=None)
_DT_BWD_EX = dict(u=P, xdbl=P, wdt=P, A=P, D=None, z=P, delta_bias=None, dout=P, x_ckpt=P, du=P, ddelta=P, dA=P, dB=P,
                  dC=P, dD=None, dz=P, ddelta_bias=None, batch=2, dim=64, seqlen=32, dstate=16, dt_rank=8, io_dtype=0,
                  z_bstride=0, dz_bstride=0, xdbl_bstride=0, xdbl_tstride=0, flags=1, workspace=P,
                  workspace_floats=1 << 40, stream=None)
_WS = dict(batch=2, dim=64, seqlen=32, dstate=16, ckpt_step=16, flags=1)

SCAN_ROWS = [
    # ---- simamba_selective_scan_bwd_ex -----------------------------------------------------------------------------
    ("simamba_selective_scan_bwd_ex", _BWD_EX, [
        (dict(dim=0), -2), (dict(batch=65536), -2), (dict(seqlen=-1), -2),                    # shape
        (dict(dstate=17), -4), (dict(dstate=0), -4), (dict(io_dtype=7), -3),
        (dict(ckpt_step=32), -9), (dict(flags=2), -9), (dict(flags=3), -9),
        (dict(A=None), -1), (dict(dA=None), -1), (dict(u=None), -1), (dict(delta=None), -1), (dict(dC=None), -1),
        (dict(z=P), -1), (dict(dz=P), -1),                                                    # z and dz go together
        (dict(x_ckpt=None), -1), (dict(x_ckpt=None, ckpt_step=128, seqlen=132), -1),
        (dict(workspace=None), -6), (dict(workspace_floats=64), -6), (dict(workspace=OFF), -8),
        (dict(batch=0, dA=None), -1), (dict(seqlen=0, workspace=OFF), -8),                    # empty, and still checked
        # what the sequential kernel cannot take (deterministic: nothing is cleared in front of this answer)
        (dict(dim=32), -9), (dict(dstate=8), -9), (dict(delta_softplus=0), -9), (dict(u=OFF), -9),
        (dict(ddelta=OFF), -9),
        (dict(seqlen=30), -9), (dict(io_dtype=1, seqlen=36), -9), (dict(A=OFF), -9), (dict(x_ckpt=OFF), -9),
        (dict(B=OFF), -9), (dict(bc_bstride=514, bc_nstride=32, bc_tstride=1), -9),
        (dict(bc_bstride=512, bc_nstride=2, bc_tstride=32), -9),
        (dict(z=P, dz=OFF), -9), (dict(z=P, dz=P, z_bstride=2050), -9), (dict(z=P, dz=P, dz_bstride=1 << 29), -9),
        (dict(batch=4096, dim=4096, seqlen=64), -9),                                          # rows * seqlen = 2^30
        # two faults: flags, shape, ckpt_step, dstate, dtype, pointers, workspace size, workspace alignment, kernel
        (dict(flags=2, dim=0), -9), (dict(dim=0, ckpt_step=32), -2), (dict(ckpt_step=32, dstate=17), -9),
        (dict(dstate=17, io_dtype=7), -4), (dict(io_dtype=7, A=None), -3), (dict(u=None, workspace=None), -1),
        (dict(workspace=OFF, workspace_floats=64), -6), (dict(workspace=OFF, dim=32), -8),
    ]),
    # ---- simamba_selective_scan_dt_fwd -----------------------------------------------------------------------------
    ("simamba_selective_scan_dt_fwd", _DT_FWD, [
        (dict(dim=0), -2), (dict(batch=65536), -2), (dict(dstate=8), -4), (dict(io_dtype=7), -3),
        (dict(ckpt_step=32), -9), (dict(variant=1), -9), (dict(variant=3), -9),
        (dict(dt_rank=6), -2), (dict(dt_rank=0), -2), (dict(dt_rank=28), -2),                 # fp32: packs of 4
        (dict(io_dtype=1, seqlen=64, dt_rank=4), -2), (dict(io_dtype=1, seqlen=64, dt_rank=12), -2),   # bf16: of 8
        (dict(u=None), -1), (dict(xdbl=None), -1), (dict(wdt=None), -1), (dict(z=None), -1), (dict(out=None), -1),
        (dict(xdbl=OFF), -9), (dict(wdt=OFF), -9), (dict(u=OFF), -9), (dict(A=OFF), -9), (dict(seqlen=30), -9),
        (dict(xdbl_bstride=1 << 29), -9), (dict(xdbl_tstride=42), -9), (dict(z_bstride=2050), -9),
        (dict(z_bstride=1 << 29), -9),
        (dict(batch=4096, dim=4096, seqlen=64), -9),
        (dict(batch=0), 0), (dict(seqlen=0, u=None, xdbl=None, out=None), 0),                 # empty problems
        # two faults: shape, dstate, dtype, ckpt_step, variant, dt_rank, empty, pointers, the kernel's conditions
        (dict(dim=0, dstate=8), -2), (dict(dstate=8, io_dtype=7), -4), (dict(io_dtype=7, ckpt_step=32), -3),
        (dict(variant=1, dt_rank=6), -9), (dict(dt_rank=6, batch=0), -2), (dict(batch=0, xdbl=OFF), 0),
        (dict(u=None, xdbl=OFF), -1),
    ]),
    # ---- simamba_selective_scan_dt_bwd_ex --------------------------------------------------------------------------
    ("simamba_selective_scan_dt_bwd_ex", _DT_BWD_EX, [
        (dict(flags=2), -9), (dict(dstate=8), -4), (dict(io_dtype=7), -3),
        (dict(dt_rank=6), -2), (dict(dt_rank=28), -2),
        (dict(io_dtype=1, seqlen=64, dt_rank=4), -2), (dict(io_dtype=1, seqlen=64, dt_rank=12), -2),
        (dict(xdbl=None), -1), (dict(wdt=None), -1), (dict(z=None), -1),
        (dict(xdbl=OFF), -9), (dict(wdt=OFF), -9), (dict(xdbl_bstride=1 << 29), -9), (dict(xdbl_tstride=42), -9),
        (dict(dim=0), -2), (dict(batch=65536), -2), (dict(u=None), -1), (dict(dA=None), -1), (dict(dz=None), -1),
        (dict(x_ckpt=None), -1), (dict(workspace=None), -6), (dict(workspace_floats=64), -6),
        (dict(workspace=OFF), -8), (dict(batch=0, dA=None), -1), (dict(seqlen=0, workspace=OFF), -8),
        (dict(dim=32), -9), (dict(u=OFF), -9), (dict(seqlen=30), -9), (dict(A=OFF), -9), (dict(dz_bstride=2050), -9),
        # two faults: flags, dstate, dtype, dt_rank, pointers, xdbl's layout -- all in front of the shape check
        (dict(flags=2, dstate=8), -9), (dict(dstate=8, dim=0), -4), (dict(io_dtype=7, dt_rank=6), -3),
        (dict(dt_rank=6, xdbl=None), -2), (dict(xdbl=None, wdt=OFF), -1), (dict(xdbl=OFF, dim=0), -9),
        (dict(batch=0, xdbl=OFF), -9), (dict(dim=0, workspace=None), -2),
    ]),
    # ---- simamba_scan_bwd_workspace_floats -------------------------------------------------------------------------
    ("simamba_scan_bwd_workspace_floats", _WS, [
        (dict(flags=2), -9), (dict(flags=0), 0), (dict(flags=0, dim=0), 0),                   # no flag: no workspace
        (dict(dim=0), -2), (dict(batch=65536), -2), (dict(dstate=17), -4), (dict(ckpt_step=32), -9),
        (dict(batch=0), 0),
        (dict(), 4352), (dict(ckpt_step=0, seqlen=200), 55808),
        (dict(flags=2, dim=0), -9), (dict(dim=0, dstate=17), -2), (dict(dstate=17, ckpt_step=32), -4),
    ]),
]


def test_argument_validation_precedes_any_launch():
    lib = _lib.load()
    n = None
    one = ctypes.c_void_p(16)   # never dereferenced: every call below fails validation first
    assert lib.simamba_selective_scan_fwd(n, n, n, n, n, n, n, n, n, n, n, 1, 1, 1, 16, 0, 1, 0, 0, 0, 0, 0, 0, n) == -1
    assert lib.simamba_selective_scan_fwd(one, one, one, one, one, n, n, n, one, n, n, 1, 8, 8, 17, 0, 1, 0, 0, 0, 0, 0, 0, n) == -4
    assert lib.simamba_selective_scan_fwd(one, one, one, one, one, n, n, n, one, n, n, 1, 8, 8, 16, 7, 1, 0, 0, 0, 0, 0, 0, n) == -3
    assert lib.simamba_selective_scan_fwd(one, one, one, one, one, n, n, n, one, n, n, 0, 8, 8, 16, 0, 1, 0, 0, 0, 0, 0, 0, n) == 0
    # an unknown kernel variant, and an explicit lanes-per-channel request the shape cannot take (dstate != 16)
    assert lib.simamba_selective_scan_fwd(one, one, one, one, one, n, n, n, one, n, n, 1, 8, 8, 16, 0, 1, 0, 0, 0, 0, 0, 3, n) == -9
    assert lib.simamba_selective_scan_fwd(one, one, one, one, one, n, n, n, one, n, n, 1, 8, 8, 8, 0, 1, 0, 0, 0, 0, 0, 2, n) == -9
    # a checkpoint layout that does not exist; 16-step checkpoints from the row-scan kernel
    assert lib.simamba_selective_scan_fwd(one, one, one, one, one, n, n, n, one, one, n, 1, 64, 64, 16, 0, 1, 0, 0, 0, 0, 32, 0, n) == -9
    assert lib.simamba_selective_scan_fwd(one, one, one, one, one, n, n, n, one, one, n, 1, 64, 64, 16, 0, 1, 0, 0, 0, 0, 16, 1, n) == -9
    assert lib.simamba_causal_conv1d_fwd(one, one, n, one, 1, 8, 8, 5, 1, 0, 0, n) == -5
    assert lib.simamba_laplacian_topk(one, n, n, n, n, n, 1, 129, 4, 0, n) == -7
    assert lib.simamba_knn_graph(one, one, n, 0, 1, 16, 3, 16, 1.0, 0, n) == -7
    assert lib.simamba_spectral_topk(one, n, n, n, one, 8, 1, 16, 4, 1.0, 4, 0, n) == -6
    assert lib.simamba_argsort_rows(one, one, 1, 2048, n) == -2
    for name, base, rows in SCAN_ROWS:
        check_rows(name, base, rows, lib)


def test_product_path_refuses_cpu_tensors():
    import torch
    from si_mamba_amd import selective_scan_fn, causal_conv1d_fn, Mamba
    u = torch.zeros(1, 4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        selective_scan_fn(u, u, torch.zeros(4, 2), torch.zeros(1, 2, 8), torch.zeros(1, 2, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        causal_conv1d_fn(u, torch.zeros(4, 4))
    with pytest.raises(RuntimeError):
        Mamba(16)(torch.zeros(1, 8, 16))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "si_mamba_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
