"""CPU: the deterministic backward's C ABI (include/simamba.h, SIMAMBA_BWD_DETERMINISTIC) -- symbols, workspace sizes,
argument validation before any launch, and (where the ROCm binutils are installed) no float atomics in the
deterministic kernel instantiations of the shipped code object."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import pytest

from si_mamba_amd import _lib

NEW = ["simamba_scan_bwd_workspace_floats", "simamba_selective_scan_bwd_ex", "simamba_selective_scan_dt_bwd_ex",
       "simamba_causal_conv1d_bwd_workspace_floats", "simamba_causal_conv1d_bwd_ex"]
DET = _lib.BWD_DETERMINISTIC


def r64(n):
    return (n + 63) // 64 * 64


def test_symbols_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert DET == 1
    assert _lib.load().simamba_abi_version() == 9


def test_scan_workspace_sizes():
    lib = _lib.load()
    ws = lib.simamba_scan_bwd_workspace_floats
    for args in [(64, 768, 1024, 16, 16), (16, 768, 1024, 16, 128), (3, 200, 301, 8, 0)]:
        assert ws(*args, 0) == 0                                # flags == 0: the atomic form needs none
    # sequential kernel (16-step checkpoints): 64 channels per workgroup, one partial per sample
    B, D, L = 64, 768, 1024
    assert ws(B, D, L, 16, 16, DET) == r64(2 * (D // 64) * B * 16 * L) + r64(B * D * 16) + 2 * r64(B * D)
    # row scan (128-step chunks): 16 * passes channels per workgroup, one partial per (chunk, sample)
    B, D, L, N = 16, 768, 1024, 16
    passes = next(c for c in (12, 8, 6, 4, 3, 2, 1) if B * -(-D // (16 * c)) >= 512)
    groups, K = -(-D // (16 * passes)), 8 * B
    assert ws(B, D, L, N, 128, DET) == r64(2 * groups * B * N * L) + r64(K * D * N) + 2 * r64(K * D)
    assert ws(B, D, L, N, 0, DET) == ws(B, D, L, N, 128, DET)
    B, D, L, N = 3, 200, 301, 8                                 # ragged: passes 1, 13 groups, 3 chunks
    assert ws(B, D, L, N, 128, DET) == r64(2 * 13 * B * N * L) + r64(9 * D * N) + 2 * r64(9 * D)
    assert ws(B, D, L, N, 0, 2) == -9 and ws(B, D, L, N, 0, 3) == -9
    assert ws(B, D, L, 17, 0, DET) == -4
    assert ws(B, D, L, N, 32, DET) == -9


def test_conv_workspace_sizes():
    lib = _lib.load()
    ws = lib.simamba_causal_conv1d_bwd_workspace_floats
    assert ws(64, 768, 1024, 4, 0) == 0
    assert ws(64, 768, 1024, 4, 4) == -9
    assert ws(64, 768, 1024, 5, DET) == -5
    assert ws(0, 768, 1024, 4, DET) == 0
    for B, D, L, W in [(64, 768, 1024, 4), (3, 40, 37, 2), (8, 96, 130, 3)]:
        n = ws(B, D, L, W, DET)
        # [slices][D][W] (rounded up to 64 floats) + [slices][D], 1 <= slices (batch slices of the launch) <= B
        assert any(n == r64(k * D * W) + k * D for k in range(1, B + 1)), (B, D, L, W, n)


def _scan_ex(lib, flags, ws, nws, dstate=16, ckpt=16, batch=2, dim=64, L=64):
    one = ctypes.c_void_p(16)                # never dereferenced: every call below fails validation first
    n = None
    return lib.simamba_selective_scan_bwd_ex(one, one, one, one, one, n, n, n, one, one, one, one, one, one, one, n, n,
                                             n, batch, dim, L, dstate, 0, 1, 0, 0, 0, 0, 0, ckpt, flags, ws, nws, n)


def _dt_ex(lib, flags, ws, nws):
    one = ctypes.c_void_p(16)
    n = None
    return lib.simamba_selective_scan_dt_bwd_ex(one, one, one, one, n, one, n, one, one, one, one, one, one, one, n,
                                                one, n, 2, 64, 64, 16, 16, 0, 0, 0, 0, 0, flags, ws, nws, n)


def _conv_ex(lib, flags, ws, nws):
    one = ctypes.c_void_p(16)
    n = None
    return lib.simamba_causal_conv1d_bwd_ex(one, one, n, one, one, one, n, 2, 64, 64, 4, 1, 0, 0, 0, flags, ws, nws, n)


def test_ex_validation_precedes_any_launch():
    lib = _lib.load()
    need = lib.simamba_scan_bwd_workspace_floats(2, 64, 64, 16, 16, DET)
    need_conv = lib.simamba_causal_conv1d_bwd_workspace_floats(2, 64, 64, 4, DET)
    assert need > 0 and need_conv > 0
    ws = ctypes.c_void_p(1 << 20)
    odd = ctypes.c_void_p((1 << 20) + 4)
    for call, n in [(_scan_ex, need), (_dt_ex, need), (_conv_ex, need_conv)]:
        assert call(lib, 2, ws, n) == -9                         # unknown flag bit
        assert call(lib, DET | 4, ws, n) == -9
        assert call(lib, DET, None, 0) == -6                     # no workspace
        assert call(lib, DET, None, n) == -6
        assert call(lib, DET, ws, n - 1) == -6                   # one float short
        assert call(lib, DET, odd, n + 4) == -8                  # not 16-byte aligned
    # the row-scan layout is asked for with ckpt_step 128 (or 0)
    need_row = lib.simamba_scan_bwd_workspace_floats(2, 64, 64, 8, 128, DET)
    assert _scan_ex(lib, DET, ws, need_row - 1, dstate=8, ckpt=128) == -6
    assert _scan_ex(lib, DET, ws, need_row - 1, dstate=8, ckpt=0) == -6
    # argument errors of the plain form keep their codes
    assert _scan_ex(lib, DET, ws, need, dstate=17) == -4
    assert _scan_ex(lib, 0, None, 0, dstate=17) == -4


# ---- the shipped code object: deterministic instantiations carry no float atomics ---------------------------------
_ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
_OBJCOPY = shutil.which("llvm-objcopy", path=os.path.join(_ROCM, "llvm", "bin"))
_OBJDUMP = shutil.which("llvm-objdump", path=os.path.join(_ROCM, "llvm", "bin"))
_FLOAT_ATOMICS = re.compile(r"\b(global|flat|buffer)_atomic_(add|pk_add)_(f32|bf16|f16)|\bds_(add|pk_add)(_rtn)?_(f32|bf16|f16)")


def _gfx950_code_objects(fatbin):
    """the gfx950 entries of every clang offload bundle in a .hip_fatbin section"""
    magic, out, pos = b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    while True:
        i = fatbin.find(magic, pos)
        if i < 0:
            return out
        (n,) = struct.unpack_from("<Q", fatbin, i + 24)
        o = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", fatbin, o)
            triple = fatbin[o + 24:o + 24 + tl].decode()
            o += 24 + tl
            if "gfx950" in triple:
                out.append(fatbin[i + off:i + off + size])
        pos = i + 1


@pytest.mark.skipif(not (_OBJCOPY and _OBJDUMP), reason="ROCm llvm-objcopy / llvm-objdump not installed")
def test_deterministic_kernels_have_no_float_atomics(tmp_path):
    fb = tmp_path / "fatbin"
    subprocess.run([_OBJCOPY, "--dump-section", f".hip_fatbin={fb}", _lib.LIB_PATH, str(tmp_path / "stripped")],
                   check=True)
    funcs = {}
    for k, co in enumerate(_gfx950_code_objects(fb.read_bytes())):
        p = tmp_path / f"{k}.co"
        p.write_bytes(co)
        txt = subprocess.run([_OBJDUMP, "-d", "--no-show-raw-insn", str(p)], capture_output=True, text=True,
                             check=True).stdout
        cur = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line.strip())
            if m:
                cur = m.group(1)
                funcs[cur] = []
            elif cur:
                funcs[cur].append(line)
    # the deterministic instantiations: the last template argument (kDet) is true
    det = {f: "\n".join(v) for f, v in funcs.items()
           if re.search(r"(scan_bwd_seq_kernel|scan_bwd_kernel|conv1d_bwd_kernel|conv1d_bwd_fast_kernel)I.*Lb1EEEvNS", f)
           or "det_sum_kernel" in f}
    names = " ".join(det)
    assert names.count("scan_bwd_seq_kernel") == 6, names    # fp32 / bf16 x (z, no z, the dt form)
    assert names.count("scan_bwd_kernel") == 4, names        # fp32 / bf16 x 4 / 8 items
    assert names.count("conv1d_bwd") == 4, names             # fp32 / bf16 x general / fast
    assert names.count("det_sum_kernel") == 1, names
    bad = {f: sorted(set(m.group(0) for m in _FLOAT_ATOMICS.finditer(t))) for f, t in det.items()
           if _FLOAT_ATOMICS.search(t)}
    assert not bad, bad
    # ... while the default instantiations still are the atomic ones (the check above would notice nothing otherwise)
    dflt = "\n".join("\n".join(v) for f, v in funcs.items() if re.search(r"scan_bwd_seq_kernelI.*Lb0EEEvNS", f))
    assert _FLOAT_ATOMICS.search(dflt)
