"""CPU: the C ABI of the large-G spectral path (128 < G <= 512) and of farthest-point sampling up to 8192 points.
Argument validation only: every call below is refused, or has B == 0, before anything touches a device."""
import ctypes
import os
import re

import pytest

from abi_tables import header_code
from conftest import ROOT
from si_mamba_amd import _lib

NEW = ("simamba_laplacian_topk_workspace_bytes", "simamba_laplacian_topk_ex")


@pytest.mark.parametrize("name", NEW)
def test_new_symbols_in_header_binding_and_library(name):
    assert re.search(r"\b" + name + r"\s*\(", header_code()), name
    assert name in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


def test_large_g_flag_matches_header():
    m = re.search(r"#define\s+SIMAMBA_SPEC_LARGE_G\s+(0x[0-9a-fA-F]+)u", open(os.path.join(ROOT, "include",
                                                                                       "simamba.h")).read())
    assert m and int(m.group(1), 16) == _lib.SPEC_LARGE_G


def test_laplacian_topk_ex_validation():
    lib = _lib.load()
    n = None
    one = ctypes.c_void_p(16)   # never dereferenced
    ws = lib.simamba_laplacian_topk_workspace_bytes(1, 256)
    assert ws == 4 * 256 * 256
    assert lib.simamba_laplacian_topk_ex(one, n, n, n, one, 1 << 30, 1, 513, 4, 0, n) == -7
    assert lib.simamba_laplacian_topk_ex(one, n, n, n, one, 1 << 30, 1, 1, 1, 0, n) == -7
    assert lib.simamba_laplacian_topk_ex(one, n, n, n, one, ws - 1, 1, 256, 4, 0, n) == -6
    assert lib.simamba_laplacian_topk_ex(n, n, n, n, one, ws, 1, 256, 4, 0, n) == -1
    assert lib.simamba_laplacian_topk_ex(one, n, n, n, n, 0, 1, 256, 4, 0, n) == -1        # no workspace above 128
    # the large-G kernel extracts at most 8 pairs; MATRIX_SYM needs one more
    assert lib.simamba_laplacian_topk_ex(one, n, n, n, one, ws, 1, 256, 9, 0, n) == -7
    assert lib.simamba_laplacian_topk_ex(one, n, n, n, one, ws, 1, 256, 8, _lib.SPEC_MATRIX_SYM, n) == -7
    assert lib.simamba_laplacian_topk_ex(one, n, n, n, one, ws, 1, 256, 4, 0x80, n) == -9  # unknown flag bit
    assert lib.simamba_laplacian_topk_ex(one, n, n, n, one, ws, 0, 256, 4, 0, n) == 0      # empty batch
    # at G <= 128 the call is simamba_laplacian_topk: no workspace needed (empty batch, nothing launched)
    assert lib.simamba_laplacian_topk_ex(one, n, n, n, n, 0, 0, 128, 4, 0, n) == 0
    # ... unless the large-G kernel is forced, which needs its workspace
    assert lib.simamba_laplacian_topk_ex(one, n, n, n, one, 8, 1, 64, 4, _lib.SPEC_LARGE_G, n) == -6
    # the G <= 128 entry point keeps its limit
    assert lib.simamba_laplacian_topk(one, n, n, n, n, n, 1, 129, 4, 0, n) == -7


def test_knn_graph_and_fused_accept_512():
    lib = _lib.load()
    n = None
    one = ctypes.c_void_p(16)
    assert lib.simamba_knn_graph(one, one, n, 0, 0, 512, 3, 20, 1.0, 0, n) == 0
    assert lib.simamba_knn_graph(one, one, n, 0, 0, 513, 3, 20, 1.0, 0, n) == -7
    assert lib.simamba_knn_graph(one, one, n, 0, 0, 512, 3, 32, 1.0, 0, n) == -7             # knn + 1 <= 32
    nb = lib.simamba_spectral_workspace_bytes(0, 512)
    assert lib.simamba_spectral_topk(one, n, n, n, one, nb, 0, 512, 20, 1.0, 4, 0, n) == 0
    assert lib.simamba_spectral_topk(one, n, n, n, one, nb, 0, 513, 20, 1.0, 4, 0, n) == -7


def test_farthest_point_sample_accepts_8192():
    lib = _lib.load()
    n = None
    one = ctypes.c_void_p(16)
    assert lib.simamba_farthest_point_sample(one, one, n, 0, 8192, 512, n) == 0
    assert lib.simamba_farthest_point_sample(one, one, n, 0, 8193, 512, n) == -2
    assert lib.simamba_farthest_point_sample(one, one, n, 0, 4097, 4097, n) == 0
    assert lib.simamba_farthest_point_sample(one, one, n, 1, 8192, 8193, n) == -2          # K <= N


def test_workspace_sizes():
    lib = _lib.load()
    for B, G in [(1, 2), (4, 64), (4, 128), (64, 128)]:
        assert lib.simamba_spectral_workspace_bytes(B, G) == 256 + 4 * B * G * G
    for B, G in [(2, 129), (64, 256), (64, 512)]:
        adj = 4 * B * G * G
        assert lib.simamba_spectral_workspace_bytes(B, G) == 256 + ((adj + 255) // 256) * 256 + adj
        assert lib.simamba_laplacian_topk_workspace_bytes(B, G) == adj
