"""ctypes binding of libsimamba_hip.so (C ABI: include/simamba.h).

The product path has NO fallback: if the shared library is missing or a symbol
is absent, importing an op raises.  Nothing here (or anywhere in this package)
imports ``oracle``.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_longlong, c_size_t, c_uint, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsimamba_hip.so")

F32, BF16 = 0, 1

SPEC_SYMMETRIC = 0x01
SPEC_SELF_LOOP = 0x02
SPEC_BINARY = 0x04
SPEC_MATRIX_SYM = 0x08
SPEC_SMALLEST = 0x10
SPEC_SIGMA_MEAN = 0x20
SPEC_LARGE_G = 0x40          # simamba_laplacian_topk_ex: the large-G kernel at G <= 128 too (parity tests only)
SPEC_MAX_G = 128             # simamba_laplacian_topk and the full-spectrum outputs
SPEC_MAX_G_LARGE = 512       # graph, simamba_laplacian_topk_ex and the fused call
# simamba_curve_order (spectral.curve_order): curve ids, box modes and the limits
CURVE_Z, CURVE_HILBERT, CURVE_TRANS, CURVE_Z_TRANS, CURVE_HILBERT_TRANS = 0, 1, 2, 2, 3
CURVE_BOX_CLOUD, CURVE_BOX_FIXED = 0, 1
CURVE_MAX_G, CURVE_MAX_K, CURVE_MAX_BITS = 8192, 8, 16

# forward-scan kernel selection (include/simamba.h): AUTO in production, the others for benchmarks / parity tests
SCAN_AUTO, SCAN_ROWSCAN, SCAN_LPC2, SCAN_LPC4, SCAN_MIX = 0, 1, 2, 4, 6
# checkpoint layouts handed from the forward scan to the backward (= which backward kernel runs)
CKPT_ROW, CKPT_SEQ = 128, 16
# flags of the *_ex backward entry points: no float atomics, bitwise reproducible parameter gradients
BWD_DETERMINISTIC = 1
# flags of the add + norm *_ex entry points: RMSNorm in place of LayerNorm
NORM_RMS = 1
# flags of simamba_sinkhorn_fwd / _bwd: subtract the two self-transport terms
SINKHORN_DEBIAS = 1
# opcodes of simamba_augment_points / _params (transforms.py); at most AUG_MAX_OPS per launch, AUG_CLOUD_PARAMS floats
# per (cloud, op) from simamba_augment_params
AUG_ROTATE, AUG_SCALE, AUG_TRANSLATE, AUG_SCALE_TRANSLATE, AUG_JITTER, AUG_DROPOUT, AUG_FLIP = 1, 2, 3, 4, 5, 6, 7
AUG_MAX_OPS = 8
AUG_CLOUD_PARAMS = 8
AUG_MAX_POINTS = 8192
# modes of simamba_dataset_fetch (data.py) and the purposes of its keyed streams
DS_SEQUENTIAL, DS_SHUFFLE = 0, 1
DS_FIRST, DS_PERMUTE, DS_CHOICE = 0, 1, 2
DS_NONE, DS_UNIT_SPHERE = 0, 1
DS_STREAM_SHUFFLE, DS_STREAM_ROWS, DS_STREAM_CHOICE = 1, 2, 3
DS_MAX_POINTS = 8192
# kinds and the flag of simamba_corrupt_points (corruptions.py); the tweak of its Philox key's high word
(CORRUPT_DROP_GLOBAL, CORRUPT_DROP_LOCAL, CORRUPT_ADD_GLOBAL, CORRUPT_ADD_LOCAL, CORRUPT_ROTATE3, CORRUPT_SCALE_AXES,
 CORRUPT_JITTER) = 1, 2, 3, 4, 5, 6, 7
CORRUPT_RENORM = 1
CORRUPT_MAX_CLUSTERS = 8
CORRUPT_KEY_TWEAK = 0x434F5252
CORRUPT_MAX_POINTS = 8192
# modes of simamba_cutmix_points, the flag and the anchor limit of simamba_pointwolf_points (mixing/); the tweak of
# their Philox key's high word, which differs from corrupt's
MIX_CUT_R, MIX_CUT_K = 1, 2
MIX_KEY_TWEAK = 0x4D495847
WOLF_RENORM = 1
WOLF_MAX_ANCHORS = 8
# simamba_optim_adamw_step (optim/adamw.py): elements per chunk-table entry, the table limits, the flag
OPTIM_CHUNK = 4096
OPTIM_MAX_SEGMENTS, OPTIM_MAX_CHUNKS, OPTIM_MAX_GROUPS = 65536, 1 << 20, 256
OPTIM_ZERO_GRADS = 1

# name -> (restype, argtypes); mirrors include/simamba.h one to one
_P = c_void_p
_LL = c_longlong
ABI_VERSION = 9
SIGNATURES = {
    "simamba_abi_version": (c_int, []),
    "simamba_strerror": (c_char_p, [c_int]),
    "simamba_scan_num_chunks": (c_int, [c_int]),
    "simamba_scan_fwd_auto_variant": (c_int, [c_int, c_int]),
    "simamba_scan_ckpt_step": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "simamba_scan_ckpt_floats": (_LL, [c_int, c_int, c_int, c_int, c_int]),
    "simamba_scan_seq_applicable": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                            c_size_t, c_size_t, c_size_t, c_size_t, _LL, _LL, _LL, _LL, _LL]),
    "simamba_selective_scan_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                           c_int, c_int, c_int, c_int, c_int, c_int,
                                           _LL, _LL, _LL, _LL, c_int, c_int, _P]),
    "simamba_selective_scan_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                           _P, _P, _P, _P, _P, _P, _P, _P,
                                           c_int, c_int, c_int, c_int, c_int, c_int,
                                           _LL, _LL, _LL, _LL, _LL, c_int, _P]),
    "simamba_scan_bwd_workspace_floats": (_LL, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "simamba_selective_scan_bwd_ex": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                              _P, _P, _P, _P, _P, _P, _P, _P,
                                              c_int, c_int, c_int, c_int, c_int, c_int,
                                              _LL, _LL, _LL, _LL, _LL, c_int, c_int, _P, _LL, _P]),
    "simamba_selective_scan_dt_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                              c_int, c_int, c_int, c_int, c_int, c_int,
                                              _LL, _LL, _LL, c_int, c_int, _P]),
    "simamba_selective_scan_dt_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P,
                                              _P, _P, _P, _P, _P, _P, _P, _P,
                                              c_int, c_int, c_int, c_int, c_int, c_int,
                                              _LL, _LL, _LL, _LL, _P]),
    "simamba_selective_scan_dt_bwd_ex": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P,
                                                 _P, _P, _P, _P, _P, _P, _P, _P,
                                                 c_int, c_int, c_int, c_int, c_int, c_int,
                                                 _LL, _LL, _LL, _LL, c_int, _P, _LL, _P]),
    "simamba_xdt_proj_fwd": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _LL, _P]),
    "simamba_conv_xdt_proj_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _LL,
                                          _P]),
    "simamba_seq_gather_fwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _LL, c_int, _P]),
    "simamba_seq_gather_bwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, _LL, c_int, _P]),
    "simamba_causal_conv1d_fwd": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _LL, _P]),
    "simamba_causal_conv1d_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P,
                                          c_int, c_int, c_int, c_int, c_int, c_int, _LL, _LL, _P]),
    "simamba_causal_conv1d_bwd_workspace_floats": (_LL, [c_int, c_int, c_int, c_int, c_int]),
    "simamba_causal_conv1d_bwd_ex": (c_int, [_P, _P, _P, _P, _P, _P, _P,
                                             c_int, c_int, c_int, c_int, c_int, c_int, _LL, _LL, c_int, _P, _LL, _P]),
    "simamba_add_layer_norm_grid": (c_int, [c_int, c_int]),
    "simamba_add_layer_norm_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_float,
                                           c_int, c_int, _P]),
    "simamba_add_layer_norm_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int,
                                           c_int, c_int, _P]),
    "simamba_add_layer_norm_fwd_ex": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_float,
                                              c_int, c_int, c_int, _P]),
    "simamba_add_layer_norm_bwd_ex": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int,
                                              c_int, c_int, c_int, _P]),
    "simamba_add_layer_norm_check_slots": (c_int, [_P, c_int, c_int]),
    "simamba_add_layer_norm_fwd_slots": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _P, c_int, c_int, c_int,
                                                 c_int, c_float, c_int, c_int, c_int, _P]),
    "simamba_add_layer_norm_bwd_slots": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _P, c_int, c_int,
                                                 c_int, c_int, c_int, c_int, c_int, _P]),
    "simamba_out_proj_add_ln_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float,
                                            c_int, _P]),
    "simamba_out_proj_add_ln_fwd_ex": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int,
                                               c_float, c_int, c_int, _P]),
    "simamba_in_proj_fwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "simamba_bn_relu_grid": (c_int, [_LL]),
    "simamba_bn_relu_fwd": (c_int, [_P, _P, c_int, _P, _P, _P, _P, c_float, c_float, c_int, _P, _P, _P, _P, _LL, c_int,
                                    _LL, c_int, _P]),
    "simamba_bn_relu_bwd": (c_int, [_P, _P, _P, c_int, _P, _P, _P, _P, _P, _P, c_int, _P, _P, _P, _LL, c_int, _LL,
                                    c_int, c_int, _P]),
    "simamba_bn_stats_local": (c_int, [_P, _P, c_int, _P, _LL, _P, _LL, c_int, _LL, c_int, _P]),
    "simamba_bn_stats_merge": (c_int, [_P, c_int, _P, _P, c_float, c_float, _P, _P, _P, c_int, _P]),
    "simamba_bn_relu_apply": (c_int, [_P, _P, c_int, _P, _P, _P, _P, _P, _LL, c_int, _LL, c_int, _P]),
    "simamba_bn_relu_bwd_sums": (c_int, [_P, _P, _P, c_int, _P, _P, _P, _P, _P, _P, _P, _LL, c_int, _LL, c_int, _P]),
    "simamba_bn_relu_bwd_dx": (c_int, [_P, _P, _P, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _LL, c_int, _LL,
                                       c_int, _P]),
    "simamba_group_max_fwd": (c_int, [_P, _P, _P, _LL, c_int, c_int, c_int, _P]),
    "simamba_group_max_bwd": (c_int, [_P, _P, _P, _LL, c_int, c_int, c_int, _P]),
    "simamba_max_linear_bwd_slabs": (c_int, [_LL, c_int]),
    "simamba_max_linear_bwd_dx": (c_int, [_P, _P, _P, _P, _LL, c_int, c_int, c_int, c_int, _P]),
    "simamba_max_linear_bwd_dw": (c_int, [_P, _P, _P, _P, _P, _LL, c_int, c_int, c_int, c_int, _P]),
    "simamba_three_nn": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "simamba_three_interpolate_fwd": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "simamba_three_interpolate_bwd": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "simamba_gather_sum_scatter": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "simamba_chamfer_fwd": (c_int, [_P, _P, _P, _P, _P, _LL, c_int, c_int, _P]),
    "simamba_chamfer_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _LL, c_int, c_int, _P]),
    "simamba_chamfer_large_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _LL, c_int, c_int, _P]),
    "simamba_chamfer_large_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _LL, c_int, c_int, _P]),
    "simamba_chamfer_large_fwd_ex": (c_int, [_P, _P, _P, _P, _P, _P, _P, _LL, c_int, c_int, c_int, _P]),
    "simamba_chamfer_large_bwd_ex": (c_int, [_P, _P, _P, _P, _P, _P, _P, _LL, c_int, c_int, c_int, _P]),
    "simamba_chamfer_ragged_fwd": (c_int, [_P] * 9 + [_LL] + [c_int] * 6 + [_P]),
    "simamba_chamfer_ragged_bwd": (c_int, [_P] * 11 + [_LL] + [c_int] * 6 + [_P]),
    "simamba_emd_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _LL, c_int, c_float, c_int, _P]),
    "simamba_sinkhorn_workspace_bytes": (c_size_t, [_LL, c_int, c_int, c_int]),
    "simamba_sinkhorn_fwd": (c_int, [_P] * 12 + [_LL, c_int, c_int, c_float, c_int, c_int, _P, c_size_t, _P]),
    "simamba_sinkhorn_bwd": (c_int, [_P] * 11 + [_LL, c_int, c_int, c_float, c_int, _P, c_size_t, _P]),
    "simamba_part_seg_eval": (c_int, [_P] * 12 + [_LL, c_int, c_int, c_int, _P]),
    "simamba_svm_ovo_fit": (c_int, [_P] * 10 + [c_int, c_int, c_int, c_int, c_int, _P]),
    "simamba_svm_ovo_vote": (c_int, [_P, _P, _P, _P, _LL, c_int, _P]),
    "simamba_tsne_calibrate": (c_int, [_P, _P, _P, c_int, c_float, _P]),
    "simamba_tsne_workspace_floats": (_LL, [c_int]),
    "simamba_tsne_gradient": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_float, _P]),
    "simamba_tsne_run": (c_int, [_P] * 8 + [c_int, c_int, c_int, c_int, _P]),
    "simamba_optim_workspace_bytes": (c_size_t, [c_int, c_int]),
    "simamba_optim_adamw_step": (c_int, [_P] * 9 + [c_size_t, c_int, c_int, c_int, c_int, c_int, c_float, c_float,
                                         c_int, _P]),
    "simamba_augment_points": (c_int, [_P, _P, c_int, _P, _P, _P, _P, _P, c_int, _P, _LL, c_int, c_int, c_int, _P]),
    "simamba_augment_params": (c_int, [_P, _P, _P, c_int, _P, _P, _P, _P, _LL, c_int, _P]),
    "simamba_philox4x32_10": (c_int, [_LL, c_uint, c_uint, c_uint, c_uint, _P]),
    "simamba_dataset_fetch": (c_int, [_P] * 10 + [_LL, _LL, _LL, _LL, c_int, c_int, _LL, c_int, c_int, c_int, c_int,
                                      c_int, _P]),
    "simamba_keyed_perm": (c_int, [_LL, _LL, _LL, _LL, _LL, _P]),
    "simamba_corrupt_points": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, _P, _LL, c_int, c_int, _P]),
    "simamba_cutmix_points": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, _LL, c_int, _P]),
    "simamba_mix_draw": (c_int, [_P, _P, _P, _LL, _P]),
    "simamba_pointwolf_points": (c_int, [_P, _P, _P, _P, _P, c_int, _P, c_int, _LL, c_int, _P]),
    "simamba_knn_group": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "simamba_knn_group_ex": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "simamba_knn_graph": (c_int, [_P, _P, _P, c_size_t, c_int, c_int, c_int, c_int, c_float, c_uint, _P]),
    "simamba_laplacian_topk": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_uint, _P]),
    "simamba_laplacian_topk_workspace_bytes": (c_size_t, [c_int, c_int]),
    "simamba_laplacian_topk_ex": (c_int, [_P, _P, _P, _P, _P, c_size_t, c_int, c_int, c_int, c_uint, _P]),
    "simamba_spectral_workspace_bytes": (c_size_t, [c_int, c_int]),
    "simamba_spectral_topk": (c_int, [_P, _P, _P, _P, _P, c_size_t, c_int, c_int, c_int, c_float,
                                      c_int, c_uint, _P]),
    "simamba_argsort_rows": (c_int, [_P, _P, c_int, c_int, _P]),
    "simamba_curve_order": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_float, c_float, _P]),
    "simamba_farthest_point_sample": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P]),
    "simamba_farthest_point_sample_ex": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
}

_lib = None


def load():
    """Load the library once; raise (never fall back) when it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C si_mamba_amd/csrc`.  si_mamba_amd has no CPU / eager fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI and this table disagree
        fn.restype = res
        fn.argtypes = args
    got = lib.simamba_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"libsimamba_hip.so ABI version {got}, binding expects {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().simamba_strerror(rc).decode()
        raise RuntimeError(f"{what} failed (rc={rc}): {msg}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def dtype_code(dtype):
    import torch
    if dtype == torch.float32:
        return F32
    if dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"si_mamba_amd kernels take float32 or bfloat16 activations, got {dtype}")


def stream_ptr(device):
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def call(name, *args, device, time_as=None):
    """Launch C-ABI entry ``name`` on ``device``'s current stream.  ``args`` are the ABI's arguments WITHOUT the trailing
    stream (every launching entry point ends in ``void* stream``): a tensor stands for its data_ptr(), None for NULL,
    everything else (ints, floats, pre-offset addresses) passes through.  ``time_as``: bracket the call with
    ``timed(time_as, device)``.  A non-zero return raises through ``check(rc, name)``."""
    import torch
    fn = getattr(load(), name)
    Tensor = torch.Tensor
    argv = [a.data_ptr() if isinstance(a, Tensor) else a for a in args]
    argv.append(torch.cuda.current_stream(device).cuda_stream)
    with torch.cuda.device(device):
        if time_as is None:
            rc = fn(*argv)
        else:
            with timed(time_as, device):
                rc = fn(*argv)
    if rc:
        check(rc, name)


def require_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(
            f"{what}: tensor is on {t.device}; si_mamba_amd runs on a ROCm device only "
            "(no CPU fallback -- the CPU restatement lives in oracle/ and is test-only)")


# ---- optional per-kernel device timing (used by bench.py only) -----------------------------------
# When enabled, each C-ABI launch is bracketed by two events recorded on the stream it is enqueued
# on; nothing synchronises until `kernel_times()` is read after the timed region.
_timing = {"on": False, "events": {}, "only": None}


def enable_kernel_timing(on=True, only=None):
    """``only``: an iterable of kernel names to time (the others run without events).  A pair of event records per
    launch is not free: timing all ~100 launches per block stack costs the fp32 step 0.5 ms and makes the bf16 step
    CPU-bound (34 -> 41 ms), so bench.py times only the scan kernels inside its timed region."""
    _timing["on"] = bool(on)
    _timing["events"] = {}
    _timing["only"] = None if only is None else frozenset(only)


class timed:
    __slots__ = ("name", "dev", "ev")

    def __init__(self, name, device):
        self.name, self.dev, self.ev = name, device, None

    def __enter__(self):
        if _timing["on"] and (_timing["only"] is None or self.name in _timing["only"]):
            import torch
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(torch.cuda.current_stream(self.dev))
            self.ev = (a, b)
        return self

    def __exit__(self, *exc):
        if self.ev is not None:
            import torch
            self.ev[1].record(torch.cuda.current_stream(self.dev))
            _timing["events"].setdefault(self.name, []).append(self.ev)
        return False


def kernel_times():
    """name -> (launches, mean ms); call after torch.cuda.synchronize()."""
    out = {}
    for name, evs in _timing["events"].items():
        ms = [a.elapsed_time(b) for a, b in evs]
        out[name] = (len(ms), sum(ms) / max(len(ms), 1))
    return out


class _Override:
    """A module-level one-element list (``cell``, read through ``[0]``) and the context manager that sets it for a block;
    ``coerce`` maps the argument to the value stored."""
    cell = None
    coerce = bool

    def __init__(self, on):
        self.v, self.prev = self.coerce(on), None

    def __enter__(self):
        self.prev, self.cell[0] = self.cell[0], self.v
        return self

    def __exit__(self, *exc):
        self.cell[0] = self.prev
        return False


def _tristate(on):
    return None if on is None else bool(on)


_scan_variant = [SCAN_AUTO]


class scan_variant(_Override):
    """Context manager for benchmarks and parity tests: the forward-scan kernel the Python ops request from the
    library inside the block (an explicit argument of simamba_selective_scan_fwd -- the library itself holds no
    state and reads no environment).  Production code never enters it: SCAN_AUTO lets the library choose."""
    cell, coerce = _scan_variant, int

    def __init__(self, variant):
        super().__init__(variant)


def current_scan_variant():
    return _scan_variant[0]


_scan_ckpt = [0]


class scan_ckpt(_Override):
    """Context manager for benchmarks and parity tests: the checkpoint layout (CKPT_ROW / CKPT_SEQ, i.e. the backward
    kernel) the Python ops request instead of the library's own choice.  Production code never enters it."""
    cell, coerce = _scan_ckpt, int

    def __init__(self, step):
        super().__init__(step)


_spectral_large_g = [False]


class spectral_large_g(_Override):
    """Context manager for parity tests and benchmarks: top-k eigenpairs through the large-G kernel
    (simamba_laplacian_topk_ex with SPEC_LARGE_G) at G <= 128 too, where the library otherwise runs the LDS-resident
    tridiagonal kernel.  Production code never enters it: above 128 patches the large-G kernel is the only route."""
    cell = _spectral_large_g

    def __init__(self, on=True):
        super().__init__(on)


def spectral_large_g_forced():
    return _spectral_large_g[0]


_fuse_dt = [None]      # None: the measured default (bf16 I/O only, see fuse_dt_enabled); True / False: forced
counters = {}          # name -> how often a route was taken (tests assert on them; nothing in the product reads them)


def count(name):
    counters[name] = counters.get(name, 0) + 1


class scan_fuse_dt(_Override):
    """Context manager for benchmarks and parity tests: force the mixer to let the scan kernels form delta themselves
    (simamba_selective_scan_dt_fwd / _bwd) wherever they can (True), or to materialise it as upstream does (False).
    Production never enters it and gets the measured default of fuse_dt_enabled()."""
    cell, coerce = _fuse_dt, staticmethod(_tristate)


def fuse_dt_enabled(dtype):
    """Default: bf16 I/O only.  Measured at (64, 768, 1024), per layer, conv + x_proj (+ dt_proj) / scan forward / scan
    backward (tools/bench_dt_fusion.py, profiles/r03b_dt_fusion.txt): bf16 96 + 315 + 691 us with delta materialised,
    62 + 314 + 691 us formed in the scans (two bf16 MFMAs per tile: free); fp32 168 + 308 + 691 us against 126 + 356 +
    790 us -- the exact-fp32 MFMA runs at the vector rate, and inside the VALU-bound scans its 12 instructions per tile
    are additive, while inside the xdt kernel (bound by bytes in flight) they are hidden."""
    import torch
    return (dtype == torch.bfloat16) if _fuse_dt[0] is None else _fuse_dt[0]


_fuse_out_norm = [True]
_hand_in_proj = [None]   # None: the measured default (in_proj_hand_enabled); True / False: forced


class fuse_out_norm(_Override):
    """Context manager for benchmarks and parity tests: let MixerModel.forward apply out_proj fused with the next block's
    add + LayerNorm (out_norm.py; the default wherever the kernel's shapes apply) or op by op as the reference does."""
    cell = _fuse_out_norm


def fuse_out_norm_enabled():
    return _fuse_out_norm[0]


_drop_path_compact = [os.environ.get("SIMAMBA_DROP_PATH_COMPACT", "1").strip().lower() not in ("0", "false", "off")]
DROP_PATH_BUCKET = 4          # compact batches are rounded up to a multiple of this many samples
compact_sizes = {}            # compact batch -> how many mixer calls ran at it (read by benchmarks and tests)


class drop_path_compact(_Override):
    """Context manager: let MixerModel run every mixer only on the samples the NEXT block's DropPath keeps (block.py,
    compact add + norm kernels) or on the whole batch as the reference does.  On by default; the environment variable
    SIMAMBA_DROP_PATH_COMPACT=0 switches it off for a whole process."""
    cell = _drop_path_compact


def drop_path_compact_enabled():
    return _drop_path_compact[0]


_sparse_max_linear = [None]   # None: the measured default (sparse_max_linear_enabled); True / False: forced


class sparse_max_linear(_Override):
    """Context manager for benchmarks and parity tests: the encoder's last layer (linear, then max over the patch) with
    the sparse backward of csrc/encoder_sparse.hip wherever its shapes apply (True), or as token_linear + group_max_fn
    with the dense gradient between them (False).  Production never enters it and gets the measured default."""
    cell, coerce = _sparse_max_linear, staticmethod(_tristate)


def sparse_max_linear_enabled(dtype):
    """Default: fp32 I/O only.  Measured at (8192 patches, 32 points, 512 -> 384), the whole backward of the pair
    (tools/bench_encoder.py, profiles/encoder_sparse_kernels.txt): fp32 877 us sparse against 1 734 us dense (the two
    exact-fp32 GEMMs run 103 GFLOP each on 31/32 zeros); bf16 904 us sparse against 489 us dense -- the bf16 MFMA does
    each of those GEMMs in ~0.1 ms, less than the sparse kernels' latency-bound LDS loops take, so bf16 keeps the dense
    route."""
    import torch
    return (dtype == torch.float32) if _sparse_max_linear[0] is None else _sparse_max_linear[0]


class hand_in_proj(_Override):
    """Context manager for benchmarks and parity tests: in_proj through the hand-written bf16 kernel
    (simamba_in_proj_fwd) wherever its shapes apply (True) or through the library GEMM (False)."""
    cell, coerce = _hand_in_proj, staticmethod(_tristate)


def in_proj_hand_enabled(workgroups, dtype=None):
    """Default: bf16 only (102 us against 116 us for the library GEMM; the fp32 form measured 650 against 535 us and stays an
    explicit variant), and only grids that fill the chip (a workgroup owns 256 tokens of one sample, alone on its CU)."""
    import torch
    if _hand_in_proj[0] is not None:
        return _hand_in_proj[0]
    return dtype != torch.float32 and workgroups >= IN_PROJ_MIN_WORKGROUPS


IN_PROJ_MIN_WORKGROUPS = 192


def scan_plan_step(batch, dim, seqlen, dstate, dtype, *, softplus=True, has_z=True, act_addr_or=0, a_addr=0,
                   b_addr=0, c_addr=0, z_bs=0, dz_bs=0, bc_strides=(0, 0, 0)):
    """The checkpoint step of one forward / backward pair: CKPT_SEQ only where the library's row-count rule picks it
    (simamba_scan_ckpt_step) AND both sequential entry points would take these operands
    (simamba_scan_seq_applicable: B / C packs and strides per dtype, A, every batch stride and the 2^30 offset
    bounds); CKPT_ROW -- the row-scan pair, which reads anything -- otherwise.  Host arithmetic only.
    ``act_addr_or``: OR of the addresses of all activation-sized operands; strides in elements, 0 = contiguous."""
    lib = load()
    code = dtype_code(dtype)
    step = _scan_ckpt[0] or lib.simamba_scan_ckpt_step(batch, dim, seqlen, dstate, code)
    if step == CKPT_SEQ and not lib.simamba_scan_seq_applicable(
            batch, dim, seqlen, dstate, code, int(bool(softplus)), int(bool(has_z)), act_addr_or, a_addr, b_addr,
            c_addr, z_bs, dz_bs, *bc_strides):
        step = CKPT_ROW
    if _scan_variant[0] == SCAN_ROWSCAN:
        step = CKPT_ROW                 # an explicit row-scan forward writes 128-step checkpoints only
    return step


def mixer_scan_operands(xz_addr, a_addr, dim, seqlen, dt_rank, dstate, esz, xz_bs):
    """scan_plan_step's operand description of the fused mixer's scan (mamba_inner.MambaInnerFn), stated before most of
    the operands exist: z / dz are the second halves of xz (B, 2 dim, L) and of a dxz with the same strides, every
    other activation-sized tensor is a fresh allocation (16-byte aligned), and B / C are the columns [R, R + N) and
    [R + N, S) of the token-major x_proj output (B, L, S = R + 2N) -- off a pack boundary, and with a token stride that
    is no multiple of the pack, when R % 4 != 0 (d_model = 32 * odd).  x_dbl's own base only has to be 16-byte
    aligned, so B / C are described by their offsets from it."""
    S = dt_rank + 2 * dstate
    return dict(softplus=True, has_z=True, act_addr_or=xz_addr | (xz_addr + dim * seqlen * esz), a_addr=a_addr,
                b_addr=dt_rank * esz, c_addr=(dt_rank + dstate) * esz, z_bs=xz_bs, dz_bs=xz_bs,
                bc_strides=(seqlen * S, 1, S))


def scan_plan(batch, dim, seqlen, dstate, dtype, device, need_grad, **operands):
    """(ckpt_step, x_ckpt or None) for one forward / backward pair; ``operands``: scan_plan_step's description of what
    the two calls will be handed (x_ckpt itself comes from the allocator, 16-byte aligned)."""
    import torch
    step = scan_plan_step(batch, dim, seqlen, dstate, dtype, **operands)
    count("scan_ckpt_seq" if step == CKPT_SEQ else "scan_ckpt_row")
    if not need_grad:
        return step, None
    n = load().simamba_scan_ckpt_floats(batch, dim, seqlen, dstate, step)
    return step, (torch.empty(n, device=device, dtype=torch.float32) if n else None)


def scan_bwd_accumulators(batch, dim, seqlen, dstate, has_D, has_bias, device):
    """(dA (D,N), dB (B,N,L), dC (B,N,L), dD (D)|None, ddelta_bias (D)|None): the fp32 accumulators
    simamba_selective_scan_bwd adds into, carved back to back (no padding between them) out of ONE allocation.
    The library zeroes exactly-adjacent spans with one memset node; it never writes outside the spans it is
    given, so separately allocated buffers are equally valid, only slower to clear (include/simamba.h)."""
    import torch
    sizes = [dim * dstate, batch * dstate * seqlen, batch * dstate * seqlen, dim if has_D else 0,
             dim if has_bias else 0]
    flat = torch.empty(sum(sizes), device=device, dtype=torch.float32)
    parts, o = [], 0
    for n in sizes:
        parts.append(flat[o:o + n])
        o += n
    dA = parts[0].view(dim, dstate)
    dB = parts[1].view(batch, dstate, seqlen)
    dC = parts[2].view(batch, dstate, seqlen)
    return dA, dB, dC, (parts[3] if has_D else None), (parts[4] if has_bias else None)


# ---- deterministic backward ------------------------------------------------------------------------------------------
_deterministic = [None]   # None: follow torch.are_deterministic_algorithms_enabled(); True / False: forced


def set_deterministic(on):
    """Deterministic backward of the scan and conv1d kernels (SIMAMBA_BWD_DETERMINISTIC: per-workgroup partials and a
    fixed-order sum instead of float atomics; bitwise reproducible gradients).  ``True`` / ``False`` force it on / off,
    ``None`` (the default) follows ``torch.use_deterministic_algorithms``.  ``torch.backends.cudnn.deterministic`` is
    not consulted."""
    _deterministic[0] = _tristate(on)


class deterministic(_Override):
    """Context manager form of set_deterministic: ``with deterministic(True): loss.backward()``."""
    cell, coerce = _deterministic, staticmethod(_tristate)


def deterministic_enabled():
    """True when the backward kernels run their deterministic form: the explicit override if one is set, else
    torch.are_deterministic_algorithms_enabled()."""
    if _deterministic[0] is not None:
        return _deterministic[0]
    import torch
    return torch.are_deterministic_algorithms_enabled()


def det_args(workspace_query, *dims, device):
    """(flags, workspace or None, its size in floats) for an *_ex backward call: (0, None, 0) unless
    deterministic_enabled(), else BWD_DETERMINISTIC and ``workspace_query(*dims, BWD_DETERMINISTIC)`` floats (the
    library's *_workspace_floats(); a negative value is an argument error the call itself reports).  The workspace
    comes from torch's caching allocator, so the route is captured by torch.cuda.graph like any other."""
    if not deterministic_enabled():
        return 0, None, 0
    import torch
    n_floats = workspace_query(*dims, BWD_DETERMINISTIC)
    if n_floats <= 0:
        return BWD_DETERMINISTIC, None, 0
    return BWD_DETERMINISTIC, torch.empty(n_floats, device=device, dtype=torch.float32), n_floats
