"""CPU: the C ABI of ragged point-cloud batches (include/simamba.h: simamba_farthest_point_sample_ex,
simamba_knn_group_ex) -- symbols, prototypes, argument validation before any launch, the unchanged ABI version -- and
the pytorch3d stand-ins accepting ``lengths`` up to the point where a ROCm device is required."""
import ctypes
import inspect

import pytest
import torch

from abi_tables import E_NULLPTR, E_SHAPE
from si_mamba_amd import _lib, grouping

NEW = ["simamba_farthest_point_sample_ex", "simamba_knn_group_ex"]


def test_symbols_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    # the old entry points with the optional pointers inserted after the inputs
    P = ctypes.c_void_p
    old = _lib.SIGNATURES["simamba_farthest_point_sample"][1]
    assert _lib.SIGNATURES["simamba_farthest_point_sample_ex"][1] == old[:1] + [P, P] + old[1:]
    old = _lib.SIGNATURES["simamba_knn_group"][1]
    assert _lib.SIGNATURES["simamba_knn_group_ex"][1] == old[:2] + [P, P] + old[2:]
    assert _lib.load().simamba_abi_version() == 9
    assert _lib.ABI_VERSION == 9


def test_fps_ex_validation_precedes_any_launch():
    lib = _lib.load()
    fps = lib.simamba_farthest_point_sample_ex
    one = ctypes.c_void_p(16)                # never dereferenced: every call below returns before a launch
    n = None
    for lengths, start in [(n, n), (one, n), (n, one), (one, one)]:
        assert fps(one, lengths, start, one, n, 1, 8193, 512, n) == E_SHAPE         # N > 8192
        assert fps(one, lengths, start, one, n, 1, 8192, 8193, n) == E_SHAPE        # K <= N also with lengths
        assert fps(one, lengths, start, one, n, -1, 1024, 128, n) == E_SHAPE
        assert fps(one, lengths, start, one, n, 1, 0, 0, n) == E_SHAPE
        assert fps(n, lengths, start, one, n, 1, 1024, 128, n) == E_NULLPTR         # points
        assert fps(one, lengths, start, n, n, 1, 1024, 128, n) == E_NULLPTR         # idx
        assert fps(n, lengths, start, n, n, 0, 8192, 512, n) == 0                   # empty batch: nothing to do
        assert fps(n, lengths, start, n, n, 4, 1024, 0, n) == 0                     # no picks: nothing to do
    # the old entry point answers the same
    old = lib.simamba_farthest_point_sample
    assert old(one, one, n, 1, 8193, 512, n) == E_SHAPE
    assert old(n, one, n, 1, 1024, 128, n) == E_NULLPTR


def test_knn_group_ex_validation_precedes_any_launch():
    lib = _lib.load()
    knn = lib.simamba_knn_group_ex
    one = ctypes.c_void_p(16)
    n = None
    for lp, lc in [(n, n), (one, n), (n, one), (one, one)]:
        assert knn(one, one, lp, lc, one, 1, 8193, 128, 32, n) == E_SHAPE           # N > 8192
        assert knn(one, one, lp, lc, one, 1, 16, 4, 32, n) == E_SHAPE               # K <= N also with lengths
        assert knn(one, one, lp, lc, one, 1, 1024, 128, 0, n) == E_SHAPE
        assert knn(one, one, lp, lc, one, 65536, 1024, 128, 32, n) == E_SHAPE
        assert knn(n, one, lp, lc, one, 1, 1024, 128, 32, n) == E_NULLPTR           # points
        assert knn(one, n, lp, lc, one, 1, 1024, 128, 32, n) == E_NULLPTR           # centers
        assert knn(one, one, lp, lc, n, 1, 1024, 128, 32, n) == E_NULLPTR           # idx
        assert knn(n, n, lp, lc, n, 0, 1024, 128, 32, n) == 0                       # empty batch
        assert knn(n, n, lp, lc, n, 2, 1024, 0, 32, n) == 0                         # no centres
    old = lib.simamba_knn_group
    assert old(one, one, one, 1, 8193, 128, 32, n) == E_SHAPE
    assert old(n, one, one, 1, 1024, 128, 32, n) == E_NULLPTR


def test_python_signatures():
    """The new arguments follow the existing positional ones, so two- and three-argument calls mean what they did."""
    assert list(inspect.signature(grouping.sample_farthest_points).parameters) == ["points", "K", "lengths", "start_idx"]
    assert list(inspect.signature(grouping.knn_group).parameters) == ["centers", "points", "K", "lengths",
                                                                      "center_lengths"]
    from si_mamba_amd.mae import Point_MAE_Mamba
    from si_mamba_amd.point_mamba import Group, PointMamba
    from si_mamba_amd.seg import PartSegMamba
    for cls in (Group, PointMamba, PartSegMamba):
        prm = inspect.signature(cls.forward).parameters["lengths"]
        assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default is None, cls
    assert inspect.signature(Point_MAE_Mamba.forward).parameters["lengths"].default is None
    # the reference's positional arguments of PointMamba.forward are where they were
    assert list(inspect.signature(PointMamba.forward).parameters)[:7] == ["self", "pts", "gt", "tau", "use_wavelets",
                                                                          "save_pts_dir", "epoch"]


def test_per_cloud_arguments_are_checked_on_the_host_by_shape_and_dtype_only():
    dev = torch.device("cpu")
    assert grouping._per_cloud(None, 4, dev, "lengths") is None
    got = grouping._per_cloud(torch.tensor([3, 4, 5, 6], dtype=torch.int32), 4, dev, "lengths")
    assert got.dtype == torch.int64 and got.tolist() == [3, 4, 5, 6]
    with pytest.raises(ValueError, match="shape"):
        grouping._per_cloud(torch.tensor([3, 4, 5]), 4, dev, "lengths")
    with pytest.raises(TypeError, match="integers"):
        grouping._per_cloud(torch.tensor([3., 4., 5., 6.]), 4, dev, "lengths")


def test_shim_accepts_lengths_up_to_the_device_check():
    """On a CPU tensor the stand-ins no longer refuse ``lengths`` / ``random_start_point``: they reach the ops, whose
    only complaint is the missing ROCm device."""
    import sys

    from si_mamba_amd.shim import install_shim
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in ("mamba_ssm", "causal_conv1d", "pytorch3d")}
    try:
        install_shim(force=True, pytorch3d=True)
        from pytorch3d.ops import knn_points, sample_farthest_points
        p = torch.randn(2, 64, 3)
        c = torch.randn(2, 8, 3)
        ln = torch.tensor([40, 64])
        for kw in (dict(lengths=ln), dict(random_start_point=True), dict(lengths=ln, random_start_point=True)):
            with pytest.raises(RuntimeError, match="ROCm device only"):
                sample_farthest_points(p, K=8, **kw)
        for kw in (dict(lengths2=ln), dict(lengths1=torch.tensor([8, 5])), dict(lengths1=torch.tensor([8, 5]), lengths2=ln)):
            with pytest.raises(RuntimeError, match="ROCm device only"):
                knn_points(c, p, K=4, return_sorted=False, **kw)
        with pytest.raises(NotImplementedError):
            knn_points(c, p, lengths2=ln, K=4, norm=1)
        with pytest.raises(NotImplementedError):
            knn_points(c, p, lengths2=ln, K=4, return_nn=True)
        from pytorch3d.loss import chamfer_distance
        with pytest.raises(NotImplementedError):
            chamfer_distance(c, c, x_lengths=torch.tensor([8, 5]))
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] in ("mamba_ssm", "causal_conv1d", "pytorch3d")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_models_refuse_lengths_where_it_is_not_built():
    """PartSegMamba and Point_MAE_Mamba name the argument; no device is needed to get that far."""
    from si_mamba_amd.mae import Point_MAE_Mamba
    from si_mamba_amd.seg import PartSegMamba
    ln = torch.tensor([100, 128])
    with pytest.raises(NotImplementedError, match="lengths"):
        PartSegMamba.forward(None, torch.zeros(2, 3, 128), torch.zeros(2, 16), lengths=ln)
    with pytest.raises(NotImplementedError, match="lengths"):
        Point_MAE_Mamba.forward(None, torch.zeros(2, 128, 3), lengths=ln)


def test_both_instantiations_of_every_kernel_are_shipped(tmp_path):
    """The code object holds the fixed-length (kRagged = false) and the ragged instantiation of the two FPS kernels and
    of the four k-NN grouping kernels, and nothing else under those names."""
    import re
    import subprocess

    import test_deterministic_abi as t
    if not (t._OBJCOPY and t._OBJDUMP):
        pytest.skip("ROCm llvm-objcopy / llvm-objdump not installed")
    fb = tmp_path / "fatbin"
    subprocess.run([t._OBJCOPY, "--dump-section", f".hip_fatbin={fb}", _lib.LIB_PATH, str(tmp_path / "stripped")],
                   check=True)
    names = []
    for k, co in enumerate(t._gfx950_code_objects(fb.read_bytes())):
        p = tmp_path / f"{k}.co"
        p.write_bytes(co)
        txt = subprocess.run([t._OBJDUMP, "-t", str(p)], capture_output=True, text=True, check=True).stdout
        names += re.findall(r"\b_ZN7simamba\d+(?:fps_kernel|fps_wide_kernel|knn_group_kernel)\w+", txt)
    names = sorted(set(names))                       # a kernel and its descriptor (<name>.kd) share the name
    want = [f"fps_kernelILb{r}E" for r in (0, 1)] + [f"fps_wide_kernelILb{r}E" for r in (0, 1)] + \
           [f"knn_group_kernelILi{per}ELb{r}E" for per in (16, 32, 64, 128) for r in (0, 1)]
    assert len(names) == len(want), names
    for w in want:
        assert sum(w in n for n in names) == 1, (w, names)
