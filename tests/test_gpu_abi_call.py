"""GPU: _lib.call, the one launch path of the Python ops -- the error names the symbol that was called, None goes out
as NULL and a tensor as its address, events are recorded only with time_as -- and the dense Chamfer route after its
fold into the ragged Function: the bits and counters of simamba_chamfer_large_fwd / _bwd."""
import re

import pytest
import torch

from si_mamba_amd import _lib
from si_mamba_amd.mae import chamfer_distance

pytestmark = pytest.mark.gpu


def test_error_names_the_called_symbol(device):
    """n = 0 is refused by the shape check in front of everything else (SIMAMBA_E_SHAPE): nothing is launched."""
    x = torch.zeros(1, 1, 3, device=device)
    out = torch.zeros(1, device=device)
    idx = torch.zeros(1, 1, device=device, dtype=torch.int32)
    with pytest.raises(RuntimeError) as err:
        _lib.call("simamba_chamfer_ragged_fwd", x, x, None, None, out, idx, idx, out, out, 1, 0, 1, 2, 0, 0, 0,
                  device=device)
    msg = str(err.value)
    assert re.findall(r"simamba_\w+", msg) == ["simamba_chamfer_ragged_fwd"], msg
    assert "rc=-2" in msg and "bad shape" in msg, msg


def test_null_tensor_and_timing(device):
    vals = torch.tensor([[3.0, 1.0, 2.0, 1.0, 0.0], [0.5, 0.5, -1.0, 4.0, 0.5]], device=device)
    want = torch.sort(vals, dim=1, stable=True)[1]
    # None reaches the library as NULL: both pointers are required, so the call is refused before any launch
    for args in ((None, torch.empty(2, 5, device=device, dtype=torch.int64)), (vals, None)):
        with pytest.raises(RuntimeError, match=r"simamba_argsort_rows failed \(rc=-1\)"):
            _lib.call("simamba_argsort_rows", *args, 2, 5, device=device)
    _lib.enable_kernel_timing(True)
    try:
        idx = torch.full((2, 5), -1, device=device, dtype=torch.int64)
        _lib.call("simamba_argsort_rows", vals, idx, 2, 5, device=device, time_as="t")
        torch.cuda.synchronize()
        assert torch.equal(idx, want)
        assert _lib.kernel_times()["t"][0] == 1
        idx.fill_(-1)
        _lib.call("simamba_argsort_rows", vals, idx, 2, 5, device=device)
        torch.cuda.synchronize()
        assert torch.equal(idx, want)
        assert {k: v[0] for k, v in _lib.kernel_times().items()} == {"t": 1}
    finally:
        _lib.enable_kernel_timing(False)


def test_dense_chamfer_is_the_large_entry_points_bit_for_bit(device):
    """(3, 65, 3): one point over the one-wave limit, the other set smaller than a wave."""
    pairs, n, m = 3, 65, 3
    gen = torch.Generator().manual_seed(11)
    x, y = torch.randn(pairs, n, 3, generator=gen).to(device), torch.randn(pairs, m, 3, generator=gen).to(device)
    gd = torch.rand(pairs, generator=gen).to(device)

    pred, gt = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    before = dict(_lib.counters)
    dist = chamfer_distance(pred, gt)
    dist.backward(gd)
    assert _lib.counters.get("chamfer_large", 0) == before.get("chamfer_large", 0) + 1
    assert _lib.counters.get("chamfer_ragged", 0) == before.get("chamfer_ragged", 0)
    assert _lib.counters.get("chamfer_small", 0) == before.get("chamfer_small", 0)

    lib, st = _lib.load(), _lib.stream_ptr(device)
    want = torch.empty(pairs, device=device)
    i1 = torch.empty(pairs, n, device=device, dtype=torch.int32)
    i2 = torch.empty(pairs, m, device=device, dtype=torch.int32)
    d1, d2 = torch.empty(pairs, n, device=device), torch.empty(pairs, m, device=device)
    dx, dy = torch.empty_like(x), torch.empty_like(y)
    assert lib.simamba_chamfer_large_fwd(x.data_ptr(), y.data_ptr(), want.data_ptr(), i1.data_ptr(), i2.data_ptr(),
                                         d1.data_ptr(), d2.data_ptr(), pairs, n, m, st) == 0
    assert lib.simamba_chamfer_large_bwd(x.data_ptr(), y.data_ptr(), gd.data_ptr(), i1.data_ptr(), i2.data_ptr(),
                                         dx.data_ptr(), dy.data_ptr(), pairs, n, m, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(dist.detach(), want)
    assert torch.equal(pred.grad, dx)
    assert torch.equal(gt.grad, dy)
