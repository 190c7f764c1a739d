"""CPU: the Sinkhorn divergence entry points (csrc/sinkhorn.hip) validate their arguments in the stated order before
touching a device, the workspace query answers what the calls ask for, and the Python route checks its own arguments
and did not grow a host implementation."""
import pytest
import torch

from abi_tables import E_ALIGN, E_NULLPTR, E_SHAPE, E_VARIANT, E_WORKSPACE, OFF, P, check_rows
from si_mamba_amd import _lib

BIG = 1 << 40

FWD = dict(x=P, y=P, xlen=None, ylen=None, div=P, ot_xy=P, merr=P, f_xy=P, g_xy=P, g_xx=P, g_yy=P, f_yy=P, pairs=2,
           n=100, m=70, eps_rel=2.0 ** -6, iters=16, flags=1, workspace=None, workspace_bytes=BIG, stream=None)
BWD = dict(x=P, y=P, xlen=None, ylen=None, ddiv=P, f_xy=P, g_xy=P, g_xx=P, f_yy=P, dx=P, dy=P, pairs=2, n=100, m=70,
           eps_rel=2.0 ** -6, flags=1, workspace=None, workspace_bytes=BIG, stream=None)

# Every row ends in validation: the base call has every pointer but the workspace, so a row that passes the checks in
# front of it answers E_WORKSPACE without a launch; a row with workspace=OFF and enough bytes answers E_ALIGN, the last
# check of all.
SHAPE_ROWS = [
    (dict(n=0), E_SHAPE), (dict(n=-1), E_SHAPE), (dict(n=8193), E_SHAPE), (dict(m=0), E_SHAPE), (dict(m=8193), E_SHAPE),
    (dict(pairs=0), E_SHAPE), (dict(pairs=-1), E_SHAPE),
    (dict(pairs=1 << 40), E_SHAPE), (dict(pairs=1 << 26, n=8192, m=8192), E_SHAPE),      # more workgroups than a grid holds
    (dict(eps_rel=0.0), E_SHAPE), (dict(eps_rel=-0.5), E_SHAPE), (dict(eps_rel=1.5), E_SHAPE),
    (dict(eps_rel=float("nan")), E_SHAPE), (dict(eps_rel=float("inf")), E_SHAPE),
    (dict(flags=2), E_VARIANT), (dict(flags=3), E_VARIANT), (dict(flags=-1), E_VARIANT),
    (dict(x=None), E_NULLPTR), (dict(y=None), E_NULLPTR),
    # the limits themselves pass every check in front of the workspace
    (dict(n=1, m=1), E_WORKSPACE), (dict(n=8192, m=8192), E_WORKSPACE), (dict(eps_rel=1.0), E_WORKSPACE),
    (dict(xlen=P, ylen=P), E_WORKSPACE), (dict(flags=0), E_WORKSPACE),
    (dict(workspace=P, workspace_bytes=0), E_WORKSPACE), (dict(workspace=OFF), E_ALIGN),
    # two faults: flags, then shape, then null pointers, then the workspace
    (dict(flags=2, n=0), E_VARIANT), (dict(flags=2, x=None), E_VARIANT), (dict(n=0, x=None), E_SHAPE),
    (dict(eps_rel=0.0, y=None), E_SHAPE), (dict(pairs=0, workspace=OFF), E_SHAPE), (dict(x=None, workspace=OFF), E_NULLPTR),
    (dict(workspace=OFF, workspace_bytes=0), E_WORKSPACE),
]
FWD_ROWS = SHAPE_ROWS + [
    (dict(iters=-1), E_SHAPE), (dict(iters=4091), E_SHAPE), (dict(iters=4090), E_WORKSPACE),     # S = 6: 6 + 4090 = 4096
    (dict(eps_rel=1.0, iters=0), E_SHAPE), (dict(eps_rel=1.0, iters=1), E_WORKSPACE),           # S = 0: one step at least
    (dict(eps_rel=1.0, iters=4097), E_SHAPE), (dict(eps_rel=0.5, iters=0), E_WORKSPACE),
    (dict(eps_rel=1e-45, iters=0), E_WORKSPACE),                                                  # S = 149
    (dict(div=None), E_NULLPTR), (dict(ot_xy=None), E_NULLPTR), (dict(f_xy=None), E_NULLPTR), (dict(g_xy=None), E_NULLPTR),
    (dict(g_xx=None), E_NULLPTR), (dict(g_yy=None), E_NULLPTR), (dict(f_yy=None), E_NULLPTR),
    (dict(merr=None), E_WORKSPACE),                                                               # optional
    (dict(flags=0, g_xx=None, g_yy=None, f_yy=None), E_WORKSPACE),                                # not touched without debias
    (dict(iters=-1, div=None), E_SHAPE), (dict(flags=4, iters=-1), E_VARIANT),
]
BWD_ROWS = SHAPE_ROWS + [
    (dict(ddiv=None), E_NULLPTR), (dict(g_xy=None), E_NULLPTR), (dict(g_xx=None), E_NULLPTR), (dict(f_xy=None), E_NULLPTR),
    (dict(f_yy=None), E_NULLPTR),
    # a skipped gradient does not need the potentials only it reads
    (dict(dx=None, g_xy=None, g_xx=None), E_WORKSPACE), (dict(dy=None, f_xy=None, f_yy=None), E_WORKSPACE),
    (dict(flags=0, g_xx=None, f_yy=None), E_WORKSPACE), (dict(dx=None, dy=None), E_WORKSPACE),
]


@pytest.mark.parametrize("name,base,rows", [("simamba_sinkhorn_fwd", FWD, FWD_ROWS),
                                            ("simamba_sinkhorn_bwd", BWD, BWD_ROWS)])
def test_return_codes_without_a_device(name, base, rows):
    check_rows(name, base, rows)


def test_workspace_bytes():
    q = _lib.load().simamba_sinkhorn_workspace_bytes
    # diam2 (pairs), the per-row marginal errors (pairs, n), and with debias f_xx (pairs, n)
    assert q(2, 100, 70, 1) == 4 * 2 * (1 + 2 * 100)
    assert q(2, 100, 70, 0) == 4 * 2 * (1 + 100)
    assert q(64, 2048, 1024, 1) == 4 * 64 * (1 + 2 * 2048)
    assert q(1, 8192, 8192, 1) == 4 * (1 + 2 * 8192)
    # arguments the calls refuse
    for bad in [(0, 100, 70, 1), (2, 0, 70, 1), (2, 100, 8193, 1), (2, 100, 70, 2), (1 << 40, 100, 70, 1)]:
        assert q(*bad) == 0, bad
    # the calls compare against the query: one byte short is refused, and the backward needs 4 * pairs bytes
    need = q(2, 100, 70, 1)
    check_rows("simamba_sinkhorn_fwd", FWD, [(dict(workspace=P, workspace_bytes=need - 1), E_WORKSPACE),
                                             (dict(workspace=OFF, workspace_bytes=need), E_ALIGN)])
    check_rows("simamba_sinkhorn_bwd", BWD, [(dict(workspace=P, workspace_bytes=7), E_WORKSPACE),
                                             (dict(workspace=OFF, workspace_bytes=8), E_ALIGN)])


def test_python_route_refuses_cpu_tensors():
    from si_mamba_amd import sinkhorn_divergence
    a, b = torch.zeros(2, 32, 3), torch.zeros(2, 48, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sinkhorn_divergence(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sinkhorn_divergence(a[0], b[0], return_info=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sinkhorn_divergence(a.clone().requires_grad_(), b.clone().requires_grad_(), debias=False)


def test_python_route_checks_its_arguments_first():
    import si_mamba_amd
    from si_mamba_amd import sinkhorn_divergence
    from si_mamba_amd.sinkhorn import scaling_steps
    assert "sinkhorn_divergence" in si_mamba_amd.__all__
    z = torch.zeros
    ok = (z(2, 32, 3), z(2, 48, 3))
    for x, y, kw in [(z(2, 32, 3), z(3, 32, 3), {}), (z(2, 32, 2), z(2, 32, 2), {}), (z(2, 32, 3), z(2, 32, 4), {}),
                     (z(2, 8193, 3), z(2, 32, 3), {}), (z(2, 32, 3), z(2, 8193, 3), {}), (z(0, 32, 3), z(0, 32, 3), {}),
                     (z(2, 0, 3), z(2, 32, 3), {}), (z(32), z(32), {}), (z(32, 3), z(2, 32, 3), {}),
                     (*ok, dict(eps_rel=0.0)), (*ok, dict(eps_rel=-1.0)), (*ok, dict(eps_rel=1.5)),
                     (*ok, dict(eps_rel=float("nan"))), (*ok, dict(eps_rel=1e-50)), (*ok, dict(iters=-1)),
                     (*ok, dict(eps_rel=1.0, iters=0)),
                     (*ok, dict(iters=4091)), (*ok, dict(x_lengths=torch.zeros(3, dtype=torch.int32))),
                     (*ok, dict(y_lengths=torch.zeros(2))), (*ok, dict(x_lengths=[32, 32]))]:
        with pytest.raises(ValueError):
            sinkhorn_divergence(x, y, **kw)
    assert [scaling_steps(e) for e in (1.0, 0.5, 0.3, 2.0 ** -6, 2.0 ** -9, 1e-45)] == [0, 1, 2, 6, 9, 149]


def test_lengths_reach_the_kernels_as_int32_without_wrapping():
    """2^32 + 5 must not become 5, a length the kernel would take as valid: it stays at least every padded size."""
    from si_mamba_amd import sinkhorn
    from si_mamba_amd._pointsets import lengths_i32
    t = torch.tensor([2 ** 32 + 5, -7, 3], dtype=torch.int64)
    want = torch.tensor([1 << 20, -1, 3], dtype=torch.int32)
    for got in (lengths_i32(t), sinkhorn._lengths(t, torch.device("cpu"))):
        assert got.dtype == torch.int32 and got.is_contiguous() and torch.equal(got, want)
    assert lengths_i32(None) is None and sinkhorn._lengths(None, torch.device("cpu")) is None
    # every integer dtype is taken, as before the clamp: its bounds must not be converted to the narrow type
    for dtype in (torch.int8, torch.uint8, torch.int16, torch.int32):
        got = sinkhorn._lengths(torch.tensor([3, 100, 1], dtype=dtype), torch.device("cpu"))
        assert got.dtype == torch.int32 and torch.equal(got, torch.tensor([3, 100, 1], dtype=torch.int32))
