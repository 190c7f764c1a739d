"""CPU: the whole-cloud Chamfer entry points (csrc/chamfer_large.hip) validate their arguments before touching a
device, in the order shape, empty, null pointers, and the Python route did not grow a host implementation."""
import pytest
import torch

from abi_tables import E_NULLPTR, E_SHAPE, E_VARIANT, OK, P, check_rows

FWD = dict(x=P, y=P, dist=P, idx1=P, idx2=P, d1=P, d2=P, pairs=2, n=100, m=100, stream=None)
BWD = dict(x=P, y=P, ddist=P, idx1=P, idx2=P, dx=P, dy=P, pairs=2, n=100, m=100, stream=None)

ROWS = [
    (dict(n=0), E_SHAPE), (dict(n=8193), E_SHAPE), (dict(m=8193), E_SHAPE), (dict(m=0), E_SHAPE),
    (dict(pairs=-1), E_SHAPE),
    (dict(pairs=0, x=None, y=None, dist=None, idx1=None, idx2=None), OK),
    (dict(x=None), E_NULLPTR), (dict(y=None), E_NULLPTR), (dict(idx2=None), E_NULLPTR),
    # two faults: shape in front of empty, empty in front of null pointers
    (dict(n=0, pairs=0), E_SHAPE), (dict(n=8193, x=None), E_SHAPE), (dict(pairs=0, x=None), OK),
    (dict(pairs=1 << 40, n=8192, m=8192), E_SHAPE),              # more workgroups than a grid holds
]


@pytest.mark.parametrize("name,base", [("simamba_chamfer_large_fwd", FWD), ("simamba_chamfer_large_bwd", BWD)])
def test_return_codes_without_a_device(name, base):
    # dist exists in the forward only
    check_rows(name, base, [({k: v for k, v in change.items() if k in base}, want) for change, want in ROWS])


def test_forward_needs_every_output_and_backward_none():
    check_rows("simamba_chamfer_large_fwd", FWD, [({k: None}, E_NULLPTR) for k in ("dist", "idx1", "d1", "d2")])
    # neither gradient wanted: nothing to launch
    check_rows("simamba_chamfer_large_bwd", BWD, [(dict(ddist=None), E_NULLPTR), (dict(dx=None, dy=None), OK)])


def test_forced_queries_per_thread_is_checked_first():
    fwd = {**FWD, "queries": 0}
    fwd = {k: fwd[k] for k in list(FWD)[:-1] + ["queries", "stream"]}
    bwd = {**BWD, "queries": 0}
    bwd = {k: bwd[k] for k in list(BWD)[:-1] + ["queries", "stream"]}
    rows = [(dict(queries=q), E_VARIANT) for q in (3, 8, -1)] + [(dict(queries=3, n=0), E_VARIANT)]
    for q in (0, 1, 2, 4):
        rows += [(dict(queries=q, n=0), E_SHAPE), (dict(queries=q, pairs=0, x=None), OK),
                 (dict(queries=q, x=None), E_NULLPTR)]
    check_rows("simamba_chamfer_large_fwd_ex", fwd, rows)
    check_rows("simamba_chamfer_large_bwd_ex", bwd, rows)


def test_python_route_refuses_cpu_tensors():
    from si_mamba_amd.mae import chamfer_distance
    a, b = torch.zeros(2, 100, 3), torch.zeros(2, 100, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        chamfer_distance(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        chamfer_distance(a.requires_grad_(), b.requires_grad_())
