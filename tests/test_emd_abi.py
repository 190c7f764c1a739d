"""CPU: the earth mover's distance entry point (csrc/emd.hip) validates its arguments before touching a device, the
Python route did not grow a host implementation, the exact assignment solver the GPU tests lean on (assignment_ref.py)
is exact, and the MAE accepts ``loss: emd``."""
import itertools

import numpy as np
import pytest
import torch

import assignment_ref as ar
from abi_tables import E_NULLPTR, E_SHAPE, P, check_rows

FWD = dict(x=P, y=P, assign=P, dist=P, rounds=P, converged=P, pairs=2, n=100, eps=0.0, max_rounds=1000, stream=None)

ROWS = [
    (dict(n=0), E_SHAPE), (dict(n=-1), E_SHAPE), (dict(n=1025), E_SHAPE), (dict(pairs=0), E_SHAPE),
    (dict(pairs=-1), E_SHAPE), (dict(max_rounds=0), E_SHAPE), (dict(max_rounds=-5), E_SHAPE),
    (dict(eps=-1e-3), E_SHAPE), (dict(eps=float("nan")), E_SHAPE), (dict(eps=-float("inf")), E_SHAPE),
    (dict(x=None), E_NULLPTR), (dict(y=None), E_NULLPTR), (dict(assign=None), E_NULLPTR), (dict(dist=None), E_NULLPTR),
    (dict(rounds=None), E_NULLPTR), (dict(converged=None), E_NULLPTR),
    # both instantiations and the limits of n, with a null pointer so that nothing is launched
    (dict(n=1, x=None), E_NULLPTR), (dict(n=64, x=None), E_NULLPTR), (dict(n=65, x=None), E_NULLPTR),
    (dict(n=1024, x=None, eps=1e-4), E_NULLPTR),
    # two faults: the shape in front of the null pointers
    (dict(n=0, x=None), E_SHAPE), (dict(pairs=0, dist=None), E_SHAPE), (dict(eps=-1.0, y=None), E_SHAPE),
    (dict(pairs=1 << 40, n=100), E_SHAPE),                       # more workgroups than a grid holds
    (dict(pairs=1 << 40, n=32), E_SHAPE),
]


def test_return_codes_without_a_device():
    check_rows("simamba_emd_fwd", FWD, ROWS)


def test_python_route_refuses_cpu_tensors():
    from si_mamba_amd import earth_movers_distance
    a, b = torch.zeros(2, 32, 3), torch.zeros(2, 32, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        earth_movers_distance(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        earth_movers_distance(a[0], b[0], return_assignment=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        earth_movers_distance(a.clone().requires_grad_(), b.clone().requires_grad_())


def test_python_route_checks_its_arguments_first():
    from si_mamba_amd import earth_movers_distance
    from si_mamba_amd.emd import default_max_rounds
    z = torch.zeros
    for x, y, kw in [(z(2, 32, 3), z(2, 31, 3), {}), (z(2, 32, 2), z(2, 32, 2), {}), (z(2, 1025, 3), z(2, 1025, 3), {}),
                     (z(0, 32, 3), z(0, 32, 3), {}), (z(2, 0, 3), z(2, 0, 3), {}), (z(32), z(32), {}),
                     (z(2, 32, 3), z(2, 32, 3), dict(eps=-1.0)), (z(2, 32, 3), z(2, 32, 3), dict(eps=float("nan"))),
                     (z(2, 32, 3), z(2, 32, 3), dict(max_rounds=0))]:
        with pytest.raises(ValueError):
            earth_movers_distance(x, y, **kw)
    assert default_max_rounds(32) == 128 * 32 + 4096 and default_max_rounds(1024) == 128 * 1024 + 4096


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_solver_equals_brute_force(n):
    rng = np.random.default_rng(n)
    for trial in range(6):
        if trial % 2:
            cost = rng.integers(0, 4, (n, n)).astype(np.float64) / 64      # many ties
        else:
            cost = rng.random((n, n))
        assign, total = ar.min_cost_assignment(cost)
        assert ar.is_permutation(assign)
        assert total == pytest.approx(cost[np.arange(n), assign].sum(), abs=0)
        want = ar.brute_force(cost)
        assert total == want if trial % 2 else abs(total - want) < 1e-12


def test_solver_on_points_and_matched_cost():
    x, y, opt, cmax = ar.solved("lattice", 2, 6, 5)
    for p in range(2):
        c = ar.cost_matrix(x[p].numpy(), y[p].numpy())
        assert opt[p] == ar.brute_force(c) and cmax[p] == c.max()
        best = min(itertools.permutations(range(6)), key=lambda a: c[np.arange(6), list(a)].sum())
        assert ar.matched_cost(x[p].numpy(), y[p].numpy(), np.array(best)) == opt[p]
    assert not ar.is_permutation(np.array([0, 0, 2])) and ar.is_permutation(np.array([2, 0, 1]))


@pytest.mark.parametrize("n", [7, 64, 200])
def test_solver_equals_scipy(n):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    for kind in ("gaussian", "lattice"):
        x, y = (ar.gaussian_pairs if kind == "gaussian" else ar.lattice_pairs)(1, n, 40 + n)
        c = ar.cost_matrix(x[0].numpy(), y[0].numpy())
        rows, cols = lsa(c)
        want = c[rows, cols].sum()
        got = ar.min_cost_assignment(c)[1]
        assert got == want if kind == "lattice" else abs(got - want) <= 1e-12 * max(1.0, want)


def test_numpy_model_of_the_kernel_reaches_the_lattice_optimum():
    """tools/emd_model.py restates the kernel round for round: on the lattice, with eps below 1 / (64 n), its matching
    costs exactly the optimum, and with one round allowed it still returns a permutation and says so."""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from emd_model import emd_model
    finally:
        sys.path.pop(0)
    n = 33
    x, y, opt, _ = ar.solved("lattice", 2, n, ar.emd_seed(n))
    for p in range(2):
        r = emd_model(x[p].numpy(), y[p].numpy(), ar.lattice_eps(n))
        assert r["converged"] and ar.is_permutation(r["assign"])
        assert ar.matched_cost(x[p].numpy(), y[p].numpy(), r["assign"]) == opt[p]
        r = emd_model(x[p].numpy(), y[p].numpy(), ar.lattice_eps(n), max_rounds=1)
        assert not r["converged"] and r["rounds"] == 1 and ar.is_permutation(r["assign"])


def test_mae_config_accepts_emd_and_refuses_the_unknown():
    from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
    small = dict(trans_dim=64, encoder_dims=64, depth=1, decoder_depth=1, num_group=8, group_size=8, knn_graph=4,
                 k_top_eigenvectors=2)
    assert Point_MAE_Mamba(default_mae_config(loss="emd", **small)).loss == "emd"
    assert Point_MAE_Mamba(default_mae_config(loss="cdl1", **small)).loss == "cdl1"
    assert Point_MAE_Mamba(default_mae_config(**small)).loss == "cdl2"
    with pytest.raises(NotImplementedError, match="sinkhorn"):
        Point_MAE_Mamba(default_mae_config(loss="sinkhorn", **small))
