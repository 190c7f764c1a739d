"""CPU: the t-SNE entry points (csrc/tsne.hip) validate their arguments before touching a device -- shapes in front of
null pointers, then the workspace and its alignment -- and the Python route (si_mamba_amd/manifold) checks its arguments
first and then refuses CPU tensors."""
import ctypes
import inspect

import pytest
import torch

from abi_tables import E_ALIGN, E_NULLPTR, E_SHAPE, E_WORKSPACE, OFF, P, check_rows
from si_mamba_amd import _lib

NAN, INF = float("nan"), float("inf")


def params(alpha=12.0, momentum=0.5, lr=200.0, min_grad_norm=1e-7):
    return (ctypes.c_double * 4)(alpha, momentum, lr, min_grad_norm)


CAL = dict(d2=P, cond=P, beta=P, n=100, perplexity=30.0, stream=None)
CAL_ROWS = [
    (dict(n=1), E_SHAPE), (dict(n=0), E_SHAPE), (dict(n=-4), E_SHAPE), (dict(n=16385), E_SHAPE),
    (dict(perplexity=0.0), E_SHAPE), (dict(perplexity=-1.0), E_SHAPE), (dict(perplexity=NAN), E_SHAPE),
    (dict(perplexity=100.0), E_SHAPE), (dict(perplexity=INF), E_SHAPE), (dict(n=30), E_SHAPE),
    (dict(d2=None), E_NULLPTR), (dict(cond=None), E_NULLPTR), (dict(beta=None), E_NULLPTR),
    # the limits pass the shape checks: a null pointer ends the call
    (dict(n=2, perplexity=1.5, d2=None), E_NULLPTR), (dict(n=16384, perplexity=16383.0, beta=None), E_NULLPTR),
    # two faults: the shape first
    (dict(n=1, d2=None), E_SHAPE), (dict(perplexity=NAN, cond=None), E_SHAPE),
]

GRAD = dict(p=P, y=P, grad=P, kl=P, ws=P, sum_plogp=P, n=100, exaggeration=1.0, stream=None)
GRAD_ROWS = [
    (dict(n=1), E_SHAPE), (dict(n=16385), E_SHAPE), (dict(n=-1), E_SHAPE),
    (dict(exaggeration=0.0), E_SHAPE), (dict(exaggeration=-2.0), E_SHAPE), (dict(exaggeration=NAN), E_SHAPE),
    (dict(exaggeration=INF), E_SHAPE),
    *[({k: None}, E_NULLPTR) for k in ("p", "y", "grad", "kl", "sum_plogp")],
    (dict(ws=None), E_WORKSPACE), (dict(ws=OFF), E_ALIGN),
    (dict(n=2, p=None), E_NULLPTR), (dict(n=16384, exaggeration=12.0, kl=None), E_NULLPTR),
    # two faults: shape, null pointer, workspace, alignment in that order
    (dict(n=1, p=None), E_SHAPE), (dict(exaggeration=NAN, ws=None), E_SHAPE), (dict(y=None, ws=None), E_NULLPTR),
    (dict(grad=None, ws=OFF), E_NULLPTR),
]

RUN = dict(p=P, y=P, update=P, gains=P, status=P, ws=P, sum_plogp=P, params=params(), n=100, first_iter=0, n_iter=250,
           window=250, stream=None)
RUN_ROWS = [
    (dict(n=1), E_SHAPE), (dict(n=16385), E_SHAPE), (dict(first_iter=-1), E_SHAPE), (dict(n_iter=-1), E_SHAPE),
    (dict(window=-1), E_SHAPE), (dict(first_iter=2 ** 31 - 100, n_iter=200), E_SHAPE),
    (dict(params=params(alpha=0.0)), E_SHAPE), (dict(params=params(alpha=NAN)), E_SHAPE),
    (dict(params=params(alpha=INF)), E_SHAPE), (dict(params=params(momentum=-0.1)), E_SHAPE),
    (dict(params=params(momentum=1.0)), E_SHAPE), (dict(params=params(momentum=NAN)), E_SHAPE),
    (dict(params=params(lr=0.0)), E_SHAPE), (dict(params=params(lr=NAN)), E_SHAPE), (dict(params=params(lr=INF)), E_SHAPE),
    (dict(params=params(min_grad_norm=-1.0)), E_SHAPE), (dict(params=params(min_grad_norm=NAN)), E_SHAPE),
    *[({k: None}, E_NULLPTR) for k in ("p", "y", "update", "gains", "status", "sum_plogp", "params")],
    (dict(ws=None), E_WORKSPACE), (dict(ws=OFF), E_ALIGN),
    (dict(n=16384, first_iter=250, n_iter=750, window=300, params=params(1.0, 0.8, 341.0, 0.0), status=None), E_NULLPTR),
    # two faults
    (dict(n=1, p=None), E_SHAPE), (dict(params=params(lr=0.0), y=None), E_SHAPE), (dict(n_iter=-1, params=None), E_SHAPE),
    (dict(update=None, ws=None), E_NULLPTR), (dict(ws=None, n=0), E_SHAPE),
]


def test_calibrate_return_codes_without_a_device():
    check_rows("simamba_tsne_calibrate", CAL, CAL_ROWS)


def test_gradient_return_codes_without_a_device():
    check_rows("simamba_tsne_gradient", GRAD, GRAD_ROWS)


def test_run_return_codes_without_a_device():
    check_rows("simamba_tsne_run", RUN, RUN_ROWS)


def test_workspace_query():
    lib = _lib.load()
    for n in (1, 0, -7, 16385):
        assert lib.simamba_tsne_workspace_floats(n) == E_SHAPE
    # [2 tiles*chunks + tiles] doubles, then 4 * chunks * n floats; a chunk is 64 columns up to n = 2560
    assert lib.simamba_tsne_workspace_floats(2) == 2 * 3 + 4 * 2
    assert lib.simamba_tsne_workspace_floats(65) == 2 * (2 * 2 + 1) + 4 * 2 * 65
    assert lib.simamba_tsne_workspace_floats(2468) == 2 * (2 * 10 * 39 + 10) + 4 * 39 * 2468
    assert lib.simamba_tsne_workspace_floats(16384) == 2 * (2 * 64 * 37 + 64) + 4 * 37 * 16384
    assert all(lib.simamba_tsne_workspace_floats(n) % 2 == 0 for n in range(2, 700))
    assert _lib.ABI_VERSION == 9 and lib.simamba_abi_version() == 9


def test_python_route_checks_its_arguments_first():
    import si_mamba_amd
    from si_mamba_amd import TSNE
    from si_mamba_amd.manifold import tsne
    assert "TSNE" in si_mamba_amd.__all__ and si_mamba_amd.manifold.TSNE is TSNE
    with pytest.raises(ValueError, match="2 dimensions"):
        TSNE(n_components=3)
    with pytest.raises(ValueError, match="euclidean"):
        TSNE(metric="cosine")
    with pytest.raises(ValueError, match="exact gradient.*more accurate"):
        TSNE(method="barnes_hut")
    with pytest.raises(ValueError, match="'exact'"):
        TSNE(method="fft")
    for kw in (dict(init="spectral"), dict(perplexity=0.0), dict(perplexity=NAN), dict(early_exaggeration=0.5),
               dict(early_exaggeration=NAN), dict(learning_rate=0.0), dict(learning_rate="fast"), dict(max_iter=249),
               dict(max_iter=300.5), dict(n_iter_without_progress=-1), dict(min_grad_norm=-1.0),
               dict(min_grad_norm=NAN)):
        with pytest.raises(ValueError):
            TSNE(**kw)
    z = torch.zeros
    for X in (z(12), z(12, 3, 2), z(12, 0), z(12, 4097), z(1, 4), z(12, 4, dtype=torch.float64),
              z(12, 4, dtype=torch.float16)):
        with pytest.raises(ValueError):
            TSNE(perplexity=5).fit(X)
    with pytest.raises(ValueError, match="16384"):
        TSNE().fit(z(16385, 2))
    with pytest.raises(ValueError, match="perplexity"):
        TSNE().fit(z(30, 4))                                      # the default perplexity of 30 needs N > 30
    with pytest.raises(ValueError, match="init"):
        TSNE(perplexity=5, init=z(11, 2)).fit(z(12, 4))
    for d2, perp in ((z(5, 4), 2.0), (z(5, 5, dtype=torch.float64), 2.0), (z(5, 5), 5.0), (z(5, 5), 0.0), (z(1, 1), 0.5)):
        with pytest.raises(ValueError):
            tsne.calibrate(d2, perp)
    with pytest.raises(ValueError):
        tsne.gradient(z(5, 5), z(5, 3))
    with pytest.raises(ValueError):
        tsne.gradient(z(5, 5), z(5, 2), exaggeration=0.0)
    with pytest.raises(ValueError):
        tsne.run(z(5, 5), z(5, 2), z(5, 2), z(4, 2), z(8, dtype=torch.float64), z(1, dtype=torch.float64), 0, 5,
                 exaggeration=1.0, momentum=0.8, learning_rate=50.0)
    with pytest.raises(ValueError):
        tsne.run(z(5, 5), z(5, 2), z(5, 2), z(5, 2), z(8), z(1, dtype=torch.float64), 0, 5,
                 exaggeration=1.0, momentum=0.8, learning_rate=50.0)


def test_python_route_refuses_cpu_tensors():
    from si_mamba_amd import TSNE
    from si_mamba_amd.manifold import tsne
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TSNE(perplexity=5).fit(z(12, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TSNE(perplexity=5, init="random", random_state=0).fit_transform(z(12, 4).bfloat16())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsne.calibrate(z(5, 5), 2.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsne.gradient(z(5, 5), z(5, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsne.run(z(5, 5), z(5, 2), z(5, 2), z(5, 2), z(8, dtype=torch.float64), z(1, dtype=torch.float64), 0, 5,
                 exaggeration=1.0, momentum=0.8, learning_rate=50.0)


def test_return_features_is_keyword_only_and_off():
    from si_mamba_amd.point_mamba import PointMamba
    p = inspect.signature(PointMamba.forward).parameters["return_features"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
