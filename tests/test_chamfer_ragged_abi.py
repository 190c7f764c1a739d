"""CPU: the ragged Chamfer entry points (simamba_chamfer_ragged_fwd / _bwd, csrc/chamfer_large.hip) validate their
arguments before touching a device, in the order variant, shape, empty, null pointers, and the Python routes name what
they refuse."""
import sys

import pytest
import torch

from abi_tables import E_NULLPTR, E_SHAPE, E_VARIANT, OK, P, checked_call

FWD = dict(x=P, y=P, xlen=P, ylen=P, dist=P, idx1=P, idx2=P, d1=P, d2=P, pairs=2, n=100, m=100, norm=2, reduction=0,
           flags=0, queries=0, stream=None)
BWD = dict(x=P, y=P, xlen=P, ylen=P, ddist=P, dd1=P, dd2=P, idx1=P, idx2=P, dx=P, dy=P, pairs=2, n=100, m=100, norm=2,
           reduction=0, flags=0, queries=0, stream=None)
HUGE = dict(pairs=1 << 40, n=8192, m=8192)                       # more workgroups than a grid holds: after the nulls
BOTH = [("simamba_chamfer_ragged_fwd", FWD), ("simamba_chamfer_ragged_bwd", BWD)]


def call(name, base, **change):
    return checked_call(name, base, change)


VARIANTS = [dict(queries=3), dict(queries=8), dict(queries=-1), dict(norm=0), dict(norm=3), dict(norm=-2),
            dict(reduction=-1), dict(reduction=3), dict(flags=2), dict(flags=3), dict(flags=-1)]


@pytest.mark.parametrize("name,base", BOTH)
def test_every_bad_variant_is_refused_first(name, base):
    for v in VARIANTS:
        assert call(name, base, **v) == E_VARIANT, v
        assert call(name, base, n=0, **v) == E_VARIANT, v        # in front of shape
        assert call(name, base, pairs=0, **v) == E_VARIANT, v    # in front of empty
        assert call(name, base, x=None, **v) == E_VARIANT, v     # in front of null pointers


@pytest.mark.parametrize("name,base", BOTH)
def test_every_good_variant_reaches_the_launch_checks(name, base):
    for norm in (1, 2):
        for reduction in (0, 1, 2):
            for flags in (0, 1):
                for queries in (0, 1, 2, 4):
                    mode = dict(norm=norm, reduction=reduction, flags=flags, queries=queries)
                    assert call(name, base, **mode, **HUGE) == E_SHAPE, mode
                    assert call(name, base, **mode, pairs=0, x=None) == OK, mode


@pytest.mark.parametrize("name,base", BOTH)
def test_shape_then_empty_then_null_pointers(name, base):
    for bad in (dict(n=0), dict(n=8193), dict(m=0), dict(m=8193), dict(pairs=-1), dict(n=-5)):
        assert call(name, base, **bad) == E_SHAPE, bad
        if "pairs" not in bad:
            assert call(name, base, pairs=0, **bad) == E_SHAPE, bad  # shape in front of empty
        assert call(name, base, x=None, **bad) == E_SHAPE, bad
    for ok in (dict(n=1, m=1), dict(n=8192, m=8192), dict(n=1, m=8192)):
        assert call(name, base, **ok, **{"pairs": 1 << 40}) == E_SHAPE
        assert call(name, base, x=None, **ok) == E_NULLPTR
    every = {k: None for k, v in base.items() if v == P}
    assert call(name, base, pairs=0, **every) == OK               # empty: nothing read
    assert call(name, base, pairs=0, n=0, **every) == E_SHAPE
    assert call(name, base, **HUGE) == E_SHAPE
    assert call(name, base, x=None, **HUGE) == E_NULLPTR          # the grid limit comes after the pointers


# Per mode, the pointers a call needs; the others may be NULL (probed with a grid that cannot be launched, so that a
# call that passes validation still ends before any device is touched).
def needed_fwd(reduction, flags):
    need = {"x", "y", "idx1", "d1"}
    if reduction != 2:
        need.add("dist")
    if not flags & 1:
        need |= {"idx2", "d2"}
    return need


def needed_bwd(reduction, flags):
    need = {"x", "y", "idx1"}
    need.add("dd1" if reduction == 2 else "ddist")
    if not flags & 1:
        need.add("idx2")
        if reduction == 2:
            need.add("dd2")
    return need


@pytest.mark.parametrize("name,base,needed", [BOTH[0] + (needed_fwd,), BOTH[1] + (needed_bwd,)])
@pytest.mark.parametrize("norm", [1, 2])
def test_required_and_optional_pointers_per_mode(name, base, needed, norm):
    pointers = [k for k, v in base.items() if v == P and k not in ("dx", "dy")]
    for reduction in (0, 1, 2):
        for flags in (0, 1):
            need = needed(reduction, flags)
            mode = dict(norm=norm, reduction=reduction, flags=flags)
            for k in pointers:
                want = E_NULLPTR if k in need else E_SHAPE       # E_SHAPE: validation passed, the grid is refused
                assert call(name, base, **mode, **HUGE, **{k: None}) == want, (mode, k)
            optional = {k: None for k in pointers if k not in need}
            assert call(name, base, **mode, **HUGE, **optional) == E_SHAPE, mode
            assert call(name, base, **mode, **optional, **{k: None for k in need}) == E_NULLPTR


def test_backward_gradient_pointers_are_optional():
    for reduction in (0, 1, 2):
        for flags in (0, 1):
            mode = dict(reduction=reduction, flags=flags)
            # neither gradient wanted: nothing to launch; one of them: validation passes (the grid is refused)
            assert call(*BOTH[1], **mode, dx=None, dy=None) == OK
            assert call(*BOTH[1], **mode, **HUGE, dx=None, dy=None) == OK
            assert call(*BOTH[1], **mode, **HUGE, dx=None) == E_SHAPE
            assert call(*BOTH[1], **mode, **HUGE, dy=None) == E_SHAPE


def test_lengths_are_optional_everywhere():
    for name, base in BOTH:
        assert call(name, base, **HUGE, xlen=None) == E_SHAPE
        assert call(name, base, **HUGE, ylen=None) == E_SHAPE
        assert call(name, base, **HUGE, xlen=None, ylen=None) == E_SHAPE


# ---- Python ----------------------------------------------------------------------------------------------------------
def test_python_argument_errors():
    from si_mamba_amd.mae import chamfer_distance
    a, b = torch.zeros(2, 100, 3), torch.zeros(2, 70, 3)
    for norm in (0, 3, "2", None):
        with pytest.raises(ValueError, match="norm"):
            chamfer_distance(a, b, norm=norm)
    for red in ("min", "none", 0):
        with pytest.raises(ValueError, match="point_reduction"):
            chamfer_distance(a, b, point_reduction=red)
    with pytest.raises(NotImplementedError, match="max"):
        chamfer_distance(a, b, point_reduction="max")
    for key in ("x_lengths", "y_lengths"):
        for bad in (torch.tensor([50.0, 60.0]), torch.tensor([True, False]),
                    torch.tensor([50, 60], dtype=torch.float16)):
            with pytest.raises(TypeError, match=key):
                chamfer_distance(a, b, **{key: bad})
        for bad in (torch.tensor([50]), torch.tensor([50, 60, 70]), torch.tensor([[50, 60]]), torch.tensor(50)):
            with pytest.raises(ValueError, match=key):
                chamfer_distance(a, b, **{key: bad})
    with pytest.raises(ValueError, match="weights"):
        chamfer_distance(a, b, weights=torch.ones(3))
    with pytest.raises(TypeError, match="weights"):
        chamfer_distance(a, b, weights=torch.ones(2, dtype=torch.int64))
    with pytest.raises(TypeError):
        chamfer_distance(a, b, torch.tensor([50, 60]))           # the new arguments are keyword-only


@pytest.mark.parametrize("kw", [dict(x_lengths=torch.tensor([50, 60])), dict(y_lengths=torch.tensor([50, 60])),
                                dict(weights=torch.ones(2)), dict(norm=1), dict(point_reduction="sum"),
                                dict(point_reduction=None), dict(single_directional=True)])
def test_python_route_has_no_host_implementation(kw):
    from si_mamba_amd.mae import chamfer_distance
    a, b = torch.zeros(2, 100, 3), torch.zeros(2, 70, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        chamfer_distance(a, b, **kw)


def test_stand_in_on_cpu_tensors():
    from si_mamba_amd.shim import install_shim
    names = ("mamba_ssm", "causal_conv1d", "pytorch3d")
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in names}
    try:
        install_shim(force=True, pytorch3d=True)
        from pytorch3d.loss import chamfer_distance
        a, b = torch.zeros(2, 100, 3), torch.zeros(2, 70, 3)
        ln = torch.tensor([50, 60])
        for kw in (dict(x_lengths=ln), dict(y_lengths=ln), dict(weights=torch.ones(2)), dict(norm=1),
                   dict(point_reduction="sum"), dict(point_reduction=None, batch_reduction=None),
                   dict(single_directional=True), dict(x_lengths=ln, y_lengths=ln, norm=1, single_directional=True)):
            with pytest.raises(NotImplementedError, match="lengths are taken by the HIP kernels only"):
                chamfer_distance(a, b, **kw)
        for kw in (dict(x_normals=a), dict(y_normals=b), dict(x_normals=a, x_lengths=ln)):
            with pytest.raises(NotImplementedError, match="normals"):
                chamfer_distance(a, b, **kw)
        for batch in ("mean", "sum"):
            with pytest.raises(ValueError, match="point_reduction=None"):
                chamfer_distance(a, b, point_reduction=None, batch_reduction=batch)
        with pytest.raises(ValueError, match="batch_reduction"):
            chamfer_distance(a, b, batch_reduction="max")
        with pytest.raises(RuntimeError, match="no CPU fallback"):   # the plain call is the plain call
            chamfer_distance(a, b)
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] in names]:
            del sys.modules[k]
        sys.modules.update(saved)
