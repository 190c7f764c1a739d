"""CPU: simamba_curve_order (csrc/curve_order.hip) is declared, bound and exported, and refuses every bad argument before
a launch -- no device is touched here."""
import ctypes
import re

import pytest
import torch

import curve_ref as cr
from abi_tables import E_NULLPTR, E_SHAPE, E_VARIANT, OK, P, check_rows, declared_params, header_code
from si_mamba_amd import _lib, spectral

NAN, INF = float("nan"), float("inf")


def ids(*v):
    """A host array of curve ids, as an address the table can pass (kept alive by the module)."""
    arr = (ctypes.c_int * len(v))(*v)
    _KEEP.append(arr)
    return ctypes.addressof(arr)


_KEEP = []
BASE = dict(centers=P, curves=ids(1, 3, 0, 2, 1, 3, 0, 2), order=P, codes=None, B=0, G=128, k=4, bits=10, box=0,
            box_lo=0.0, box_hi=0.0, stream=None)
ROWS = [
    # accepted: B == 0 passes every check and launches nothing; codes may be NULL or not
    (dict(), OK), (dict(codes=P), OK), (dict(G=2), OK), (dict(G=8192), OK), (dict(k=1), OK), (dict(k=8), OK),
    (dict(bits=1), OK), (dict(bits=16), OK), (dict(box=1, box_lo=-1.0, box_hi=1.0), OK),
    (dict(box=0, box_lo=NAN, box_hi=-INF), OK),                                   # the cloud box ignores both
    # shape: G, k, bits, B
    (dict(G=1), E_SHAPE), (dict(G=0), E_SHAPE), (dict(G=8193), E_SHAPE), (dict(G=-1), E_SHAPE),
    (dict(k=0), E_SHAPE), (dict(k=9), E_SHAPE), (dict(bits=0), E_SHAPE), (dict(bits=17), E_SHAPE),
    (dict(bits=-1), E_SHAPE), (dict(B=-1), E_SHAPE),
    # null pointers; B = 5 shows that nothing is launched in front of these answers
    (dict(centers=None), E_NULLPTR), (dict(curves=None), E_NULLPTR), (dict(order=None), E_NULLPTR),
    (dict(B=5, centers=None), E_NULLPTR), (dict(B=5, order=None, codes=P), E_NULLPTR),
    # unknown box mode and curve ids
    (dict(box=2), E_VARIANT), (dict(box=-1), E_VARIANT),
    (dict(curves=ids(0, 1, 2, 4)), E_VARIANT), (dict(curves=ids(-1, 1, 2, 3)), E_VARIANT),
    (dict(curves=ids(0, 1, 2, 3, 9), k=5), E_VARIANT), (dict(curves=ids(0, 1, 2, 3, 9), k=4), OK),
    # the fixed box: lo < hi, both finite
    (dict(box=1, box_lo=1.0, box_hi=1.0), E_SHAPE), (dict(box=1, box_lo=1.0, box_hi=-1.0), E_SHAPE),
    (dict(box=1, box_lo=NAN, box_hi=1.0), E_SHAPE), (dict(box=1, box_lo=-1.0, box_hi=NAN), E_SHAPE),
    (dict(box=1, box_lo=-INF, box_hi=1.0), E_SHAPE), (dict(box=1, box_lo=-1.0, box_hi=INF), E_SHAPE),
    (dict(B=5, box=1, box_lo=0.0, box_hi=0.0), E_SHAPE),
    # two faults: shape, null pointers, box mode, curve ids, fixed box
    (dict(G=1, centers=None), E_SHAPE), (dict(bits=17, box=2), E_SHAPE), (dict(order=None, box=2), E_NULLPTR),
    (dict(curves=None, box=1), E_NULLPTR), (dict(box=2, curves=ids(7, 7, 7, 7)), E_VARIANT),
    (dict(curves=ids(7, 7, 7, 7), box=1, box_lo=1.0, box_hi=0.0), E_VARIANT),
]


def test_curve_order_return_codes_without_a_device():
    check_rows("simamba_curve_order", BASE, ROWS)


def test_symbol_is_declared_bound_and_exported():
    assert "simamba_curve_order" in declared_params()
    assert "simamba_curve_order" in _lib.SIGNATURES
    assert set(declared_params()) == set(_lib.SIGNATURES)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "simamba_curve_order")
    lib = _lib.load()
    assert lib.simamba_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert re.search(r"#define\s+SIMAMBA_ABI_VERSION\s+9\b", header_code())


def test_curve_ids_and_limits_equal_the_header():
    header = {k: int(v) for k, v in re.findall(r"#define\s+SIMAMBA_CURVE_([A-Z_]+)\s+(\d+)", header_code())}
    assert header == dict(Z=0, HILBERT=1, TRANS=2, Z_TRANS=2, HILBERT_TRANS=3, BOX_CLOUD=0, BOX_FIXED=1)
    for k, v in header.items():
        assert getattr(_lib, "CURVE_" + k) == v
    assert spectral.CURVES == {"z": header["Z"], "hilbert": header["HILBERT"], "z-trans": header["Z_TRANS"],
                               "hilbert-trans": header["HILBERT_TRANS"]}
    assert spectral.CURVES == cr.CURVES and spectral.DEFAULT_CURVES == cr.DEFAULT_CURVES
    assert (_lib.CURVE_MAX_G, _lib.CURVE_MAX_K, _lib.CURVE_MAX_BITS) == (8192, 8, 16)


def test_python_route_refuses_the_cpu_and_unknown_names():
    c = torch.zeros(2, 16, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spectral.curve_order(c)
    with pytest.raises(ValueError, match="unknown curves"):
        spectral.curve_ids(("hilbert", "peano"))
    with pytest.raises(ValueError):
        spectral.curve_ids(())
    with pytest.raises(ValueError):
        spectral.curve_ids(("z",) * 9)
    assert list(spectral.curve_ids(("z-trans", "hilbert"))) == [2, 1]
    assert list(spectral.curve_ids(["z", "hilbert"])) == [0, 1]                               # any sequence of names
    with pytest.raises(NotImplementedError):
        spectral.order_tokens("PEANO", (c,), c, None, 4)


def test_models_take_the_method_and_refuse_what_they_refused():
    from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
    from si_mamba_amd.point_mamba import PointMamba, default_config
    small = dict(trans_dim=32, depth=1, num_group=8, group_size=4, encoder_dims=32)
    m = PointMamba(default_config(method="CURVE", **small))
    assert m.n_orders() == 4 and m.seq_len() == 2 * 4 * 8 and m._on_tokens() is True
    dropped = PointMamba(default_config(method="CURVE", drop_out=0.1, **small))              # SAST's conditions
    assert dropped._on_tokens() is False and dropped.eval()._on_tokens() is True
    m3 = PointMamba(default_config(method="CURVE", curves=("z", "hilbert", "z-trans"), reverse=False, **small))
    assert m3.n_orders() == 3 and m3.seq_len() == 3 * 8
    sast = PointMamba(default_config(method="SAST", **small))
    assert list(m.state_dict()) == list(sast.state_dict()) and sast.n_orders() == 4
    with pytest.raises(ValueError, match="add_after_layer"):
        PointMamba(default_config(method="CURVE", add_after_layer=True, **small))
    with pytest.raises(ValueError, match="unknown curves"):
        PointMamba(default_config(method="CURVE", curves=("peano",), **small))
    for name in ("WAVELET", "curve", "HILBERT"):
        with pytest.raises(NotImplementedError):
            PointMamba(default_config(method=name, **small))
    with pytest.raises(NotImplementedError, match="SAST route only"):
        m(torch.zeros(2, 64, 3), gt=torch.zeros(2, dtype=torch.long))
    mae = Point_MAE_Mamba(default_mae_config(ordering="curve", curves=("z", "hilbert"), depth=1, decoder_depth=1,
                                             trans_dim=32, encoder_dims=32, num_group=8, group_size=4))
    assert mae.ordering == "curve" and mae.curves == ("z", "hilbert")
    assert Point_MAE_Mamba(default_mae_config(depth=1, decoder_depth=1, trans_dim=32, encoder_dims=32, num_group=8,
                                              group_size=4)).ordering == "spectral"
    with pytest.raises(NotImplementedError):
        Point_MAE_Mamba(default_mae_config(ordering="wavelet", depth=1, decoder_depth=1, trans_dim=32, encoder_dims=32))
