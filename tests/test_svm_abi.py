"""CPU: the two SVM entry points (csrc/svm.hip) validate their arguments before touching a device -- shape errors in
front of null pointers -- and the Python route checks its arguments first and then refuses
CPU tensors."""
import ctypes

import pytest
import torch

from abi_tables import E_NULLPTR, E_SHAPE, P, check_rows

NAN = float("nan")


def starts(*sizes):
    out = [0]
    for s in sizes:
        out.append(out[-1] + s)
    return (ctypes.c_int * len(out))(*out)


def c_tol(c, tol):
    return (ctypes.c_double * 2)(c, tol)


# 3 classes of 4 + 3 + 3 = 10 rows; every row of the tables below has at least one fault, so nothing is launched
FIT = dict(gram=P, x=P, order=P, class_start=starts(4, 3, 3), c_tol=c_tol(0.01, 1e-3), alpha=P, w=P, rho=P, n_iter=P,
           converged=P, n=10, d=8, nc=3, max_iter=100, max_iter_per_sample=0, stream=None)
FIT_REQUIRED = ["gram", "x", "order", "class_start", "c_tol", "alpha", "w", "rho", "n_iter", "converged"]
FIT_ROWS = [
    (dict(nc=1), E_SHAPE), (dict(nc=0), E_SHAPE), (dict(nc=65), E_SHAPE), (dict(nc=-3), E_SHAPE),
    (dict(n=1), E_SHAPE), (dict(n=0), E_SHAPE), (dict(n=16385), E_SHAPE), (dict(n=-1), E_SHAPE),
    (dict(d=0), E_SHAPE), (dict(d=4097), E_SHAPE), (dict(d=-1), E_SHAPE),
    (dict(c_tol=c_tol(0.0, 1e-3)), E_SHAPE), (dict(c_tol=c_tol(-1.0, 1e-3)), E_SHAPE),
    (dict(c_tol=c_tol(NAN, 1e-3)), E_SHAPE), (dict(c_tol=c_tol(0.01, 0.0)), E_SHAPE),
    (dict(c_tol=c_tol(0.01, -1e-3)), E_SHAPE), (dict(c_tol=c_tol(0.01, NAN)), E_SHAPE),
    (dict(max_iter=0), E_SHAPE), (dict(max_iter=-5), E_SHAPE), (dict(max_iter_per_sample=-1), E_SHAPE),
    # the host array: an empty class, ends that are not 0 and n, a pair above 4096 samples
    (dict(class_start=starts(4, 0, 6)), E_SHAPE), (dict(class_start=starts(10, 0, 0)), E_SHAPE),
    (dict(class_start=starts(4, 3, 2)), E_SHAPE), (dict(class_start=starts(4, 3, 4)), E_SHAPE),
    (dict(class_start=(ctypes.c_int * 4)(1, 4, 7, 10)), E_SHAPE),
    (dict(class_start=(ctypes.c_int * 4)(0, 7, 4, 10)), E_SHAPE),
    (dict(n=4100, class_start=starts(2049, 2048, 3)), E_SHAPE),
    (dict(n=8000, class_start=starts(4000, 3900, 100)), E_SHAPE),
    *[({k: None}, E_NULLPTR) for k in FIT_REQUIRED],
    # the limits themselves pass the shape checks: a null pointer ends the call
    (dict(nc=2, n=2, d=1, class_start=starts(1, 1), gram=None), E_NULLPTR),
    (dict(n=4099, class_start=starts(2048, 2048, 3), x=None), E_NULLPTR),
    (dict(n=16384, nc=64, d=4096, class_start=starts(*([256] * 64)), w=None), E_NULLPTR),
    (dict(max_iter=1, max_iter_per_sample=2 ** 31 - 1, rho=None), E_NULLPTR),
    # two faults: the shape in front of the null pointer
    (dict(nc=65, gram=None), E_SHAPE), (dict(n=1, alpha=None), E_SHAPE), (dict(d=0, x=None), E_SHAPE),
    (dict(c_tol=c_tol(NAN, 1e-3), order=None), E_SHAPE), (dict(c_tol=c_tol(0.01, 0.0), converged=None), E_SHAPE),
    (dict(max_iter=0, w=None), E_SHAPE), (dict(max_iter=0, c_tol=None), E_SHAPE),
    (dict(class_start=starts(4, 0, 6), gram=None), E_SHAPE),
    (dict(n=4100, class_start=starts(2049, 2048, 3), n_iter=None), E_SHAPE),
    (dict(nc=1, class_start=None), E_SHAPE),
]

VOTE = dict(dec=P, labels=None, pred=P, matches=None, m=5, nc=3, stream=None)
VOTE_ROWS = [
    (dict(nc=1), E_SHAPE), (dict(nc=65), E_SHAPE), (dict(m=0), E_SHAPE), (dict(m=-1), E_SHAPE),
    (dict(m=1 << 31), E_SHAPE), (dict(dec=None), E_NULLPTR), (dict(pred=None), E_NULLPTR),
    (dict(labels=P), E_NULLPTR),                              # labels without a counter
    (dict(nc=64, m=(1 << 31) - 1, dec=None), E_NULLPTR), (dict(nc=2, m=1, pred=None), E_NULLPTR),
    (dict(nc=65, dec=None), E_SHAPE), (dict(m=0, pred=None), E_SHAPE), (dict(nc=1, labels=P), E_SHAPE),
]


def test_fit_return_codes_without_a_device():
    check_rows("simamba_svm_ovo_fit", FIT, FIT_ROWS)


def test_vote_return_codes_without_a_device():
    check_rows("simamba_svm_ovo_vote", VOTE, VOTE_ROWS)


def _xy(n=12, d=4, nc=3, dtype=torch.float32):
    return torch.zeros(n, d, dtype=dtype), torch.arange(n) % nc


def test_python_route_refuses_cpu_tensors():
    from si_mamba_amd import OvOLinearSVC, evaluate_svm
    from si_mamba_amd.svm import ovo_vote
    X, y = _xy()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OvOLinearSVC().fit(X, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OvOLinearSVC(C=1.0, tol=1e-7, max_iter=5).fit(X.bfloat16(), (y * 7 - 3).int())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate_svm(torch.zeros(12, 5, 4), y, torch.zeros(3, 5, 4), y[:3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate_svm(X, y, X[:3], y[:3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ovo_vote(torch.zeros(4, 3, dtype=torch.float64), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ovo_vote(torch.zeros(4, 3, dtype=torch.float64), 3, torch.zeros(4, dtype=torch.int64))


def test_python_route_checks_its_arguments_first():
    from si_mamba_amd import OvOLinearSVC, evaluate_svm
    from si_mamba_amd.svm import ovo_vote
    z = torch.zeros
    X, y = _xy()
    bad_fit = [
        (z(12), y), (z(12, 4, 2), y), (z(12, 0), y), (z(12, 4097), y), (z(1, 4), y[:1]),
        (z(12, 4, dtype=torch.float64), y), (z(12, 4, dtype=torch.float16), y),
        (X, y[:11]), (X, y.float()), (X, y[:, None]), (X, y == 1),
        (X, z(12, dtype=torch.int64)),                                   # a single class
        (z(130, 2), torch.arange(130)),                                  # 130 classes
        (z(4100, 2), (torch.arange(4100) >= 2049).long()),               # a pair of 4100
    ]
    for Xb, yb in bad_fit:
        with pytest.raises(ValueError):
            OvOLinearSVC().fit(Xb, yb)
    with pytest.raises(ValueError, match="16384"):
        OvOLinearSVC().fit(z(16385, 1), torch.arange(16385) % 2)
    with pytest.raises(ValueError, match="4096"):
        OvOLinearSVC().fit(z(4100, 2), (torch.arange(4100) >= 2049).long())
    with pytest.raises(ValueError, match="64"):
        OvOLinearSVC().fit(z(130, 2), torch.arange(130))
    for kw in (dict(C=0.0), dict(C=-1.0), dict(C=NAN), dict(tol=0.0), dict(tol=NAN), dict(max_iter=0),
               dict(max_iter=2.5), dict(max_iter=2 ** 31)):
        with pytest.raises(ValueError):
            OvOLinearSVC(**kw)
    with pytest.raises(ValueError):
        evaluate_svm(z(12, 5, 4), y, z(3, 5, 6), y[:3])                   # another feature width
    with pytest.raises(ValueError):
        evaluate_svm(z(12, 5, 4), y, z(3, 5, 4), y[:2])
    with pytest.raises(ValueError):
        evaluate_svm(z(12, 5, 4, 2), y, z(3, 5, 4), y[:3])
    with pytest.raises(ValueError):
        evaluate_svm(z(12, 0, 4), y, z(3, 5, 4), y[:3])
    for dec, nc, labels in [(z(4, 3), 3, None), (z(4, 2, dtype=torch.float64), 3, None),
                            (z(0, 3, dtype=torch.float64), 3, None), (z(4, 3, dtype=torch.float64), 1, None),
                            (z(4, 2016, dtype=torch.float64), 65, None),
                            (z(4, 3, dtype=torch.float64), 3, z(3, dtype=torch.int64)),
                            (z(4, 3, dtype=torch.float64), 3, z(4))]:
        with pytest.raises(ValueError):
            ovo_vote(dec, nc, labels)
    with pytest.raises(RuntimeError, match="fit first"):
        OvOLinearSVC().predict(X)
