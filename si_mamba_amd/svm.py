"""Linear one-vs-one C-SVC on the device (csrc/svm.hip): the score the reference validates pre-training with,
``evaluate_svm`` of tools/runner_pretrain.py:66-77 -- scikit-learn's ``SVC(C=0.01, kernel='linear')``, i.e. libsvm --
without the copy of the features to the host.

``OvOLinearSVC`` solves every class pair's dual in float64 with one workgroup per pair; ``evaluate_svm`` pools token
features as the reference does (``mean(1) + max(1)``), fits on the train split and returns the accuracy on the test
split.  Not built: kernels other than linear, probability estimates, class weights, liblinear's one-vs-rest
``LinearSVC``, and more than 16 384 training rows (the solver reads a full Gram matrix; beyond that it would need a row
cache).
"""
from __future__ import annotations

import ctypes
import warnings

import torch

from . import _lib

MAX_CLASSES = 64       # nc
MAX_SAMPLES = 16384    # N: the Gram matrix is N x N float64
MAX_FEATURES = 4096    # d
MAX_PAIR = 4096        # samples of the two largest classes together: a pair's problem lives in LDS
DEFAULT_ITER = (10000, 200)   # the default cap of a pair of n_p samples: 10000 + 200 n_p updates


def _is_index(t):
    return not (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool)


def _check_features(what, X, d=None):
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        raise ValueError(f"{what}: X must be a (N, d) tensor, got {tuple(getattr(X, 'shape', ()))}")
    if X.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{what}: X must be float32 or bfloat16, got {X.dtype}")
    if not 1 <= X.shape[1] <= MAX_FEATURES:
        raise ValueError(f"{what}: d = {X.shape[1]} is outside [1, {MAX_FEATURES}]")
    if d is not None and X.shape[1] != d:
        raise ValueError(f"{what}: X has {X.shape[1]} features, the model was fitted on {d}")
    if X.shape[0] < 1:
        raise ValueError(f"{what}: X has no rows")


def _check_labels(what, y, n):
    if not isinstance(y, torch.Tensor) or tuple(y.shape) != (n,) or not _is_index(y):
        raise ValueError(f"{what}: y must be ({n},) integers, got {tuple(getattr(y, 'shape', ()))} "
                         f"{getattr(y, 'dtype', type(y).__name__)}")


def ovo_vote(dec, num_classes, labels=None):
    """libsvm's vote on decision values (simamba_svm_ovo_vote).  ``dec`` (M, P) float64 in libsvm's pair order,
    P = nc (nc - 1) / 2: ``dec > 0`` votes for the pair's lower class, anything else -- exactly 0 and NaN too -- for the
    higher; the most votes win, the lowest class index on a tie.  Returns ``(pred, matches)``: pred (M,) int32 class
    indices, and with ``labels`` (M,) integer class indices a (1,) int64 device tensor holding the number of rows with
    ``pred == labels`` (None without).  Nothing is read on the host."""
    nc = int(num_classes)
    if not 2 <= nc <= MAX_CLASSES:
        raise ValueError(f"ovo_vote: {nc} classes are outside [2, {MAX_CLASSES}]")
    P = nc * (nc - 1) // 2
    if not isinstance(dec, torch.Tensor) or dec.dim() != 2 or dec.shape[1] != P or dec.shape[0] < 1 \
            or dec.dtype != torch.float64:
        raise ValueError(f"ovo_vote: dec must be (M, {P}) float64 with M >= 1, got "
                         f"{tuple(getattr(dec, 'shape', ()))} {getattr(dec, 'dtype', None)}")
    M = dec.shape[0]
    if labels is not None:
        _check_labels("ovo_vote", labels, M)
    _lib.require_gpu(dec, "ovo_vote")
    if labels is not None:
        _lib.require_gpu(labels, "ovo_vote")
        labels = labels.long().contiguous()
    dec = dec.contiguous()
    pred = torch.empty(M, device=dec.device, dtype=torch.int32)
    matches = None if labels is None else torch.zeros(1, device=dec.device, dtype=torch.int64)
    _lib.count("svm_ovo_vote")
    _lib.call("simamba_svm_ovo_vote", dec, labels, pred, matches, M, nc, device=dec.device, time_as="svm_ovo_vote")
    return pred, matches


class OvOLinearSVC:
    """``sklearn.svm.SVC(C, kernel='linear', tol=tol)`` on the device: libsvm's one-vs-one C-SVC, all solver state in
    float64.

    ``fit(X, y)``: X (N, d) float32 or bfloat16 on the device (bfloat16 is widened; the Gram matrix is
    ``X.double() @ X.double().T``), y (N,) integers -- any values, in any order.  2 <= N <= 16 384, 1 <= d <= 4096,
    2 to 64 classes, and the two largest classes together at most 4096 rows; anything else is a ValueError naming the
    limit.  fit reads the class counts and the convergence flags on the host; it is not meant for graph capture.
    ``predict`` / ``decision_function`` read nothing on the host; ``score`` reads one integer.

    After fit: ``classes_`` (nc,) the sorted labels; ``coef_`` (P, d) and ``intercept_`` (P,) float64 for the
    P = nc (nc - 1) / 2 pairs in libsvm's order (0,1), (0,2), ... (nc-2, nc-1); ``n_iter_`` (P,) int32; ``converged_``
    (P,) uint8.  A pair that reached the iteration cap first raises a RuntimeWarning; its alpha is still feasible.
    ``max_iter``: the cap on a pair's updates; None = 10000 + 200 n_p for a pair of n_p rows (a choice that bounds the
    time, not a measurement; libsvm's own 10^7 would bound nothing).

    ``decision_function`` has libsvm's pair order and sign: positive for the LOWER class of the pair.  For two classes
    this is the negative of what scikit-learn's ``decision_function`` returns (it flips the sign in the binary case);
    for more classes it equals scikit-learn's with ``decision_function_shape='ovo'``."""

    def __init__(self, C=0.01, tol=1e-3, max_iter=None):
        C, tol = float(C), float(tol)
        if not C > 0.0:
            raise ValueError(f"OvOLinearSVC: C must be > 0, got {C}")
        if not tol > 0.0:
            raise ValueError(f"OvOLinearSVC: tol must be > 0, got {tol}")
        if max_iter is not None and (int(max_iter) != max_iter or not 1 <= max_iter < 2 ** 31):
            raise ValueError(f"OvOLinearSVC: max_iter must be None or an integer in [1, 2^31), got {max_iter}")
        self.C, self.tol, self.max_iter = C, tol, None if max_iter is None else int(max_iter)
        self.classes_ = None

    def fit(self, X, y):
        what = "OvOLinearSVC.fit"
        _check_features(what, X)
        N, d = X.shape
        if not 2 <= N <= MAX_SAMPLES:
            raise ValueError(f"{what}: N = {N} is outside [2, {MAX_SAMPLES}] (the solver reads a full N x N Gram "
                             "matrix; more rows would need a row cache, which is not built)")
        _check_labels(what, y, N)
        classes, inv = torch.unique(y.long(), return_inverse=True)
        nc = classes.numel()
        if not 2 <= nc <= MAX_CLASSES:
            raise ValueError(f"{what}: y holds {nc} class{'es' if nc != 1 else ''}, outside [2, {MAX_CLASSES}]")
        counts = torch.bincount(inv, minlength=nc).tolist()          # the host read fit is allowed
        big = sorted(counts)[-2:]
        if sum(big) > MAX_PAIR:
            raise ValueError(f"{what}: the two largest classes have {big[1]} + {big[0]} rows, a pair takes at most "
                             f"{MAX_PAIR}")
        _lib.require_gpu(X, what)
        _lib.require_gpu(y, what)

        dev = X.device
        x32 = X.float().contiguous()
        x64 = x32.double()
        gram = (x64 @ x64.T).contiguous()
        order = torch.argsort(inv, stable=True).to(torch.int32).contiguous()
        starts = [0]
        for c in counts:
            starts.append(starts[-1] + c)
        class_start = (ctypes.c_int * (nc + 1))(*starts)
        P = nc * (nc - 1) // 2
        alpha = torch.empty((nc - 1) * N, device=dev, dtype=torch.float64)
        w = torch.empty(P, d, device=dev, dtype=torch.float64)
        rho = torch.empty(P, device=dev, dtype=torch.float64)
        n_iter = torch.empty(P, device=dev, dtype=torch.int32)
        converged = torch.empty(P, device=dev, dtype=torch.uint8)
        base, per_sample = DEFAULT_ITER if self.max_iter is None else (self.max_iter, 0)
        _lib.count("svm_ovo_fit")
        c_tol = (ctypes.c_double * 2)(self.C, self.tol)               # host arrays both, read during the call
        _lib.call("simamba_svm_ovo_fit", gram, x32, order, class_start, c_tol, alpha, w, rho, n_iter, converged, N, d,
                  nc, base, per_sample, device=dev, time_as="svm_ovo_fit")
        self.classes_, self.coef_, self.intercept_ = classes, w, -rho
        self.n_iter_, self.converged_ = n_iter, converged
        self._alpha, self._order, self._starts = alpha, order.long(), starts
        bad = int((converged == 0).sum().item())
        if bad:
            warnings.warn(f"OvOLinearSVC.fit: {bad} of {P} class pairs reached the iteration cap before "
                          f"m(alpha) - M(alpha) < {self.tol}", RuntimeWarning, stacklevel=2)
        return self

    def _fitted(self, what):
        if self.classes_ is None:
            raise RuntimeError(f"{what}: call fit first")

    def dual_coef_pairs(self):
        """Every pair's solution, for tests: a list of ``(a, b, rows, alpha)`` in pair order -- the class indices, the
        training rows of the pair's problem (class a's, y = +1, then class b's, y = -1; int64) and its alpha
        (float64), views of device tensors."""
        self._fitted("OvOLinearSVC.dual_coef_pairs")
        s, nc = self._starts, len(self._starts) - 1
        out, off = [], 0
        for a in range(nc):
            for b in range(a + 1, nc):
                rows = torch.cat([self._order[s[a]:s[a + 1]], self._order[s[b]:s[b + 1]]])
                out.append((a, b, rows, self._alpha[off:off + rows.numel()]))
                off += rows.numel()
        return out

    def decision_function(self, X):
        """(M, P) float64, ``X.double() @ coef_.T + intercept_``: libsvm's pair order and sign (positive = the pair's
        lower class; for two classes the negative of scikit-learn's)."""
        what = "OvOLinearSVC.decision_function"
        self._fitted(what)
        _check_features(what, X, self.coef_.shape[1])
        _lib.require_gpu(X, what)
        return X.double() @ self.coef_.T + self.intercept_

    def predict(self, X):
        pred, _ = ovo_vote(self.decision_function(X), self.classes_.numel())
        return self.classes_[pred.long()]

    def score(self, X, y):
        """The accuracy on (X, y) as a Python float: one host read of the match counter.  A label that is none of
        ``classes_`` matches nothing."""
        what = "OvOLinearSVC.score"
        self._fitted(what)
        _check_features(what, X, self.coef_.shape[1])
        _check_labels(what, y, X.shape[0])
        _lib.require_gpu(X, what)
        _lib.require_gpu(y, what)
        y = y.long()
        nc = self.classes_.numel()
        pos = torch.searchsorted(self.classes_, y).clamp(max=nc - 1)
        labels = torch.where(self.classes_[pos] == y, pos, torch.full_like(pos, -1))
        _, matches = ovo_vote(self.decision_function(X), nc, labels)
        return matches.item() / float(X.shape[0])


def _pool(what, f):
    if not isinstance(f, torch.Tensor) or f.dim() not in (2, 3):
        raise ValueError(f"{what}: features must be (N, L, d) tokens or (N, d), got {tuple(getattr(f, 'shape', ()))}")
    if f.dim() == 3:
        if f.shape[1] < 1:
            raise ValueError(f"{what}: features have no tokens: {tuple(f.shape)}")
        f = f.mean(1) + f.max(1)[0]
    return f


def evaluate_svm(train_features, train_labels, test_features, test_labels, C=0.01):
    """The reference's ``evaluate_svm`` (tools/runner_pretrain.py:66-77) on the device: (N, L, d) token features are
    pooled ``mean(1) + max(1)`` as there (:73, :75), (N, d) features are taken as they are; a linear one-vs-one SVC
    with ``C`` is fitted on the train split and the accuracy on the test split is returned as a Python float."""
    what = "evaluate_svm"
    tr, te = _pool(what, train_features), _pool(what, test_features)
    _check_features(what, tr)
    _check_features(what, te, tr.shape[1])
    _check_labels(what, test_labels, te.shape[0])
    clf = OvOLinearSVC(C=C).fit(tr, train_labels)
    return clf.score(te, test_labels)
