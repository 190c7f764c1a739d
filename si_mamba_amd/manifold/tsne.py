"""Exact t-SNE in two dimensions on the device (csrc/tsne.hip): the map the reference draws of the classifier's pooled
features, ``TSNE(n_components=2, init='pca', random_state=0).fit_transform(test_feature)`` of
tools/runner_finetune.py:605-612, without the copy of the features to the host and without scikit-learn.

``calibrate`` / ``joint_probabilities`` / ``gradient`` / ``run`` are the stages, one C-ABI call each; ``TSNE`` strings
them together with scikit-learn's schedule: 250 iterations with the joint probabilities exaggerated and momentum 0.5,
the rest with momentum 0.8, ``update`` and ``gains`` reset in between, the error looked at every 50 iterations.  All
``max_iter`` iterations are enqueued by two calls; the stop rule lives in a status record on the device, and the kernels
behind a stop return at once.

What differs from scikit-learn, on purpose: the gradient is the exact one for every N (scikit-learn's default,
Barnes-Hut, approximates it); the joint probabilities are normalised by 2 N, the sum of the conditional rows, not by
their measured sum; a stop inside the exaggerated stage (only ``min_grad_norm`` can cause one: that stage's no-progress
window is its whole length) ends the fit, where scikit-learn goes on to the second stage; ``n_iter_`` counts the
iterations done, scikit-learn reports the index of the last one.  Not built: a sparse k-NN P, Barnes-Hut,
``n_components`` other than 2, metrics other than Euclidean, more than 16 384 rows, plotting.
"""
from __future__ import annotations

import ctypes
import math
import sys

import torch

from .. import _lib

MAX_SAMPLES = 16384         # P is dense, N x N fp32
MAX_FEATURES = 4096
MACHINE_EPSILON = 2.220446049250313e-16     # scikit-learn's floor of the joint probabilities
EXPLORATION_ITER = 250      # scikit-learn's _EXPLORATION_MAX_ITER: the exaggerated stage, and its no-progress window
N_ITER_CHECK = 50           # fixed in the kernels' host loop
STATUS_FLOATS = 8
ST_KL, ST_GRAD_NORM, ST_BEST_ERROR, ST_BEST_ITER, ST_ITERS, ST_STOPPED = range(6)


def _check_n(what, n):
    if not 2 <= n <= MAX_SAMPLES:
        raise ValueError(f"{what}: N = {n} is outside [2, {MAX_SAMPLES}] (P is a dense N x N matrix; more rows would "
                         "need the sparse k-NN form, which is not built)")


def _check_square(what, name, t, n=None):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] != t.shape[1] or t.dtype != torch.float32 \
            or (n is not None and t.shape[0] != n):
        raise ValueError(f"{what}: {name} must be a square float32 matrix, got {tuple(getattr(t, 'shape', ()))} "
                         f"{getattr(t, 'dtype', type(t).__name__)}")


def _check_points(what, name, t, n):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != (n, 2) or t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be ({n}, 2) float32, got {tuple(getattr(t, 'shape', ()))} "
                         f"{getattr(t, 'dtype', type(t).__name__)}")


def workspace(n, device):
    """The workspace ``gradient`` and ``run`` take for n points."""
    return torch.empty(_lib.load().simamba_tsne_workspace_floats(n), device=device, dtype=torch.float32)


def calibrate(d2, perplexity):
    """``(cond, beta)``: the conditional rows p_{j|i} (N, N) float32 with zero diagonal and beta_i (N,) float64, from
    squared distances ``d2`` (N, N) float32: every row's entropy is log(perplexity) to 1e-5 (scikit-learn's search)."""
    what = "tsne.calibrate"
    _check_square(what, "d2", d2)
    n = d2.shape[0]
    _check_n(what, n)
    perplexity = float(perplexity)
    if not 0.0 < perplexity < n:
        raise ValueError(f"{what}: perplexity must be in (0, N = {n}), got {perplexity}")
    _lib.require_gpu(d2, what)
    d2 = d2.contiguous()
    cond = torch.empty(n, n, device=d2.device, dtype=torch.float32)
    beta = torch.empty(n, device=d2.device, dtype=torch.float64)
    _lib.count("tsne_calibrate")
    _lib.call("simamba_tsne_calibrate", d2, cond, beta, n, perplexity, device=d2.device, time_as="tsne_calibrate")
    return cond, beta


def joint_probabilities(cond):
    """``(P, sum_plogp)``: P = max((C + C') / (2 N), 2.2e-16) with zero diagonal, (N, N) float32 and exactly symmetric;
    the constant sum_ij p log p as a (1,) float64 device tensor."""
    n = cond.shape[0]
    P = cond + cond.T
    P.mul_(1.0 / (2.0 * n)).clamp_(min=MACHINE_EPSILON)
    P.fill_diagonal_(0.0)
    Pd = P.double()
    return P, torch.xlogy(Pd, Pd).sum().reshape(1)


def gradient(P, Y, exaggeration=1.0, sum_plogp=None, ws=None):
    """``(grad, kl)`` at Y: grad (N, 2) float32 = 4 sum_j (exaggeration p_ij - q_ij) w_ij (y_i - y_j), kl (1,) float64
    the KL divergence of P itself from Q.  P (N, N) float32 symmetric with zero diagonal."""
    what = "tsne.gradient"
    _check_square(what, "P", P)
    n = P.shape[0]
    _check_n(what, n)
    _check_points(what, "Y", Y, n)
    exaggeration = float(exaggeration)
    if not (0.0 < exaggeration < math.inf):
        raise ValueError(f"{what}: exaggeration must be positive and finite, got {exaggeration}")
    _lib.require_gpu(P, what)
    _lib.require_gpu(Y, what)
    P, Y = P.contiguous(), Y.contiguous()
    if sum_plogp is None:
        Pd = P.double()
        sum_plogp = torch.xlogy(Pd, Pd).sum().reshape(1)
    ws = workspace(n, P.device) if ws is None else ws
    grad = torch.empty(n, 2, device=P.device, dtype=torch.float32)
    kl = torch.empty(1, device=P.device, dtype=torch.float64)
    _lib.count("tsne_gradient")
    _lib.call("simamba_tsne_gradient", P, Y, grad, kl, ws, sum_plogp, n, exaggeration, device=P.device,
              time_as="tsne_gradient")
    return grad, kl


def new_status(device, first_iter=0):
    """A status record for ``run``: nothing computed yet, best error DBL_MAX at ``first_iter``, not stopped."""
    st = torch.empty(STATUS_FLOATS, device=device, dtype=torch.float64)
    st.copy_(torch.tensor([0.0, 0.0, sys.float_info.max, float(first_iter), float(first_iter), 0.0, 0.0, 0.0],
                          dtype=torch.float64))
    return st


def run(P, Y, update, gains, status, sum_plogp, first_iter, n_iter, *, exaggeration, momentum, learning_rate,
        min_grad_norm=1e-7, n_iter_without_progress=300, ws=None):
    """Iterations ``first_iter .. first_iter + n_iter - 1`` of scikit-learn's ``_gradient_descent`` in place on
    ``Y``, ``update``, ``gains`` (N, 2) float32 and ``status`` (8,) float64 (include/simamba.h lists its fields): one
    call enqueues them all and reads nothing back."""
    what = "tsne.run"
    _check_square(what, "P", P)
    n = P.shape[0]
    _check_n(what, n)
    for name, t in (("Y", Y), ("update", update), ("gains", gains)):
        _check_points(what, name, t, n)
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} is updated in place and must be contiguous")
    if not isinstance(status, torch.Tensor) or tuple(status.shape) != (STATUS_FLOATS,) \
            or status.dtype != torch.float64:
        raise ValueError(f"{what}: status must be ({STATUS_FLOATS},) float64")
    for t in (P, Y, update, gains, status, sum_plogp):
        _lib.require_gpu(t, what)
    P = P.contiguous()
    ws = workspace(n, P.device) if ws is None else ws
    params = (ctypes.c_double * 4)(exaggeration, momentum, learning_rate, min_grad_norm)   # a host array
    _lib.count("tsne_run")
    _lib.call("simamba_tsne_run", P, Y, update, gains, status, ws, sum_plogp, params, n, int(first_iter), int(n_iter),
              int(n_iter_without_progress), device=P.device, time_as="tsne_run")


def squared_distances(X):
    """(N, N) float32 squared Euclidean distances from a float64 Gram matrix, clamped at 0, zero diagonal."""
    x64 = X.double()
    gram = x64 @ x64.T
    sq = gram.diagonal()
    d2 = (sq[:, None] + sq[None, :] - 2.0 * gram).clamp_(min=0.0)
    d2.fill_diagonal_(0.0)
    return d2.float()


def pca_init(X):
    """scikit-learn's ``init='pca'``: the top two principal components of centred X (``torch.linalg.eigh`` of the
    float64 covariance), each signed so that its largest-magnitude loading is positive (the first such on a tie),
    scaled to ``std(Y[:, 0]) = 1e-4``.  (N, 2) float32."""
    x64 = X.double()
    xc = x64 - x64.mean(0, keepdim=True)
    _, vecs = torch.linalg.eigh(xc.T @ xc)                 # ascending eigenvalues
    v = vecs[:, [-1, -2]]
    lead = v.gather(0, v.abs().argmax(0, keepdim=True))
    v = v * torch.where(lead < 0, -1.0, 1.0)
    y = xc @ v
    y = y / y[:, 0].std(unbiased=False).clamp_min(sys.float_info.min) * 1e-4
    return y.float()


class TSNE:
    """``sklearn.manifold.TSNE(n_components=2, method='exact')`` on the device, with scikit-learn's schedule and stop
    rule (this module's docstring lists what differs).

    ``fit(X)`` / ``fit_transform(X)``: X (N, d) float32 or bfloat16 on the device, 2 <= N <= 16 384, d <= 4096,
    perplexity < N.  After fitting: ``embedding_`` (N, 2) float32 on the device, ``kl_divergence_`` (the KL divergence
    at ``embedding_``, a Python float), ``n_iter_`` (iterations done) and ``learning_rate_``.  ``init``: 'pca',
    'random' (1e-4 N(0, 1) from a ``torch.Generator`` seeded by ``random_state``) or an (N, 2) tensor.

    fit reads the status record and the final KL on the host once, at the end; like ``OvOLinearSVC.fit`` it is not
    meant for graph capture.  Two fits of the same input give the same bits."""

    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7, metric="euclidean", init="pca", method="exact",
                 random_state=None):
        what = "TSNE"
        if n_components != 2:
            raise ValueError(f"{what}: n_components = {n_components!r}; the kernels embed in 2 dimensions only")
        if metric != "euclidean":
            raise ValueError(f"{what}: metric = {metric!r}; only 'euclidean' is built")
        if method == "barnes_hut":
            raise ValueError(f"{what}: method = 'barnes_hut' is not built: the exact gradient is what runs here, for "
                             "every N up to 16384, and it is the more accurate of the two (Barnes-Hut approximates "
                             "it); pass method='exact'")
        if method != "exact":
            raise ValueError(f"{what}: method = {method!r}; only 'exact' is built")
        if not (isinstance(init, torch.Tensor) or init in ("pca", "random")):
            raise ValueError(f"{what}: init must be 'pca', 'random' or an (N, 2) tensor, got {init!r}")
        if not float(perplexity) > 0.0:
            raise ValueError(f"{what}: perplexity must be > 0, got {perplexity}")
        if not float(early_exaggeration) >= 1.0 or not float(early_exaggeration) < math.inf:
            raise ValueError(f"{what}: early_exaggeration must be finite and >= 1, got {early_exaggeration}")
        if learning_rate != "auto" and not (isinstance(learning_rate, (int, float)) and 0.0 < learning_rate < math.inf):
            raise ValueError(f"{what}: learning_rate must be 'auto' or a positive number, got {learning_rate!r}")
        if int(max_iter) != max_iter or not EXPLORATION_ITER <= max_iter < 2 ** 30:
            raise ValueError(f"{what}: max_iter must be an integer of at least {EXPLORATION_ITER} (the exaggerated "
                             f"stage), got {max_iter}")
        if int(n_iter_without_progress) != n_iter_without_progress or not 0 <= n_iter_without_progress < 2 ** 30:
            raise ValueError(f"{what}: n_iter_without_progress must be a non-negative integer")
        if not float(min_grad_norm) >= 0.0:
            raise ValueError(f"{what}: min_grad_norm must be >= 0, got {min_grad_norm}")
        self.n_components, self.perplexity, self.early_exaggeration = 2, float(perplexity), float(early_exaggeration)
        self.learning_rate, self.max_iter = learning_rate, int(max_iter)
        self.n_iter_without_progress, self.min_grad_norm = int(n_iter_without_progress), float(min_grad_norm)
        self.metric, self.init, self.method, self.random_state = metric, init, method, random_state
        self.embedding_ = None

    def _initial(self, X):
        n = X.shape[0]
        if isinstance(self.init, torch.Tensor):
            if tuple(self.init.shape) != (n, 2):
                raise ValueError(f"TSNE.fit: init must be ({n}, 2), got {tuple(self.init.shape)}")
            return self.init.to(device=X.device, dtype=torch.float32)
        if self.init == "pca":
            if X.shape[1] < 2:
                raise ValueError("TSNE.fit: init='pca' needs at least 2 features")
            return pca_init(X)
        g = torch.Generator()
        if self.random_state is None:
            g.seed()
        else:
            g.manual_seed(int(self.random_state))
        return (1e-4 * torch.randn(n, 2, generator=g, dtype=torch.float32)).to(X.device)

    def fit(self, X):
        what = "TSNE.fit"
        if not isinstance(X, torch.Tensor) or X.dim() != 2:
            raise ValueError(f"{what}: X must be a (N, d) tensor, got {tuple(getattr(X, 'shape', ()))}")
        if X.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"{what}: X must be float32 or bfloat16, got {X.dtype}")
        n, d = X.shape
        if not 1 <= d <= MAX_FEATURES:
            raise ValueError(f"{what}: d = {d} is outside [1, {MAX_FEATURES}]")
        _check_n(what, n)
        if not self.perplexity < n:
            raise ValueError(f"{what}: perplexity = {self.perplexity} must be less than N = {n}")
        if isinstance(self.init, torch.Tensor) and tuple(self.init.shape) != (n, 2):
            raise ValueError(f"{what}: init must be ({n}, 2), got {tuple(self.init.shape)}")
        _lib.require_gpu(X, what)
        dev = X.device
        X = X.float()
        cond, _ = calibrate(squared_distances(X), self.perplexity)
        P, sum_plogp = joint_probabilities(cond)
        del cond
        Y = torch.empty(n, 2, device=dev, dtype=torch.float32)
        Y.copy_(self._initial(X))
        lr = max(n / self.early_exaggeration / 4.0, 50.0) if self.learning_rate == "auto" else float(self.learning_rate)
        update = torch.empty(n, 2, device=dev, dtype=torch.float32).zero_()
        gains = torch.empty(n, 2, device=dev, dtype=torch.float32).fill_(1.0)
        status = new_status(dev, 0)
        ws = workspace(n, dev)
        common = dict(learning_rate=lr, min_grad_norm=self.min_grad_norm, ws=ws)
        run(P, Y, update, gains, status, sum_plogp, 0, EXPLORATION_ITER, exaggeration=self.early_exaggeration,
            momentum=0.5, n_iter_without_progress=EXPLORATION_ITER, **common)
        if self.max_iter > EXPLORATION_ITER:
            # scikit-learn calls _gradient_descent a second time: update, gains and the best error start afresh
            update.zero_()
            gains.fill_(1.0)
            status[ST_BEST_ERROR:ST_BEST_ITER + 1] = torch.tensor([sys.float_info.max, float(EXPLORATION_ITER)],
                                                                  dtype=torch.float64)
            run(P, Y, update, gains, status, sum_plogp, EXPLORATION_ITER, self.max_iter - EXPLORATION_ITER,
                exaggeration=1.0, momentum=0.8, n_iter_without_progress=self.n_iter_without_progress, **common)
        _, kl = gradient(P, Y, 1.0, sum_plogp, ws)
        st = status.tolist()                                             # the host read fit is allowed
        self.embedding_, self.learning_rate_ = Y, lr
        self.kl_divergence_ = float(kl.item())
        self.n_iter_ = int(st[ST_ITERS])
        self.status_ = st
        return self

    def fit_transform(self, X):
        return self.fit(X).embedding_
