"""A numpy restatement of exact t-SNE as si_mamba_amd/manifold/tsne.py and csrc/tsne.hip state it (scikit-learn's
``_joint_probabilities``, ``_kl_divergence``, ``_gradient_descent`` and the two-stage schedule of ``TSNE._tsne``), for the
oracle tests and as the yardstick of the GPU tests.  A helper module: pytest collects nothing from it.

Every function takes a ``dtype``: float64 is the reference, and the float32 run of the very same statements measures
what fp32 arithmetic alone costs on the inputs at hand -- the unit the device's tolerances are counted in.
"""
import numpy as np

MACHINE_EPSILON = np.finfo(np.double).eps
N_ITER_CHECK = 50
EXPLORATION_ITER = 250
PERPLEXITY_TOL = 1e-5
FLOAT_MAX = np.finfo(float).max


def blobs(n, d, k, seed):
    """k Gaussian classes around means of scale 4: ``(X (n, d) float32, y (n,))``."""
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((k, d)) * 4
    y = np.arange(n) % k
    X = mu[y] + rng.standard_normal((n, d))
    return X.astype(np.float32), y


def squared_distances(X):
    """(N, N) float32 from a float64 Gram matrix, clamped at 0, zero diagonal: what TSNE.fit hands the kernel."""
    x = np.asarray(X, dtype=np.float64)
    g = x @ x.T
    sq = np.diag(g)
    d2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * g, 0.0)
    np.fill_diagonal(d2, 0.0)
    return d2.astype(np.float32)


def _shifted(d2, dtype):
    """The rows less their smallest off-diagonal entry, and the off-diagonal mask."""
    n = d2.shape[0]
    off = ~np.eye(n, dtype=bool)
    d = np.asarray(d2, dtype=dtype)
    mn = np.where(off, d, np.inf).min(1)
    return d - mn[:, None].astype(dtype), off


def rows_from_beta(d2, beta, dtype=np.float64):
    """``(rows, entropy)`` of p_{j|i} ~ exp(-beta_i d2_ij), j != i, at a given beta: the normalised rows (zero
    diagonal) and H_i = log S + beta T / S."""
    d, off = _shifted(d2, dtype)
    b = np.asarray(beta, dtype=dtype)[:, None]
    p = np.where(off, np.exp(np.where(off, -b * d, dtype(0))), dtype(0))
    S = p.sum(1)
    T = (d * p).sum(1)
    H = np.log(S) + b[:, 0] * T / S
    return (p / S[:, None]).astype(dtype), H.astype(dtype)


def calibrate(d2, perplexity, dtype=np.float64):
    """scikit-learn's ``_binary_search_perplexity`` on dense rows, all rows at once: ``(rows, beta)``.  Start at
    beta = 1, double or halve until bracketed, then bisect; at most 100 steps; stop at |H - log perplexity| <= 1e-5."""
    n = d2.shape[0]
    target = dtype(np.log(np.float32(perplexity).astype(np.float64)))
    beta = np.ones(n, dtype=dtype)
    lo = np.full(n, -np.inf, dtype=dtype)
    hi = np.full(n, np.inf, dtype=dtype)
    live = np.ones(n, dtype=bool)
    for _ in range(100):
        _, H = rows_from_beta(d2, beta, dtype)
        diff = H - target
        live &= ~(np.abs(diff) <= PERPLEXITY_TOL)
        if not live.any():
            break
        up = live & (diff > 0)
        down = live & ~(diff > 0)
        lo[up] = beta[up]
        beta[up] = np.where(np.isinf(hi[up]), beta[up] * 2, (beta[up] + hi[up]) / 2)
        hi[down] = beta[down]
        beta[down] = np.where(np.isinf(lo[down]), beta[down] / 2, (beta[down] + lo[down]) / 2)
    rows, _ = rows_from_beta(d2, beta, dtype)
    return rows, beta


def joint(cond, dtype=np.float64):
    """P = max((C + C') / (2 N), eps) with zero diagonal."""
    c = np.asarray(cond, dtype=dtype)
    n = c.shape[0]
    P = np.maximum((c + c.T) / dtype(2 * n), dtype(MACHINE_EPSILON))
    np.fill_diagonal(P, 0)
    return P


def sum_plogp(P):
    p = np.asarray(P, dtype=np.float64)
    return float(np.sum(np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)))


def grad_kl(P, Y, alpha=1.0, dtype=np.float64):
    """scikit-learn's ``_kl_divergence`` with P exaggerated by alpha, dense: ``(kl, grad (N, 2))``.
    w = 1 / (1 + |yi - yj|^2), Q = max(w / sum w, eps), grad_i = 4 sum_j (alpha P - Q) w (yi - yj),
    kl = sum_{i != j} alpha P log(max(alpha P, eps) / Q)."""
    P = np.asarray(P, dtype=dtype) * dtype(alpha)
    Y = np.asarray(Y, dtype=dtype)
    n = Y.shape[0]
    off = ~np.eye(n, dtype=bool)
    dx = Y[:, None, 0] - Y[None, :, 0]
    dy = Y[:, None, 1] - Y[None, :, 1]
    w = np.where(off, 1 / (1 + (dx * dx + dy * dy)), dtype(0))
    Q = np.maximum(w / w.sum(), dtype(MACHINE_EPSILON))
    kl = np.sum(np.where(off, P * np.log(np.maximum(P, dtype(MACHINE_EPSILON)) / Q), dtype(0)))
    pq = np.where(off, (P - Q) * w, dtype(0))
    grad = 4 * np.stack([(pq * dx).sum(1), (pq * dy).sum(1)], 1)
    return dtype(kl), grad.astype(dtype)


def step(Y, update, gains, grad, momentum, lr, dtype=np.float64):
    """One update of scikit-learn's ``_gradient_descent``: ``(Y, update, gains, gains * grad)``."""
    inc = update * grad < 0
    gains = np.where(inc, gains + dtype(0.2), gains * dtype(0.8))
    gains = np.maximum(gains, dtype(0.01))
    gg = grad * gains
    update = dtype(momentum) * update - dtype(lr) * gg
    return (Y + update).astype(dtype), update.astype(dtype), gains.astype(dtype), gg


def gradient_descent(P, Y, it, max_iter, alpha, momentum, lr, window, min_grad_norm=1e-7, dtype=np.float64,
                     update=None, gains=None, keep=()):
    """scikit-learn's ``_gradient_descent`` from iteration ``it`` with n_iter_check = 50.  Returns a dict: Y, update,
    gains, error (the last computed, of alpha P), done (iterations done in all), stopped, and ``kept``: Y after each
    iteration count listed in ``keep``."""
    Y = np.asarray(Y, dtype=dtype).copy()
    update = np.zeros_like(Y) if update is None else np.asarray(update, dtype=dtype).copy()
    gains = np.ones_like(Y) if gains is None else np.asarray(gains, dtype=dtype).copy()
    error, best, best_iter, done, stopped, kept = FLOAT_MAX, FLOAT_MAX, it, it, False, {}
    for i in range(it, max_iter):
        check = (i + 1) % N_ITER_CHECK == 0
        kl, grad = grad_kl(P, Y, alpha, dtype)
        if check or i == max_iter - 1:
            error = float(kl)
        Y, update, gains, gg = step(Y, update, gains, grad, momentum, lr, dtype)
        done = i + 1
        if done in keep:
            kept[done] = Y.copy()
        if check:
            if error < best:
                best, best_iter = error, i
            elif i - best_iter > window:
                stopped = True
            if np.sqrt(np.sum(np.asarray(gg, dtype=np.float64) ** 2)) <= min_grad_norm:
                stopped = True
            if stopped:
                break
    return dict(Y=Y, update=update, gains=gains, error=error, done=done, stopped=stopped, kept=kept)


def fit(P, Y0, max_iter=1000, lr=None, early_exaggeration=12.0, n_iter_without_progress=300, min_grad_norm=1e-7,
        dtype=np.float64, keep=()):
    """The two stages of ``TSNE._tsne`` as si_mamba_amd.manifold.TSNE runs them: 250 iterations of alpha P with
    momentum 0.5, the rest of P with momentum 0.8, update and gains fresh in each.  A stop in the first stage ends the
    fit.  Returns Y, kl (of P at Y), n_iter (iterations done) and ``kept``."""
    n = P.shape[0]
    lr = max(n / early_exaggeration / 4.0, 50.0) if lr is None else lr
    a = gradient_descent(P, Y0, 0, min(EXPLORATION_ITER, max_iter), early_exaggeration, 0.5, lr, EXPLORATION_ITER,
                         min_grad_norm, dtype, keep=keep)
    kept = dict(a["kept"])
    if not a["stopped"] and max_iter > EXPLORATION_ITER:
        a = gradient_descent(P, a["Y"], EXPLORATION_ITER, max_iter, 1.0, 0.8, lr, n_iter_without_progress,
                             min_grad_norm, dtype, keep=keep)
        kept.update(a["kept"])
    return dict(Y=a["Y"], kl=float(grad_kl(P, a["Y"], 1.0, np.float64)[0]), n_iter=a["done"], kept=kept)


def pca_init(X):
    """``init='pca'`` as manifold.tsne.pca_init states it, in float64: (N, 2)."""
    x = np.asarray(X, dtype=np.float64)
    xc = x - x.mean(0, keepdims=True)
    _, vecs = np.linalg.eigh(xc.T @ xc)
    v = vecs[:, [-1, -2]]
    lead = v[np.abs(v).argmax(0), [0, 1]]
    v = v * np.where(lead < 0, -1.0, 1.0)
    y = xc @ v
    return y / y[:, 0].std() * 1e-4


def knn1_accuracy(Y, labels):
    """The share of points whose nearest other point in the embedding carries their label."""
    Y = np.asarray(Y, dtype=np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    return float(np.mean(np.asarray(labels)[d.argmin(1)] == np.asarray(labels)))


def deviation(a32, a64):
    """max |float32 run - float64 run|: the yardstick of the device's tolerances."""
    return float(np.abs(np.asarray(a32, dtype=np.float64) - np.asarray(a64, dtype=np.float64)).max())


def bound(a32, a64, factor=8.0, floor=1e-6):
    """The device's allowance: ``factor`` times the float32 run's deviation (summation order, v_rcp_f32 and exp2 in
    place of correctly rounded operations), at least ``floor`` of the largest magnitude."""
    return max(factor * deviation(a32, a64), floor * float(np.abs(np.asarray(a64, dtype=np.float64)).max()))
