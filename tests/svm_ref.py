"""Float64 numpy restatement of the linear one-vs-one C-SVC of csrc/svm.hip (libsvm's C-SVC as scikit-learn's
SVC(kernel='linear') runs it): the SMO solver with the second-order working-set rule, the rho rule, the votes and the
reference's pooling.  Test-only; the GPU tests and the fixture generator compare against it."""
import numpy as np

TAU = 1e-12


def smo(K, y, C, tol, max_iter):
    """libsvm's Solver on one pair.  K (n, n) float64, y (n,) of +-1.  Returns (alpha, G, rho, n_iter, converged).
    Ties go to the lower position (np.argmax), as in the kernel; libsvm itself takes the higher one."""
    n = len(y)
    y = y.astype(np.float64)
    alpha = np.zeros(n)
    G = -np.ones(n)
    QD = np.diag(K).copy()
    it, conv = 0, False
    while it < max_iter:
        pos = y > 0
        up = np.where(pos, alpha < C, alpha > 0)
        low = np.where(pos, alpha > 0, alpha < C)
        v = -y * G
        vu = np.where(up, v, -np.inf)
        i = int(np.argmax(vu))
        gmax = vu[i]
        if not up[i] or not gmax > -np.inf:
            break
        yg = np.where(low, -v, -np.inf)
        gmax2 = yg.max()
        gd = gmax + yg
        quad = QD[i] + QD - 2.0 * K[i]
        quad = np.where(quad > 0, quad, TAU)
        ok = low & (gd > 0)
        gain = np.where(ok, gd * gd / quad, -np.inf)
        j = int(np.argmax(gain))
        if gmax + gmax2 < tol:
            conv = True
            break
        if not ok[j]:
            break
        q = QD[i] + QD[j] - 2.0 * K[i, j]
        q = q if q > 0 else TAU
        ai, aj = alpha[i], alpha[j]
        if y[i] != y[j]:
            delta = (-G[i] - G[j]) / q
            diff = ai - aj
            ai += delta
            aj += delta
            if diff > 0:
                if aj < 0:
                    aj, ai = 0.0, diff
                if ai > C:
                    ai, aj = C, C - diff
            else:
                if ai < 0:
                    ai, aj = 0.0, -diff
                if aj > C:
                    aj, ai = C, C + diff
        else:
            delta = (G[i] - G[j]) / q
            s = ai + aj
            ai -= delta
            aj += delta
            if s > C:
                if ai > C:
                    ai, aj = C, s - C
                if aj > C:
                    aj, ai = C, s - C
            else:
                if aj < 0:
                    aj, ai = 0.0, s
                if ai < 0:
                    ai, aj = 0.0, s
        ai, aj = min(max(ai, 0.0), C), min(max(aj, 0.0), C)
        ci, cj = y[i] * (ai - alpha[i]), y[j] * (aj - alpha[j])
        alpha[i], alpha[j] = ai, aj
        G += y * (ci * K[i] + cj * K[j])
        it += 1
    return alpha, G, rho_of(alpha, G, y, C), it, conv


def rho_of(alpha, G, y, C):
    """libsvm's calculate_rho: the mean of yG over the free alpha; with none free the midpoint of the two bounds."""
    yg = y * G
    upper, lower = alpha >= C, alpha <= 0
    free = ~upper & ~lower
    if free.any():
        return float(yg[free].sum() / free.sum())
    ub_set = (upper & (y < 0)) | (lower & ~upper & (y > 0))
    lb_set = (upper & (y > 0)) | (lower & ~upper & (y < 0))
    ub = yg[ub_set].min() if ub_set.any() else np.inf
    lb = yg[lb_set].max() if lb_set.any() else -np.inf
    return float((ub + lb) / 2.0)


def pairs_of(nc):
    return [(a, b) for a in range(nc) for b in range(a + 1, nc)]


def fit(X, y, C, tol=1e-3, max_iter=None):
    """One-vs-one fit.  Returns dict(classes, coef (P, d), intercept (P,), n_iter, converged, pairs): pairs is a list of
    (a, b, rows, alpha) in libsvm's pair order, rows = class a's samples then class b's, input order inside a class."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y)
    classes = np.unique(y)
    K = X @ X.T
    coef, icpt, iters, convs, pairs = [], [], [], [], []
    for a, b in pairs_of(len(classes)):
        rows = np.concatenate([np.flatnonzero(y == classes[a]), np.flatnonzero(y == classes[b])])
        na = int((y == classes[a]).sum())
        yy = np.where(np.arange(len(rows)) < na, 1.0, -1.0)
        cap = 200 * len(rows) + 10000 if max_iter is None else max_iter
        alpha, _, rho, it, conv = smo(K[np.ix_(rows, rows)], yy, C, tol, cap)
        coef.append((alpha * yy) @ X[rows])
        icpt.append(-rho)
        iters.append(it)
        convs.append(conv)
        pairs.append((a, b, rows, alpha))
    return dict(classes=classes, coef=np.array(coef), intercept=np.array(icpt), n_iter=np.array(iters),
                converged=np.array(convs), pairs=pairs)


def decision_function(model, X):
    """(M, P), libsvm's pair order and sign: positive for the pair's lower class."""
    return np.asarray(X, dtype=np.float64) @ model["coef"].T + model["intercept"]


def vote(dec, nc):
    """libsvm's svm_predict_values: dec > 0 votes a, anything else (0, NaN) votes b; most votes, lowest class on a
    tie.  Returns class indices (M,) int32."""
    dec = np.asarray(dec, dtype=np.float64)
    votes = np.zeros((dec.shape[0], nc), dtype=np.int64)
    for p, (a, b) in enumerate(pairs_of(nc)):
        pos = dec[:, p] > 0
        votes[:, a] += pos
        votes[:, b] += ~pos
    return np.argmax(votes, axis=1).astype(np.int32)


def predict(model, X):
    return model["classes"][vote(decision_function(model, X), len(model["classes"]))]


def pool(features):
    """The reference's pooling of token features (runner_pretrain.py:73, :75): mean(1) + max(1); (N, d) as it is."""
    f = np.asarray(features)
    return f.mean(1) + f.max(1) if f.ndim == 3 else f
