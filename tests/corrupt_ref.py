"""numpy restatement of csrc/corrupt.hip, independent of the library: the counter layout and the key tweak of
include/simamba.h, and the seven kinds.

Everything a discrete decision rests on (how many rows go, the cluster count and sizes, the seeds, the removal order,
sigma, the angles, the scale factors) is computed in float32 with one rounding per operation and integer arithmetic, as
the kernel does, and is compared bit for bit.  Everything else (the outliers' coordinates, the normals, the rotation,
the products) is computed in float64 from the same float32 inputs.  A helper module: pytest collects nothing from it."""
import numpy as np

from augment_ref import MASK32, TWO_PI, f32, normal_pair, philox4x32_10, uniform
from dataset_ref import unit_sphere64

DROP_GLOBAL, DROP_LOCAL, ADD_GLOBAL, ADD_LOCAL, ROTATE3, SCALE_AXES, JITTER = 1, 2, 3, 4, 5, 6, 7
RENORM = 1
MAX_CLUSTERS = 8
KEY_TWEAK = 0x434F5252
INT_MIN = -2 ** 31
MAX_POINTS = 8192
# python kind -> (opcode, parameter names in the ABI's order)
KIND = {
    "drop_global": (DROP_GLOBAL, ("ratio",)),
    "drop_local": (DROP_LOCAL, ("total", "max_clusters")),
    "add_global": (ADD_GLOBAL, ("count", "radius")),
    "add_local": (ADD_LOCAL, ("total", "max_clusters", "sigma_low", "sigma_high")),
    "rotate": (ROTATE3, ("theta",)),
    "scale": (SCALE_AXES, ("scale",)),
    "jitter": (JITTER, ("sigma",)),
}


def block(seed, step, cloud, per_point, index):
    """The four words of Philox block ``index`` (an int or an array): augment's counter at chain position 0 under the
    key (seed & 0xffffffff, (seed >> 32) ^ KEY_TWEAK)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    index = np.asarray(index, dtype=np.uint64)
    c3 = ((step >> 32) & 0x0FFFFFFF) | ((1 << 31) if per_point else 0)
    full = lambda v: np.full(index.shape, v, dtype=np.uint64)      # noqa: E731
    return philox4x32_10((full(seed & MASK32), full((seed >> 32) ^ KEY_TWEAK)),
                         (index, full(cloud), full(step & MASK32), full(c3)))


def n_clusters(w0, cmax):
    """C = min(1 + (int)(u * float(Cmax)), Cmax)"""
    return min(1 + int(f32(uniform(w0) * f32(cmax))), cmax)


def cluster_sizes(total, C):
    return [total // C + (1 if j < total % C else 0) for j in range(C)]


def pick(w, a):
    """min((int)(u * float(a)), a - 1)"""
    return min(int(f32(uniform(w) * f32(a))), a - 1)


def normals(seed, step, cloud, count):
    """(count, 3) float64 standard normals of per-point blocks 0 .. count-1."""
    w = block(seed, step, cloud, True, np.arange(count))
    n0, n1 = normal_pair(w[0], w[1])
    n2, _ = normal_pair(w[2], w[3])
    return np.stack([n0, n1, n2], -1).reshape(count, 3)


def dropped_global(n, ratio, seed, step, cloud):
    """(m, keep mask): the m rows with the smallest (w0 of row i's block, i) go."""
    m = min(int(f32(f32(n) * f32(ratio))), n - 1)
    w0 = block(seed, step, cloud, True, np.arange(n))[0]
    order = np.lexsort((np.arange(n), w0))
    keep = np.ones(n, dtype=bool)
    keep[order[:m]] = False
    return m, keep


def dropped_local(pts, total, cmax, seed, step, cloud):
    """(keep mask, sizes, seeds): clusters in order on the rows still alive, nearest (d2, i) to the seed first."""
    p = np.asarray(pts, dtype=f32)
    n = len(p)
    C = n_clusters(block(seed, step, cloud, False, 0)[0], cmax)
    sizes = cluster_sizes(min(total, n - 1), C)
    alive = np.ones(n, dtype=bool)
    seeds = []
    for j, size in enumerate(sizes):
        if size == 0:
            seeds.append(-1)
            continue
        idx = np.nonzero(alive)[0]
        s = idx[pick(block(seed, step, cloud, False, 1 + j)[0], len(idx))]
        seeds.append(int(s))
        d = p[idx] - p[s]                                            # float32, one rounding each
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d2.dtype == f32
        alive[idx[np.lexsort((idx, d2))[:size]]] = False
    return alive, sizes, seeds


def corrupt_cloud(pts, kind, params, seed, step, cloud, K=None, renorm=False):
    """One cloud (n, 3) float32 through ``kind`` (an opcode) with ``params`` (the ABI's order): a dict with
    ``out`` (len, 3) float64, ``src`` (len,) int64, and what the kind drew (``angles`` / ``factors`` / ``sigmas`` /
    ``sizes`` / ``seeds``).  ``K``: the row limit of the output (default: nothing is clamped)."""
    p32 = np.asarray(pts, dtype=f32)
    n = len(p32)
    K = MAX_POINTS if K is None else K
    assert 1 <= n <= K
    p = p32.astype(np.float64)
    par = [f32(v) for v in params] + [f32(0)] * 4
    q0 = block(seed, step, cloud, False, 0)
    res = {}
    if kind == DROP_GLOBAL:
        m, keep = dropped_global(n, par[0], seed, step, cloud)
        out, src = p[keep], np.nonzero(keep)[0]
        res["removed"] = m
    elif kind == DROP_LOCAL:
        keep, sizes, seeds = dropped_local(p32, int(par[0]), int(par[1]), seed, step, cloud)
        out, src = p[keep], np.nonzero(keep)[0]
        res.update(sizes=sizes, seeds=seeds)
    elif kind == ADD_GLOBAL:
        A = min(int(par[0]), K - n)
        w = block(seed, step, cloud, True, np.arange(A))
        u0, u1, u2 = (uniform(w[k]).astype(np.float64) for k in range(3))
        a = 2.0 * u1
        z, s = 1.0 - a, np.sqrt(a * (2.0 - a))
        phi = np.float64(TWO_PI) * u2
        r = np.float64(par[1]) * np.cbrt(u0)
        add = (r[:, None] * np.stack([s * np.cos(phi), s * np.sin(phi), z], -1)).reshape(A, 3)
        out, src = np.concatenate([p, add]), np.concatenate([np.arange(n), np.full(A, -1)])
    elif kind == ADD_LOCAL:
        T = min(int(par[0]), K - n)
        C = n_clusters(q0[0], int(par[1]))
        sizes = cluster_sizes(T, C)
        rng = f32(par[3] - par[2])
        seeds, sigmas = [], []
        for j in range(C):
            w = block(seed, step, cloud, False, 1 + j)
            seeds.append(pick(w[0], n))
            sigmas.append(f32(par[2] + f32(uniform(w[1]) * rng)))
        owner = np.repeat(np.arange(C), sizes)
        z = normals(seed, step, cloud, T)
        add = p[np.array(seeds, dtype=np.int64)[owner]] + np.array(sigmas, dtype=np.float64)[owner][:, None] * z
        out, src = np.concatenate([p, add.reshape(T, 3)]), np.concatenate([np.arange(n), -1 - owner])
        res.update(sizes=sizes, seeds=seeds, sigmas=sigmas)
    elif kind == ROTATE3:
        ang = [f32(f32(f32(f32(2) * uniform(q0[k])) - f32(1)) * par[0]) for k in range(3)]
        c, s = np.cos(np.float64(ang)), np.sin(np.float64(ang))
        Rx = np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]])
        Ry = np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
        Rz = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]])
        out, src = p @ (Rz @ Ry @ Rx).T, np.arange(n)
        res["angles"] = ang
    elif kind == SCALE_AXES:
        inv = f32(f32(1) / par[0])
        rng = f32(par[0] - inv)
        fac = [f32(inv + f32(uniform(q0[k]) * rng)) for k in range(3)]
        out, src = p * np.float64(fac), np.arange(n)
        res["factors"] = fac
    elif kind == JITTER:
        out, src = p + np.float64(par[0]) * normals(seed, step, cloud, n), np.arange(n)
    else:
        raise ValueError(kind)
    res["raw"] = out
    if renorm:
        out, res["renorm_bound"] = unit_sphere64(out)
    res.update(out=out, src=np.asarray(src, dtype=np.int64), len=len(out))
    return res
