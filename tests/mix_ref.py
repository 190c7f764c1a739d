"""numpy restatement of csrc/mix.hip, independent of the library: the key tweak and counter layout of
include/simamba.h, the partner map, PointCutMix-R / -K and the PointWOLF-style deformation.

Everything a discrete decision rests on (the partner, lambda, m, the ratio, the seeds, which rows go and come, the
anchors, the angles, factors and shifts, the argument of every exponential) is computed in float32 with one rounding per
operation and integer arithmetic, as the kernel does, and is compared bit for bit.  The deformed coordinates are
computed in float64 from the same float32 inputs.  A helper module: pytest collects nothing from it."""
import numpy as np

from augment_ref import MASK32, f32, philox4x32_10, uniform
from dataset_ref import perm

CUT_R, CUT_K = 1, 2
WOLF_RENORM = 1
MAX_ANCHORS = 8
KEY_TWEAK = 0x4D495847
INT_MIN = -2 ** 31
U = 2.0 ** -24
MODE = {"r": CUT_R, "k": CUT_K}
# The largest relative error of the device library's expf on [-80, 0] against float64, doubled: 8.41e-8 (0.84 ulp)
# measured by tools/bench_mix.py on gfx950 (profiles/mix.json, "expf"); no documented bound ships with the toolchain.
EPS_EXP = 2 * 8.41e-8
EXP_ARG_MIN = -80.0
# the state the GPU tests run at: both key words and both step words in use, the low step word wraps within a few calls
SEED = 0xa4093822299f31d0
STEP = (0x0123456 << 32) | 0xfffffffe
# the exact-tie case of test_gpu_mix.py: three 5 x 5 x 5 lattices, cloud b replaced to the share LATTICE_LAM[b];
# test_mix_ref.py confirms that at this state the m-th and (m + 1)-th smallest d2 are equal on both sides of every cloud
LATTICE_LAM = (0.2, 0.5, 0.7)


def lattice(side, step=0.25):
    """side^3 points (float32) on a cubic lattice, multiples of ``step``: every distance repeats many times, exactly."""
    a = np.arange(side, dtype=f32) * f32(step) - f32(step * (side // 2))
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)


def block(seed, step, cloud, per_point, index):
    """The four words of Philox block ``index`` (an int or an array): augment's counter at chain position 0 under the
    key (seed & 0xffffffff, (seed >> 32) ^ KEY_TWEAK)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    index = np.asarray(index, dtype=np.uint64)
    c3 = ((step >> 32) & 0x0FFFFFFF) | ((1 << 31) if per_point else 0)
    full = lambda v: np.full(index.shape, v, dtype=np.uint64)      # noqa: E731
    return philox4x32_10((full(seed & MASK32), full((seed >> 32) ^ KEY_TWEAK)),
                         (index, full(cloud), full(step & MASK32), full(c3)))


def mix_seed(seed):
    """The 64-bit seed whose plain key is the mix key: what simamba_keyed_perm takes."""
    return (int(seed) & (2 ** 64 - 1)) ^ (KEY_TWEAK << 32)


def partner_map(B, seed, step):
    """(B,) int64: perm(n = B, the mix key, stream = step, b)."""
    return perm(B, mix_seed(seed), int(step) & (2 ** 64 - 1), np.arange(B))


def clamp_partner(q, B):
    return min(max(int(q), 0), B - 1)


def lam_of(lam, seed, step, b):
    """lambda of cloud b as float32: the caller's forced into [0, 1] (NaN -> 0), or u(cloud block 0, w0)."""
    if lam is None:
        return f32(uniform(block(seed, step, b, False, 0)[0]))
    l = f32(lam)
    return (l if l < 1 else f32(1)) if l > 0 else f32(0)


def rows_taken(nb, nq, lam):
    """m = min((int)(float(n_b) * lambda), n_b, n_q)"""
    return min(int(f32(f32(nb) * f32(lam))), nb, nq)


def pick(w, a):
    """min((int)(u * float(a)), a - 1)"""
    return min(int(f32(uniform(w) * f32(a))), a - 1)


def d2_f32(p, s):
    """(dx dx + dy dy) + dz dz in float32, one rounding per operation, from the rows p (n, 3) to the row s (3,)."""
    d = np.asarray(p, dtype=f32) - np.asarray(s, dtype=f32)
    out = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert out.dtype == f32
    return out


def smallest(rank, m):
    """The rows of the m smallest (rank as unsigned 32 bits, row), ascending in the row."""
    rank = np.asarray(rank)
    rank = rank.view(np.uint32) if rank.dtype == f32 else rank.astype(np.uint64)
    return np.sort(np.lexsort((np.arange(len(rank)), rank))[:m])


def cutmix_cloud(own, other, mode, lam, seed, step, b):
    """Cloud b (n_b, 3) float32 mixed with its partner's rows (n_q, 3): a dict with ``out`` (n_b, 3) float32 (copies),
    ``src`` (n_b,) int64, ``m``, ``ratio`` float32, ``removed`` / ``taken`` (row arrays) and, in mode K, ``seeds``."""
    own, other = np.asarray(own, dtype=f32), np.asarray(other, dtype=f32)
    nb, nq = len(own), len(other)
    lam = lam_of(lam, seed, step, b)
    m = rows_taken(nb, nq, lam)
    res = dict(m=m, lam=lam, ratio=f32(f32(m) / f32(nb)))
    if mode == CUT_R:
        w = block(seed, step, b, True, np.arange(max(nb, nq)))
        removed, taken = smallest(w[0][:nb], m), smallest(w[1][:nq], m)
    elif mode == CUT_K:
        q1 = block(seed, step, b, False, 1)
        so, sq = pick(q1[0], nb), pick(q1[1], nq)
        res["seeds"] = (so, sq)
        res["d2"] = (d2_f32(own, own[so]), d2_f32(other, other[sq]))
        removed, taken = smallest(res["d2"][0], m), smallest(res["d2"][1], m)
    else:
        raise ValueError(mode)
    keep = np.setdiff1d(np.arange(nb), removed)
    res.update(removed=removed, taken=taken, out=np.concatenate([own[keep], other[taken]]),
               src=np.concatenate([keep, -1 - taken]).astype(np.int64))
    return res


def fps_anchors(p, M, first):
    """M rows by farthest-point sampling in float32 from row ``first``: each the row with the largest minimum d2 to
    the rows so far, ties to the lower row."""
    p = np.asarray(p, dtype=f32)
    rows = [int(first)]
    mind = d2_f32(p, p[first])
    for _ in range(1, M):
        rows.append(int(np.argmax(mind)))                            # the first of the largest
        mind = np.minimum(mind, d2_f32(p, p[rows[-1]]))
    return rows


def wolf_draws(M, params, seed, step, b):
    """(angles (M, 3), factors (M, 3), shifts (M, 3)) float32, and c = fp32(1 / (2 sigma^2))."""
    sigma, rot, scale, trans = (f32(v) for v in params)
    c = f32(1.0 / (2.0 * np.float64(sigma) * np.float64(sigma)))
    ang, fac, sh = (np.zeros((M, 3), dtype=f32) for _ in range(3))
    rng = f32(scale - f32(1))
    for j in range(M):
        wa, ws, wt = (block(seed, step, b, False, base + j) for base in (1, 9, 17))
        for k in range(3):
            ang[j, k] = f32(f32(f32(f32(2) * uniform(wa[k])) - f32(1)) * rot)
            f = f32(f32(1) + f32(uniform(ws[k]) * rng))
            fac[j, k] = f32(f32(1) / f) if int(ws[3]) >> 31 else f
            sh[j, k] = f32(f32(f32(f32(2) * uniform(wt[k])) - f32(1)) * trans)
    return ang, fac, sh, c


def pointwolf_cloud(pts, M, params, seed, step, b):
    """One cloud (n, 3) float32: a dict with ``anchors`` (M rows), ``out`` (n, 3) float64 (before any normalisation),
    ``args`` (n, M) float32 (the exponentials' arguments) and ``bound``, per coordinate, on |kernel - out|.

    The bound, with u = 2^-24, V = max |f (p - a_j)| and Q = max over j of |R v + a_j| and |q_j(p)| per coordinate:
      q_j:   p - a_j and the product with f_j, one rounding each: 2 u V per coordinate, sqrt(3) times that behind a
             rotation; the rotation itself 8e-6 V (three rotations of two products and a sum each on cos / sin good to
             1e-6: test_gpu_corrupt.py's bound); + a_j and + t_j, one rounding each: 2 u Q.
      blend: the arguments of the exponentials are reproduced exactly, so a weight is off by the relative EPS_EXP of
             expf alone; a convex combination whose weights move by a relative e moves by at most 2 e max |q_j|; M
             products, the two sums and the quotient add (M + 2) u:   Q (2 EPS_EXP + (M + 2) u).
    and 1 % on top for the terms of second order."""
    p32 = np.asarray(pts, dtype=f32)
    n = len(p32)
    p = p32.astype(np.float64)
    anchors = fps_anchors(p32, M, pick(block(seed, step, b, False, 0)[0], n))
    ang, fac, sh, c = wolf_draws(M, params, seed, step, b)
    d2 = np.stack([d2_f32(p32, p32[a]) for a in anchors], 1)          # (n, M) float32
    args = -((d2 - d2.min(1, keepdims=True)) * c)
    assert args.dtype == f32
    w = np.exp(args.astype(np.float64))
    num, V, Q = np.zeros((n, 3)), 0.0, 0.0
    for j, a in enumerate(anchors):
        v = (p - p[a]) * fac[j].astype(np.float64)
        cs, sn = np.cos(ang[j].astype(np.float64)), np.sin(ang[j].astype(np.float64))
        Rx = np.array([[1, 0, 0], [0, cs[0], -sn[0]], [0, sn[0], cs[0]]])
        Ry = np.array([[cs[1], 0, sn[1]], [0, 1, 0], [-sn[1], 0, cs[1]]])
        Rz = np.array([[cs[2], -sn[2], 0], [sn[2], cs[2], 0], [0, 0, 1]])
        r = v @ (Rz @ Ry @ Rx).T + p[a]
        q = r + sh[j].astype(np.float64)
        V = max(V, np.abs(v).max())
        Q = max(Q, np.abs(r).max(), np.abs(q).max())
        num += w[:, j:j + 1] * q
    out = num / w.sum(1, keepdims=True)
    bound = 1.01 * (8e-6 * V + 2 * np.sqrt(3) * U * V + 2 * U * Q + Q * (2 * EPS_EXP + (M + 2) * U))
    return dict(anchors=anchors, out=out, args=args, bound=bound, angles=ang, factors=fac, shifts=sh, c=c)
