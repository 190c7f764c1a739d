"""numpy restatement of csrc/augment.hip, independent of the library: Philox4x32-10, the counter layout of
include/simamba.h, the uniform and Box-Muller maps, and the transform arithmetic.

Everything a discrete decision rests on (theta, s, t, ratio, the keep mask, the flip bits) is computed in float32 with
one rounding per operation, as the kernel does, and is compared bit for bit.  cos / sin / the normals are computed in
float64 from the same float32 inputs; the transforms are applied in float64."""
import numpy as np

ROTATE, SCALE, TRANSLATE, SCALE_TRANSLATE, JITTER, DROPOUT, FLIP = 1, 2, 3, 4, 5, 6, 7
CLOUD_PARAMS = 8
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
f32 = np.float32
TWO_PI = f32(2.0 * np.pi)
# the distribution test of test_gpu_augment.py; test_augment_abi.py confirms the seed under this restatement
DIST_SEED, DIST_B, DIST_N = 20240607, 64, 1024


def philox4x32_10(key, ctr):
    """key (k0, k1), ctr (c0, c1, c2, c3): Python ints or equal-shaped uint32/uint64 arrays -> four uint64 arrays
    holding 32-bit words."""
    k0, k1 = (np.asarray(k, dtype=np.uint64) & np.uint64(MASK32) for k in key)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK32) for c in ctr)
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0          # < 2^64: both factors below 2^32
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + np.uint64(W0)) & m32
        k1 = (k1 + np.uint64(W1)) & m32
    return c0, c1, c2, c3


def block(seed, step, cloud, pos, per_point, index):
    """The four words of Philox block ``index`` (an int or an array) of stream (cloud, step, pos, per-cloud|per-point)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    index = np.asarray(index, dtype=np.uint64)
    c3 = ((step >> 32) & 0x0FFFFFFF) | (pos << 28) | ((1 << 31) if per_point else 0)
    full = lambda v: np.full(index.shape, v, dtype=np.uint64)      # noqa: E731
    return philox4x32_10((full(seed & MASK32), full(seed >> 32)),
                         (index, full(cloud), full(step & MASK32), full(c3)))


def uniform(w):
    """(w >> 8) * 2^-24 as float32: exact."""
    return (np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(f32) * f32(2.0 ** -24)


def normal_pair(wa, wb):
    """Box-Muller in float64 from the float32 inputs the kernel uses."""
    a = ((np.asarray(wa, dtype=np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(a))
    ang = 2.0 * np.pi * uniform(wb).astype(np.float64)
    return r * np.cos(ang), r * np.sin(ang)


def point_normals(seed, step, cloud, pos, n):
    """(n, 3) float64 standard normals of rows 0 .. n-1."""
    w = block(seed, step, cloud, pos, True, np.arange(n))
    n0, n1 = normal_pair(w[0], w[1])
    n2, _ = normal_pair(w[2], w[3])
    return np.stack([n0, n1, n2], -1)


def point_uniforms(seed, step, cloud, pos, n):
    return uniform(block(seed, step, cloud, pos, True, np.arange(n))[0])


def cloud_draw(seed, step, cloud, pos, op, p):
    """The 8 floats simamba_augment_params writes for (cloud, op at pos); cos / sin in float64 of the float32 theta."""
    p = [f32(v) for v in p] + [f32(0)] * 4
    w = block(seed, step, cloud, pos, False, 0)
    u = [uniform(w[k]) for k in range(3)]
    d = np.zeros(CLOUD_PARAMS, dtype=np.float64)
    if op == ROTATE:
        th = f32(u[0] * TWO_PI)
        d[:3] = th, np.cos(np.float64(th)), np.sin(np.float64(th))
    elif op in (SCALE, SCALE_TRANSLATE):
        rng = f32(p[1] - p[0])
        for a in range(3):
            d[a] = f32(p[0] + f32(u[a] * rng))
        if op == SCALE_TRANSLATE:
            w1 = block(seed, step, cloud, pos, False, 1)
            span = f32(f32(2) * p[2])
            for a in range(3):
                d[3 + a] = f32(-p[2] + f32(uniform(w1[a]) * span))
    elif op == TRANSLATE:
        span = f32(f32(2) * p[0])
        for a in range(3):
            d[a] = f32(-p[0] + f32(u[a] * span))
    elif op == JITTER:
        d[:2] = p[0], p[1]
    elif op == DROPOUT:
        d[0] = f32(u[0] * p[0])
    elif op == FLIP:
        up = int(p[0])
        gate = bool(u[0] < f32(0.95))
        d[0] = gate
        for h, a in enumerate(a for a in range(3) if a != up):
            d[1 + a] = gate and bool(u[1 + h] < f32(0.5))
    else:
        raise ValueError(op)
    return d


def cloud_params(seed, step, B, chain):
    """(B, n_ops, 8) float64: cloud_draw for every cloud and op; chain = [(opcode, params), ...]."""
    return np.array([[cloud_draw(seed, step, b, o, op, p) for o, (op, p) in enumerate(chain)] for b in range(B)])


def keep_mask(seed, step, cloud, pos, n, ratio):
    """True where the dropout op at pos keeps row i: not (u_i <= ratio), both float32."""
    return ~(point_uniforms(seed, step, cloud, pos, n) <= f32(ratio))


def apply_chain(pts, chain, draws, noise=None, keep=None):
    """One cloud (n, 3) through the chain in float64, with GIVEN parameters: draws (n_ops, 8) (the kernel's emitted
    float32 values or cloud_draw's), noise (n, 3) for the chain's first jitter, keep (n,) for its first dropout.
    Returns (result (n, 3) float64, the largest magnitude met along the way)."""
    x = np.array(pts, dtype=np.float64)
    big = np.abs(x).max()
    seen_jitter = seen_dropout = False
    for (op, p), d in zip(chain, np.asarray(draws, dtype=np.float64)):
        if op == ROTATE:
            c, s = d[1], d[2]
            x = np.stack([x[:, 0] * c - x[:, 2] * s, x[:, 1], x[:, 0] * s + x[:, 2] * c], -1)
        elif op == SCALE:
            x = x * d[:3]
        elif op == TRANSLATE:
            x = x + d[:3]
        elif op == SCALE_TRANSLATE:
            x = x * d[:3] + d[3:6]
        elif op == JITTER:
            assert not seen_jitter, "noise is emitted for the first jitter only"
            seen_jitter = True
            sd, clip = np.float64(f32(p[0])), np.float64(f32(p[1]))
            x = x + np.clip(sd * np.asarray(noise, dtype=np.float64), -clip, clip)
        elif op == DROPOUT:
            assert not seen_dropout, "the keep mask is emitted for the first dropout only"
            seen_dropout = True
            x = np.where(np.asarray(keep, dtype=bool)[:, None], x, x[0:1])
        elif op == FLIP:
            for a in range(3):
                if d[1 + a]:
                    x[:, a] = x[:, a].max() - x[:, a]
        else:
            raise ValueError(op)
        big = max(big, np.abs(x).max())
    return x, big


def reference_cloud(pts, chain, seed, step, cloud):
    """One cloud through the chain with this module's OWN draws (nothing from the library): float64."""
    n = len(pts)
    draws = np.array([cloud_draw(seed, step, cloud, o, op, p) for o, (op, p) in enumerate(chain)])
    noise = keep = None
    for o, (op, p) in enumerate(chain):
        if op == JITTER and noise is None:
            noise = point_normals(seed, step, cloud, o, n)
        if op == DROPOUT and keep is None:
            keep = keep_mask(seed, step, cloud, o, n, draws[o][0])
    return apply_chain(pts, chain, draws, noise, keep)
