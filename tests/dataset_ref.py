"""numpy restatement of csrc/keyed_perm.h and of the index arithmetic of csrc/dataset.hip, independent of the library:
the keyed bijection (a four-round balanced Feistel network over Philox4x32-10 with cycle walking), the stream layout of
include/simamba.h, the slot-to-sample map and the three row rules.  Integer arithmetic throughout, so every comparison
of indices is bit for bit.  ``unit_sphere64`` is pc_norm in float64 on given picks, with the error bound of the fp32
kernel derived from its order of operations."""
import numpy as np

from augment_ref import MASK32, philox4x32_10

SEQUENTIAL, SHUFFLE = 0, 1
FIRST, PERMUTE, CHOICE = 0, 1, 2
NONE, UNIT_SPHERE = 0, 1
STREAM_SHUFFLE, STREAM_ROWS, STREAM_CHOICE = 1, 2, 3
DOMAIN = 0x80000000          # bit 31 of c1 in every Philox block drawn here
MASK64 = (1 << 64) - 1
U = 2.0 ** -24               # unit roundoff of fp32


def stream(purpose, epoch, p):
    """purpose << 60 | (epoch mod 2^29) << 31 | p"""
    assert 0 <= p < 1 << 31
    return (purpose << 60) | ((int(epoch) & ((1 << 29) - 1)) << 31) | int(p)


def half_bits(n):
    bits = 0
    while (1 << bits) < n:
        bits += 1
    return 1 if bits < 2 else (bits + 1) // 2


def _words(strm, shape):
    """(low, high) 32-bit words of a stream, or of an array of streams, as uint64 arrays of ``shape``."""
    if isinstance(strm, np.ndarray):
        strm = np.broadcast_to(strm.astype(np.uint64), shape)
        return strm & np.uint64(MASK32), strm >> np.uint64(32)
    strm = int(strm) & MASK64
    return np.full(shape, strm & MASK32, dtype=np.uint64), np.full(shape, strm >> 32, dtype=np.uint64)


def _network(h, seed, lo, hi, x):
    mask = np.uint64((1 << h) - 1)
    key = (seed & MASK32, seed >> 32)
    L, R = x >> np.uint64(h), x & mask
    for r in range(4):
        F = philox4x32_10(key, (R, np.full(x.shape, DOMAIN | r, dtype=np.uint64), lo, hi))[0] & mask
        L, R = R, L ^ F
    return (L << np.uint64(h)) | R


def perm(n, seed, strm, i):
    """perm(n, seed, stream, i) for an int or an array i of values in [0, n): int64 array of i's shape.  ``strm``: one
    stream, or a uint64 array of streams that broadcasts against i (one per row, say)."""
    seed = int(seed) & MASK64
    i = np.asarray(i, dtype=np.uint64)
    assert 1 <= n < 1 << 31 and (i.size == 0 or int(i.max()) < n)
    if n == 1:
        return np.zeros(i.shape, dtype=np.int64)
    h = half_bits(n)
    lo, hi = (w.ravel() for w in _words(strm, i.shape))
    x = _network(h, seed, lo, hi, i.ravel().copy())
    while True:
        out = np.nonzero(x >= np.uint64(n))[0]
        if out.size == 0:
            break
        x[out] = _network(h, seed, lo[out], hi[out], x[out])
    return x.astype(np.int64).reshape(i.shape)


def steps_per_epoch(S, B, world, drop_last):
    return S // (B * world) if drop_last else -(-S // (B * world))


def slot_samples(S, B, seed, step, spe, rank=0, world=1, shuffle=True):
    """(index (B,) int64 with -1 in empty slots, epoch, the global positions p (B,))."""
    step = int(step) & MASK64
    epoch, pos = divmod(step, spe)
    p = (pos * B + np.arange(B, dtype=np.int64)) * world + rank
    idx = np.full(B, -1, dtype=np.int64)
    ok = p < S
    if shuffle:
        idx[ok] = perm(S, seed, stream(STREAM_SHUFFLE, epoch, 0), p[ok])
    else:
        idx[ok] = p[ok]
    return idx, epoch, p


def candidates(n_s, first):
    return min(n_s, first) if first > 0 else n_s


def rows_of(c, K, rows, seed, epoch, p):
    """The rows that slots at the global positions p (an int or an (m,) array) take out of c candidates each:
    int64 (m, len) (or (len,) for an int p), len = K for CHOICE, else min(K, c)."""
    single = np.ndim(p) == 0
    p = np.atleast_1d(np.asarray(p, dtype=np.int64))
    if c == 0:
        out = np.zeros((len(p), 0), dtype=np.int64)
    elif rows == FIRST:
        out = np.broadcast_to(np.arange(min(K, c), dtype=np.int64), (len(p), min(K, c))).copy()
    elif rows == PERMUTE:
        strm = np.array([stream(STREAM_ROWS, epoch, int(q)) for q in p], dtype=np.uint64)[:, None]
        out = perm(c, seed, strm, np.broadcast_to(np.arange(min(K, c)), (len(p), min(K, c))))
    else:
        assert rows == CHOICE
        seed = int(seed) & MASK64
        strm = np.array([stream(STREAM_CHOICE, epoch, int(q)) for q in p], dtype=np.uint64)[:, None]
        i = np.broadcast_to(np.arange(K, dtype=np.uint64), (len(p), K))
        lo, hi = _words(strm, i.shape)
        w = philox4x32_10((seed & MASK32, seed >> 32), (i, np.full(i.shape, DOMAIN, dtype=np.uint64), lo, hi))[0]
        out = ((w * np.uint64(c)) >> np.uint64(32)).astype(np.int64)          # w < 2^32, c < 2^31: no overflow
    return out[0] if single else out


def slot_rows(n_s, K, first, rows, seed, epoch, p):
    """The rows of a cloud of n_s points that the slot at global position p takes: int64 (len,)."""
    return rows_of(candidates(n_s, first), K, rows, seed, epoch, int(p))


def batch(lengths, B, K, seed, step, spe, rank=0, world=1, shuffle=True, rows=PERMUTE, first=0):
    """The whole map for a store whose cloud s has lengths[s] points: (index (B,) int64 with -1 in empty slots,
    picks (B, K) int64 with -1 behind a slot's length, length (B,) int64).  Slots with equal candidate counts are
    computed together."""
    idx, epoch, p = slot_samples(len(lengths), B, seed, step, spe, rank, world, shuffle)
    lengths = np.asarray(lengths, dtype=np.int64)
    picks = np.full((B, K), -1, dtype=np.int64)
    length = np.zeros(B, dtype=np.int64)
    c = np.where(idx >= 0, lengths[np.maximum(idx, 0)], 0)
    if first > 0:
        c = np.minimum(c, first)
    for cv in np.unique(c[idx >= 0]):
        at = np.nonzero((idx >= 0) & (c == cv))[0]
        got = rows_of(int(cv), K, rows, seed, epoch, p[at])
        picks[at, :got.shape[1]] = got
        length[at] = got.shape[1]
    return idx, picks, length


# ---- pc_norm -------------------------------------------------------------------------------------------------------
SUM_DEPTH = 8 + 6 + 16       # additions a term of the kernel's sum passes through at most: lane, butterfly, waves


def unit_sphere64(rows):
    """pc_norm of (n, 3) rows in float64, and the bound on |kernel - this| per coordinate.

    With A = max |coordinate| and u = 2^-24, to first order in u:
      d = row - row 0, |d| <= 2 A, one subtraction:                  |d~ - d| <= 2 u A
      mean of d: every term passes at most SUM_DEPTH additions, then one division, and carries d's own error:
            |mean~ - mean| <= (SUM_DEPTH + 1) u 2 A + 2 u A
      r = d - mean, |r| <= 2 A per coordinate, one subtraction:
            e_r = 2 u A + (2 SUM_DEPTH + 4) u A + 2 u A = (2 SUM_DEPTH + 8) u A
      m = max |r|: the perturbation of r moves a norm by at most sqrt(3) e_r; the squares, their two sums and the root
            add a relative 4 u:                                      |m~ - m| <= sqrt(3) e_r + 4 u m
      out = r / m, |r| / m <= 1, one division:
            |out~ - out| <= e_r / m + (sqrt(3) e_r / m + 4 u) + u
    and 1 % on top for the terms of second order (SUM_DEPTH u < 2e-6)."""
    x = np.asarray(rows, dtype=np.float64)
    A = np.abs(x).max()
    r = x - x.mean(0)
    m = np.sqrt((r * r).sum(1)).max()
    if m == 0:
        return np.zeros_like(x), 0.0
    e_r = (2 * SUM_DEPTH + 8) * U * A
    return r / m, 1.01 * ((1 + np.sqrt(3)) * e_r / m + 5 * U)
