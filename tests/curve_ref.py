"""numpy restatement of si_mamba_amd/csrc/curve_order.hip (include/simamba.h, simamba_curve_order): the float64 cell of
every coordinate, the Morton and Hilbert codes as plain integer loops, and a stable argsort.  A helper module: pytest
collects nothing from it.

TEST INFRASTRUCTURE.  Everything here is integer arithmetic except the cell, which is three correctly rounded float64
operations (a subtraction, a division, a multiplication by a power of two), so the kernel is held to exact equality.
"""
import numpy as np

CURVES = {"z": 0, "hilbert": 1, "z-trans": 2, "hilbert-trans": 3}         # the header's SIMAMBA_CURVE_* ids
DEFAULT_CURVES = ("hilbert", "hilbert-trans", "z", "z-trans")


def cells(centers, bits, box="cloud"):
    """centers (B, G, 3) float32 -> (B, G, 3) int64 cells on the 2^bits lattice."""
    c = np.asarray(centers, dtype=np.float32)
    assert c.ndim == 3 and c.shape[2] == 3
    top = (1 << bits) - 1
    finite = np.isfinite(c)
    if isinstance(box, str):
        assert box == "cloud"
        lo = np.where(finite, c, np.float32(np.inf)).min(axis=1)                           # (B, 3) float32
        hi = np.where(finite, c, np.float32(-np.inf)).max(axis=1)
        has = hi >= lo
        with np.errstate(invalid="ignore", over="ignore"):
            extent = np.where(has, hi - lo, np.float32(0)).astype(np.float32)              # one fp32 subtraction
        lo = np.where(has, lo, np.float32(0)).astype(np.float32)
        ext = extent.max(axis=1)                                                           # (B,) float32
    else:
        blo, bhi = np.float32(box[0]), np.float32(box[1])
        lo = np.full((c.shape[0], 3), blo, dtype=np.float32)
        with np.errstate(over="ignore"):
            ext = np.full(c.shape[0], bhi - blo, dtype=np.float32)                         # inf: every cell is 0
    x = np.where(finite, c, np.float32(0)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (x - lo.astype(np.float64)[:, None, :]) / ext.astype(np.float64)[:, None, None] * float(1 << bits)
    v = np.where(np.isnan(v), 0.0, v)                                                      # ext == 0 below anyway
    q = np.clip(np.floor(v), 0, top).astype(np.int64)
    q = np.where((ext == 0)[:, None, None], 0, q)
    return np.where(finite, q, top)


def morton(x, y, z, bits):
    """Bit i of x, y, z at bits 3i+2, 3i+1, 3i, one bit at a time."""
    x, y, z = (np.asarray(v, dtype=np.int64) for v in (x, y, z))
    code = np.zeros(np.broadcast(x, y, z).shape, dtype=np.int64)
    for i in range(bits):
        code |= ((x >> i) & 1) << (3 * i + 2)
        code |= ((y >> i) & 1) << (3 * i + 1)
        code |= ((z >> i) & 1) << (3 * i)
    return code


def hilbert(x, y, z, bits):
    """Skilling, "Programming the Hilbert curve" (AIP Conf. Proc. 707, 2004): AxestoTranspose on (x, y, z), the
    transposed index read out most significant bit first, axis 0 first."""
    X = [np.array(v, dtype=np.int64, copy=True) for v in np.broadcast_arrays(x, y, z)]
    M = 1 << (bits - 1)
    Q = M
    while Q > 1:                                         # inverse undo
        P = Q - 1
        for i in range(3):
            hit = (X[i] & Q) != 0
            t = np.where(hit, 0, (X[0] ^ X[i]) & P)
            X[0] = np.where(hit, X[0] ^ P, X[0] ^ t)
            X[i] = X[i] ^ t if i else X[0]               # i == 0: t is 0 and X[0] was just updated
        Q >>= 1
    X[1] = X[1] ^ X[0]                                   # Gray encode
    X[2] = X[2] ^ X[1]
    t = np.zeros_like(X[0])
    Q = M
    while Q > 1:
        t = np.where((X[2] & Q) != 0, t ^ (Q - 1), t)
        Q >>= 1
    X = [v ^ t for v in X]
    return morton(X[0], X[1], X[2], bits)


def codes(centers, curves=DEFAULT_CURVES, bits=10, box="cloud"):
    """(B, G, 3) -> (B, len(curves), G) int64: the code of every patch on every curve."""
    q = cells(centers, bits, box)
    out = []
    for name in curves:
        cid = CURVES[name]
        a, b = (q[..., 1], q[..., 0]) if cid & 2 else (q[..., 0], q[..., 1])
        out.append((hilbert if cid & 1 else morton)(a, b, q[..., 2], bits))
    return np.stack(out, axis=1)


def order(centers, curves=DEFAULT_CURVES, bits=10, box="cloud"):
    """-> (order (B, k, G) int64, codes (B, k, G) int64): ascending by (code, patch index)."""
    c = codes(centers, curves, bits, box)
    return np.argsort(c, axis=-1, kind="stable").astype(np.int64), c


def lattice(side):
    """The side^3 integer cells, (side^3, 3) int64, x slowest."""
    g = np.arange(side, dtype=np.int64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def lattice_centers(side, rng=None):
    """Cell centres of the full lattice in the fixed box (0, side): (1, side^3, 3) float32, shuffled by ``rng``."""
    cell = lattice(side)
    if rng is not None:
        cell = cell[rng.permutation(len(cell))]
    return (cell.astype(np.float32) + np.float32(0.5))[None], cell
