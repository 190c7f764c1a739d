"""Point clouds on a binary lattice, and the float64 answers of the selection kernels on them.

TEST INFRASTRUCTURE (shared by test_oracle_lattice_clouds.py, CPU, and test_gpu_lattice_selection.py).  FPS, k-NN
grouping, 3-NN interpolation and the one-wave Chamfer kernel all pick indices by arg-min / arg-max and all document
one tie rule: the lower index wins.  On Gaussian clouds no two distances are ever equal, so that rule never runs.  Here
every coordinate is an integer in [-R, R] divided by a power of two: every fp32 difference, square, product and sum of
the kernels is then exact (the integers stay far below 2^24), distances are equal exactly when they are equal in float64,
and a float64 brute force with a stable sort / first maximum is THE answer, index for index, with nothing to mask.
Small R forces repeated points (R = 2 has 125 sites) on top of the ties between the lattice's shells.

  lattice                 random lattice clouds
  fps_pair, knn_shell     directed inputs: one tie at chosen indices (which register, lane or wave holds either side)
  chamfer_sets            lattice set pairs with a repeated prediction and target in every other pair
  fps_ref .. chamfer_ref  the float64 references (stable sorts, first maximum)
  *_tied                  the share of decisions that really are ties, from the inputs alone (test_oracle_lattice_clouds
                          asserts them for every case below: they are what makes the GPU comparisons mean something)
  *_CASES                 the shapes both test files walk

No GPU code runs here and no expected output is written down.
"""
import itertools

import numpy as np
import torch

EPS32 = float(np.float32(1e-8))          # three_nn's 1e-8f as the kernel holds it
FAR32 = float(np.float32(3.0e38))        # the distance three_nn gives the repeated slots when S < 3


# ---- inputs ----------------------------------------------------------------------------------------------------------
def lattice(B, N, R, seed, scale=8):
    """(B, N, 3) fp32: integer coordinates in [-R, R] over ``scale`` (a power of two)."""
    assert scale & (scale - 1) == 0
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-R, R + 1, (B, N, 3), generator=g).float() / scale


def subset(points, S, seed):
    """S of every cloud's points, in a random order: centres that coincide with points, as after FPS."""
    g = torch.Generator().manual_seed(seed)
    return points[:, torch.randperm(points.shape[1], generator=g)[:S]].clone()


def fps_pair(N, a, b):
    """(1, N, 3): every point at the origin but a at (1, 0, 0) and b at (-1, 0, 0), 0 < a, b < N.  From point 0 the two
    are equally far, then the other one is still 1 away from the picked set, then everything is at distance 0:
    picks [0, min(a, b), max(a, b), 0, 0, ...]."""
    assert 0 < a < N and 0 < b < N and a != b
    p = torch.zeros(1, N, 3)
    p[0, a, 0], p[0, b, 0] = 1.0, -1.0
    return p


_SHELL = sorted({tuple(s * v for s, v in zip(sg, pm)) for pm in itertools.permutations((1, 2, 3))
                 for sg in itertools.product((1, -1), repeat=3)})           # 48 vectors of one length


def knn_shell(N, where, far=64.0):
    """(centre (1, 1, 3) at the origin, points (1, N, 3)): the points at the indices ``where`` (at most 48) sit at
    distinct permutations / sign flips of (1, 2, 3) / 8, all equally far from the centre; every other point is far away.
    The K = len(where) - 1 nearest are the K lowest of ``where``, ascending."""
    assert len(where) <= len(_SHELL) and len(set(where)) == len(where) and max(where) < N
    p = torch.full((1, N, 3), far)
    for i, v in zip(where, _SHELL):
        p[0, i] = torch.tensor(v) / 8
    return torch.zeros(1, 1, 3), p


def chamfer_sets(pairs, n, m, seed, R=2):
    """(pred (pairs, n, 3), gt (pairs, m, 3)) on the lattice.  In every even pair the last target is a copy of target 0,
    prediction 0 sits on both, and the last prediction is a copy of prediction 0 (where the set has two points): each
    direction has a tie at distance 0 between index 0 and the last index, and the lower copy owns the match -- and with
    it, for the predictions, target 0's term of the gradient."""
    pred, gt = lattice(pairs, n, R, seed), lattice(pairs, m, R, seed + 1)
    if m > 1:
        gt[0::2, m - 1] = gt[0::2, 0]
    pred[0::2, 0] = gt[0::2, 0]
    if n > 1:
        pred[0::2, n - 1] = pred[0::2, 0]
    return pred, gt


def small_integers(count, seed, lo=-3, hi=4):
    """(count,) fp32 integers in [lo, hi]: gradients of the Chamfer distance that keep every product exact."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, (count,), generator=g).float()


# ---- distances -------------------------------------------------------------------------------------------------------
def direct_distance(a, b):
    """(B, n, 3), (B, m, 3) -> (B, n, m): (dx^2 + dy^2) + dz^2 in the dtype of the arguments (FPS, k-NN, Chamfer)."""
    d = a[:, :, None, :] - b[:, None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _first_max(v):
    return int((v == v.max()).nonzero()[0])


# ---- float64 references ----------------------------------------------------------------------------------------------
def fps_ref(points, K, lengths=None, start_idx=None):
    """Farthest-point sampling in float64, first maximum on ties -> (centers (B, K, 3) fp32, idx (B, K) int64).  Cloud b
    is its first lengths[b] points and starts at start_idx[b]; with fewer than K points the rest is -1 / 0."""
    B, N, _ = points.shape
    idx = torch.full((B, K), -1, dtype=torch.long)
    centers = torch.zeros(B, K, 3)
    for b in range(B):
        n = N if lengths is None else int(lengths[b])
        p = points[b, :n].double()
        cur = 0 if start_idx is None else int(start_idx[b])
        md = torch.full((n,), float("inf"), dtype=torch.float64)
        for r in range(min(K, n)):
            idx[b, r] = cur
            centers[b, r] = points[b, cur]
            md = torch.minimum(md, direct_distance(p[None], p[None, cur:cur + 1])[0, :, 0])
            cur = _first_max(md)
    return centers, idx


def knn_ref(centers, points, K, lengths=None):
    """(B, G, K) int64: the first K of the stable float64 argsort of every centre's distances to its cloud's first
    lengths[b] points; slots past lengths[b] are 0."""
    B, G, _ = centers.shape
    out = torch.zeros(B, G, K, dtype=torch.long)
    for b in range(B):
        n = points.shape[1] if lengths is None else int(lengths[b])
        d = direct_distance(centers[b:b + 1].double(), points[b:b + 1, :n].double())[0]
        k = min(K, n)
        out[b, :, :k] = d.sort(dim=-1, stable=True)[1][:, :k]
    return out


def three_nn_ref(xyz1, xyz2):
    """(idx (B, N, 3) int64 in order of distance, weight (B, N, 3) float64): the first three of the stable float64
    argsort and the normalised 1 / (d + 1e-8f).  With S < 3 centres the last one is repeated at the kernel's stand-in
    distance 3e38, which makes the repeated slots' weight about 1e-38."""
    S = xyz2.shape[1]
    d, idx = direct_distance(xyz1.double(), xyz2.double()).sort(dim=-1, stable=True)
    d, idx = d[..., :3], idx[..., :3]
    if S < 3:
        pad = 3 - S
        idx = torch.cat([idx, idx[..., -1:].expand(-1, -1, pad)], -1)
        d = torch.cat([d, torch.full(d.shape[:2] + (pad,), FAR32, dtype=torch.float64)], -1)
    r = 1.0 / (d + EPS32)
    return idx, r / r.sum(-1, keepdim=True)


def interpolate_ref(feats, idx, weight):
    """out[b, n] = sum_k w[b, n, k] feats[b, idx[b, n, k]] in float64 -> (out, sum_k |w v|), both (B, N, C)."""
    B, N, _ = idx.shape
    f, w = feats.double(), weight.double()
    rows = torch.arange(B)[:, None, None]
    terms = f[rows, idx.long()] * w[..., None]                     # (B, N, 3, C)
    return terms.sum(2), terms.abs().sum(2)


def interpolate_grad_ref(dout, idx, weight, S):
    """dfeats[b, s] = sum over the entries (n, k) with idx[b, n, k] == s of w[b, n, k] dout[b, n] in float64
    -> (dfeats, sum |w dout|, number of entries), shapes (B, S, C), (B, S, C), (B, S)."""
    B, N, _ = idx.shape
    C = dout.shape[-1]
    d, w = dout.double(), weight.double()
    grad = torch.zeros(B, S, C, dtype=torch.float64)
    mag = torch.zeros(B, S, C, dtype=torch.float64)
    cnt = torch.zeros(B, S, dtype=torch.long)
    for b in range(B):
        for k in range(3):
            t = d[b] * w[b, :, k, None]
            grad[b].index_add_(0, idx[b, :, k].long(), t)
            mag[b].index_add_(0, idx[b, :, k].long(), t.abs())
            cnt[b].index_add_(0, idx[b, :, k].long(), torch.ones(N, dtype=torch.long))
    return grad, mag, cnt


def chamfer_ref(pred, gt, ddist=None):
    """The one-wave kernel's outputs in float64: dist (P,), idx1 (P, n) nearest target of every prediction, idx2 (P, m)
    nearest prediction of every target (stable: the lowest index among equals), and, given ddist (P,), dpred (P, n, 3) =
    g (2/n (p_i - gt[idx1_i]) + 2/m sum_{j: idx2_j = i} (p_i - gt_j))."""
    p, g = pred.double(), gt.double()
    P, n, _ = p.shape
    m = g.shape[1]
    d = direct_distance(p, g)
    d1, idx1 = (t[..., 0] for t in d.sort(dim=2, stable=True))
    d2, idx2 = (t[..., 0] for t in d.transpose(1, 2).sort(dim=2, stable=True))
    out = {"dist": d1.sum(1) / n + d2.sum(1) / m, "idx1": idx1, "idx2": idx2}
    if ddist is not None:
        rows = torch.arange(P)[:, None]
        dp = (2.0 / n) * (p - g[rows, idx1])
        back = (2.0 / m) * (p[rows, idx2] - g)                     # (P, m, 3): target j's pull on prediction idx2_j
        dp.scatter_add_(1, idx2[..., None].expand(-1, -1, 3), back)
        out["dpred"] = dp * ddist.double()[:, None, None]
    return out


# ---- how many decisions are ties (float64, inputs only) -------------------------------------------------------------
def fps_tied(points, K, lengths=None, start_idx=None):
    """(rounds, tied): the arg-max decisions FPS takes (K - 1 per cloud, fewer for short clouds) and how many of them
    have the maximum at two or more points."""
    B, N, _ = points.shape
    rounds = tied = 0
    for b in range(B):
        n = N if lengths is None else int(lengths[b])
        p = points[b, :n].double()
        cur = 0 if start_idx is None else int(start_idx[b])
        md = torch.full((n,), float("inf"), dtype=torch.float64)
        for r in range(min(K, n) - 1):
            md = torch.minimum(md, direct_distance(p[None], p[None, cur:cur + 1])[0, :, 0])
            rounds += 1
            tied += int((md == md.max()).sum()) > 1
            cur = _first_max(md)
    return rounds, tied


def knn_tied(centers, points, K, lengths=None):
    """(rows, boundary, inside): the rows that have more candidates than K (all rows, for ``inside``, when none has), how
    many of them have d_K == d_(K+1) (the tie decides who is in the row), and how many have two equal distances among
    their first K (the tie decides the order)."""
    rows = boundary = inside = 0
    for b in range(centers.shape[0]):
        n = points.shape[1] if lengths is None else int(lengths[b])
        d = direct_distance(centers[b:b + 1].double(), points[b:b + 1, :n].double())[0].sort(dim=-1)[0]
        k = min(K, n)
        inside += int((d[:, 1:k] == d[:, :k - 1]).any(-1).sum())
        if n > K:
            rows += d.shape[0]
            boundary += int((d[:, K - 1] == d[:, K]).sum())
    return rows, boundary, inside


def three_nn_tied(xyz1, xyz2):
    """(rows, tied): query points, and how many have their third and fourth nearest centres equally far (S > 3)."""
    d = direct_distance(xyz1.double(), xyz2.double()).sort(dim=-1)[0]
    return d.shape[0] * d.shape[1], int((d[..., 2] == d[..., 3]).sum())


def chamfer_tied(pred, gt):
    """(tied1, tied2): predictions with two or more nearest targets, targets with two or more nearest predictions."""
    d = direct_distance(pred.double(), gt.double())
    t1 = ((d == d.min(2, keepdim=True)[0]).sum(2) > 1).sum()
    t2 = ((d == d.min(1, keepdim=True)[0]).sum(1) > 1).sum()
    return int(t1), int(t2)


# ---- the cases both test files walk ----------------------------------------------------------------------------------
# FPS: (N, K, R).  256 lanes x 16 registers up to N = 4096, 1024 lanes x 8 above; (300, 300) has about 110 distinct
# sites, so the picks must repeat.
FPS_CASES = [(1, 1, 4), (100, 17, 4), (255, 32, 4), (256, 32, 4), (257, 32, 4), (1024, 128, 6), (4096, 64, 6),
             (4097, 64, 6), (8192, 128, 8), (300, 300, 2)]
FPS_BATCH = 2
# ragged FPS: clouds of these lengths (and the full N) padded to N; the padding holds a point that would win if read
FPS_RAGGED_LENGTHS = (1, 63, 64, 65, 257)
FPS_RAGGED = [(1024, 32, 4), (4097, 32, 6)]                    # (N, K, R)
# directed FPS ties, offsets from a: same lane (256: the 256-lane kernel, 1024: the wide one), same wave (1, 32),
# different waves (64, 192)
FPS_PAIR_N = (1024, 8192)
FPS_PAIR_A = 37
FPS_PAIR_OFFSETS = (1, 32, 64, 192, 256, 1024)

# k-NN: (N, G, K, R), one per register count (16, 32, 64, 128 per lane), then the small and degenerate ones
KNN_CASES = [(1024, 130, 32, 6), (2048, 33, 32, 8), (4096, 17, 32, 8), (8192, 10, 64, 12), (100, 17, 9, 3),
             (64, 8, 64, 3), (1, 1, 1, 3), (256, 16, 1, 2)]
KNN_BATCH = 2
KNN_RAGGED = (1024, 9, 16, 4)                                  # (N, G, K, R) with lengths (1, 63, 65, N)
KNN_RAGGED_LENGTHS = (1, 63, 65)
# directed k-NN ties, offsets from a: same lane (64, 256), same wave (1, 32)
KNN_SHELL_N = (1024, 8192)
KNN_SHELL_A = 70
KNN_SHELL_OFFSETS = (1, 32, 64, 256)

# 3-NN: (B, N, S, R); the centres are S of the points
NN_CASES = [(2, 512, 64, 4), (3, 300, 37, 3), (1, 8192, 256, 6), (2, 256, 3, 3), (2, 130, 2, 3), (1, 2048, 2, 4),
            (2, 64, 1, 3)]
# interpolation forward and backward: (B, N, S, R, C); S = 2 at N = 2048 names one centre more than N times
INTERP_CASES = [(2, 512, 64, 4, 8), (3, 300, 37, 3, 1152), (1, 8192, 256, 6, 8), (2, 256, 3, 3, 8), (2, 130, 2, 3, 8),
                (1, 2048, 2, 4, 8), (1, 2048, 2, 4, 1152), (2, 64, 1, 3, 8)]

# one-wave Chamfer: (n, m) x pairs
CHAMFER_SHAPES = [(32, 32), (64, 64), (1, 64), (64, 1), (8, 16)]
CHAMFER_PAIRS = (1, 5, 1001)


def fps_case(N, K, R):
    return lattice(FPS_BATCH, N, R, 1000 + N + K)


def fps_ragged_case(N, K, R, last):
    """(points, lengths, start_idx): ``last`` starts every cloud at its last point instead of its first."""
    lengths = torch.tensor(FPS_RAGGED_LENGTHS + (N,))
    pts = lattice(len(lengths), N, R, 2000 + N)
    for b, n in enumerate(lengths):
        pts[b, int(n):] = 64.0
    return pts, lengths, (lengths - 1 if last else torch.zeros_like(lengths))


def knn_case(N, G, K, R):
    return lattice(KNN_BATCH, G, R, 3000 + N + G), lattice(KNN_BATCH, N, R, 4000 + N + K)


def knn_ragged_case():
    N, G, K, R = KNN_RAGGED
    lengths = torch.tensor(KNN_RAGGED_LENGTHS + (N,))
    pts = lattice(len(lengths), N, R, 5000)
    for b, n in enumerate(lengths):
        pts[b, int(n):] = 0.0                                   # the middle of the cloud: near every centre, if read
    return lattice(len(lengths), G, R, 5001), pts, K, lengths


def nn_case(B, N, S, R):
    pts = lattice(B, N, R, 6000 + N + S)
    return pts, subset(pts, S, 6001 + N + S)


def interp_case(B, N, S, R, C, dtype):
    """(xyz1, xyz2, feats (B, S, C), dout (B, N, C)): the features rounded to ``dtype`` once, kept as fp32."""
    xyz1, xyz2 = nn_case(B, N, S, R)
    g = torch.Generator().manual_seed(7000 + N + S + C)
    feats = torch.randn(B, S, C, generator=g).to(dtype).float()
    dout = torch.randn(B, N, C, generator=g).to(dtype).float()
    return xyz1, xyz2, feats, dout


def chamfer_case(n, m, pairs):
    pred, gt = chamfer_sets(pairs, n, m, 8000 + 64 * n + m)
    return pred, gt, small_integers(pairs, 8001 + n + m + pairs)
