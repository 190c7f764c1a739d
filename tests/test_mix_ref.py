"""CPU: the numpy restatement of csrc/mix.hip (tests/mix_ref.py) pinned on its own: the partner map is the library's
keyed permutation, m follows its formula at the edges of lambda, the mixed cloud is a disjoint union of own and partner
rows, the anchors are those of a brute-force float32 farthest-point sampling, and the lattice case of test_gpu_mix.py
really puts ties on the selection boundary.  No device is touched here."""
import ctypes

import numpy as np
import pytest

import corrupt_ref as cf
import mix_ref as mr
from si_mamba_amd import _lib

SEED, STEP = mr.SEED, mr.STEP
f32 = np.float32


def host_perm(seed, stream, n):
    out = (ctypes.c_longlong * n)()
    sgn = lambda v: v - (1 << 64) if v >= 1 << 63 else v           # noqa: E731
    assert _lib.load().simamba_keyed_perm(sgn(seed), sgn(stream), n, 0, n, out) == 0
    return np.array(out[:], dtype=np.int64)


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 16, 17, 64, 257])
def test_partner_map_is_the_keyed_permutation(B):
    for step in (0, STEP, STEP + 1, STEP + 2):
        got = mr.partner_map(B, SEED, step)
        assert np.array_equal(got, host_perm(mr.mix_seed(SEED), step, B)), (B, step)
        assert sorted(got.tolist()) == list(range(B))
    if B >= 16:                                                     # another step, another key: another map
        assert not np.array_equal(mr.partner_map(B, SEED, STEP), mr.partner_map(B, SEED, STEP + 1))
        assert not np.array_equal(mr.partner_map(B, SEED, STEP), host_perm(SEED, STEP, B))
        assert not np.array_equal(mr.partner_map(B, SEED, STEP), host_perm(SEED ^ (cf.KEY_TWEAK << 32), STEP, B))


def test_key_tweaks_are_distinct_and_the_streams_differ():
    assert mr.KEY_TWEAK != cf.KEY_TWEAK and mr.KEY_TWEAK == _lib.MIX_KEY_TWEAK and mr.KEY_TWEAK >> 32 == 0
    for per_point in (False, True):
        mine = {int(w[0]) for w in mr.block(SEED, STEP, 3, per_point, [7])}
        theirs = {int(w[0]) for w in cf.block(SEED, STEP, 3, per_point, [7])}
        assert not mine & theirs
    a = mr.block(SEED, STEP, 2, True, 11)                            # the tweak is the key's high word only
    b = cf.block(SEED ^ ((cf.KEY_TWEAK ^ mr.KEY_TWEAK) << 32), STEP, 2, True, 11)
    assert [int(v) for v in a] == [int(v) for v in b]


def test_rows_taken_at_the_edges_of_lambda():
    below1 = float(f32(1) - f32(2.0 ** -24))
    for n in (1, 7, 8, 9, 511, 512, 513, 8191, 8192):
        assert mr.rows_taken(n, n, 0.0) == 0
        assert mr.rows_taken(n, n, 2.0 ** -24) == 0                  # n 2^-24 < 1 for every n <= 8192
        assert mr.rows_taken(n, n, 0.5) == n // 2                    # n / 2 is exact in float32
        assert mr.rows_taken(n, n, 1.0) == n
        # n (1 - 2^-24) = n - n 2^-24: for n = 2^k that is the float32 just below n, exactly; for 2^k < n < 2^(k+1) it
        # lies more than half an ulp (2^(k-24)) and less than one ulp below n and rounds to the float32 just below n
        assert mr.rows_taken(n, n, below1) == n - 1
    # the partner is shorter than (int)(n_b lambda)
    assert mr.rows_taken(512, 7, 0.5) == 7 and mr.rows_taken(8192, 1, 1.0) == 1 and mr.rows_taken(9, 8, 1.0) == 8
    assert mr.rows_taken(7, 512, 1.0) == 7
    # lambda as the kernel forces it into [0, 1]
    assert mr.lam_of(float("nan"), SEED, STEP, 0) == 0 and mr.lam_of(-0.5, SEED, STEP, 0) == 0
    assert mr.lam_of(1.5, SEED, STEP, 0) == 1 and mr.lam_of(float("inf"), SEED, STEP, 0) == 1
    assert mr.lam_of(0.25, SEED, STEP, 0) == f32(0.25)
    drawn = [mr.lam_of(None, SEED, STEP, b) for b in range(64)]
    assert all(0 <= v < 1 for v in drawn) and len(set(map(float, drawn))) == 64
    assert mr.clamp_partner(-3, 4) == 0 and mr.clamp_partner(9, 4) == 3 and mr.clamp_partner(2, 4) == 2


def _cloud(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, size=(n, 3)).astype(f32)


@pytest.mark.parametrize("mode", [mr.CUT_R, mr.CUT_K])
@pytest.mark.parametrize("nb,nq", [(1, 1), (9, 7), (7, 9), (513, 512), (129, 1024)])
def test_mixed_cloud_is_a_disjoint_union(mode, nb, nq):
    own, other = _cloud(nb, nb), _cloud(nq, 1000 + nq)
    for lam in (0.0, 0.3, 0.5, 1.0, None):
        r = mr.cutmix_cloud(own, other, mode, lam, SEED, STEP, 3)
        m = r["m"]
        assert m == min(int(f32(f32(nb) * r["lam"])), nb, nq) and r["ratio"] == f32(f32(m) / f32(nb))
        src = r["src"]
        assert len(src) == nb == len(r["out"]) and len(r["removed"]) == m == len(r["taken"])
        mine, theirs = src[src >= 0], -1 - src[src < 0]
        assert len(mine) == nb - m and len(theirs) == m
        assert np.array_equal(src[:nb - m], mine) and np.all(np.diff(mine) > 0) and np.all(np.diff(theirs) > 0)
        assert not set(mine.tolist()) & set(r["removed"].tolist())
        assert sorted(mine.tolist() + r["removed"].tolist()) == list(range(nb))
        assert theirs.size == 0 or (theirs.min() >= 0 and theirs.max() < nq)
        assert np.array_equal(r["out"][:nb - m].view(np.uint32), own[mine].view(np.uint32))
        assert np.array_equal(r["out"][nb - m:].view(np.uint32), other[theirs].view(np.uint32))
        if mode == mr.CUT_K and m:                                   # the nearest m of each side, its seed among them
            so, sq = r["seeds"]
            assert so in r["removed"] and sq in r["taken"]
            assert r["d2"][0][r["removed"]].max() <= np.delete(r["d2"][0], r["removed"]).min(initial=np.inf)
            assert r["d2"][1][r["taken"]].max() <= np.delete(r["d2"][1], r["taken"]).min(initial=np.inf)
    same = mr.cutmix_cloud(own, own, mode, 0.5, SEED, STEP, 3)      # a cloud with itself: made of its own rows
    assert set(map(tuple, same["out"].tolist())) <= set(map(tuple, own.tolist())) and len(same["out"]) == nb


def test_mode_r_draws_both_sides_from_one_block_under_the_output_cloud():
    own, other = _cloud(64, 1), _cloud(64, 2)
    r = mr.cutmix_cloud(own, other, mr.CUT_R, 0.25, SEED, STEP, 5)
    w = mr.block(SEED, STEP, 5, True, np.arange(64))
    assert r["removed"].tolist() == sorted(np.argsort(w[0], kind="stable")[:16].tolist())
    assert r["taken"].tolist() == sorted(np.argsort(w[1], kind="stable")[:16].tolist())
    assert r["removed"].tolist() != r["taken"].tolist()


def brute_fps(p, M, first):
    """Farthest-point sampling spelled out row by row in float32."""
    rows = [first]
    for _ in range(1, M):
        best, best_row = f32(-1), -1
        for i in range(len(p)):
            near = min(f32(f32(f32(p[i, 0] - p[r, 0]) * f32(p[i, 0] - p[r, 0])
                               + f32(p[i, 1] - p[r, 1]) * f32(p[i, 1] - p[r, 1]))
                           + f32(p[i, 2] - p[r, 2]) * f32(p[i, 2] - p[r, 2])) for r in rows)
            if near > best:                                          # strictly: ties stay with the lower row
                best, best_row = near, i
        rows.append(best_row)
    return rows


@pytest.mark.parametrize("n,M", [(1, 4), (7, 8), (9, 3), (125, 8), (200, 4)])
def test_anchors_equal_a_brute_force_float32_fps(n, M):
    p = mr.lattice(5) if n == 125 else _cloud(n, 50 + n)
    for b in range(3):
        r = mr.pointwolf_cloud(p, M, (0.5, 0.17, 3.0, 0.25), SEED, STEP, b)
        first = mr.pick(mr.block(SEED, STEP, b, False, 0)[0], n)
        assert r["anchors"][0] == first and r["anchors"] == brute_fps(p, M, first)
        assert all(0 <= a < n for a in r["anchors"])
        if n >= M and n != 125:
            assert len(set(r["anchors"])) == M
    if n == 125:                                                     # the lattice's corners tie: the lower row wins
        d = mr.d2_f32(p, p[r["anchors"][0]])
        assert (d == d.max()).sum() >= 1 and r["anchors"][1] == int(np.nonzero(d == d.max())[0][0])


def test_pointwolf_restatement_draws_and_limits():
    p = _cloud(129, 9)
    r = mr.pointwolf_cloud(p, 4, (0.5, 0.17, 3.0, 0.25), SEED, STEP, 1)
    assert np.all(np.abs(r["angles"]) <= f32(0.17)) and np.all(np.abs(r["shifts"]) <= f32(0.25))
    fac = r["factors"]
    assert np.all((fac >= f32(1 / 3) * (1 - 1e-6)) & (fac <= 3)) and len({float(v) for v in fac.ravel()}) == 12
    assert all((row >= 1).all() or (row <= 1).all() for row in fac)   # one inversion bit for the three axes
    assert r["c"] == f32(2.0) and r["args"].max() == 0 and np.all((r["args"] == 0).sum(1) >= 1)
    assert r["args"].min() >= mr.EXP_ARG_MIN
    # no rotation, no scale, no shift: every q_j(p) is p, so is the blend
    still = mr.pointwolf_cloud(p, 4, (0.5, 0.0, 1.0, 0.0), SEED, STEP, 1)
    assert np.abs(still["out"] - p.astype(np.float64)).max() < 1e-15
    # one anchor: its transform alone
    one = mr.pointwolf_cloud(p, 1, (0.5, 0.0, 1.0, 0.25), SEED, STEP, 1)
    assert np.allclose(one["out"], p.astype(np.float64) + one["shifts"][0].astype(np.float64), atol=1e-15)


def test_lattice_case_puts_ties_on_the_selection_boundary():
    """The (m)-th and (m + 1)-th smallest d2 are equal on both sides of every cloud of the GPU test's lattice batch, for
    the seeds drawn at (SEED, STEP): the rule that ties go to the lower row decides which rows move."""
    L = mr.lattice(5)
    assert L.shape == (125, 3)
    for b, lam in enumerate(mr.LATTICE_LAM):
        r = mr.cutmix_cloud(L, L, mr.CUT_K, lam, SEED, STEP, b)
        m = r["m"]
        assert 0 < m < 125
        for d2, rows in zip(r["d2"], (r["removed"], r["taken"])):
            s = np.sort(d2)
            assert s[m - 1] == s[m], (b, lam, m)
            edge = np.nonzero(d2 == s[m - 1])[0]                     # the shell the boundary cuts through
            inside = np.intersect1d(edge, rows)
            assert 0 < len(inside) < len(edge) and np.array_equal(inside, edge[:len(inside)])
