"""CPU: simamba_corrupt_points (csrc/corrupt.hip) is declared, bound and exported and refuses every bad argument before
a launch; the Python tables hold what they document; the restatement (corrupt_ref.py) draws under a key of its own and
meets the structural rules of every kind; evaluate_robustness' arithmetic equals a hand computation.  No device is
touched here."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import augment_ref as ar
import corrupt_ref as cf
from abi_tables import E_NULLPTR, E_SHAPE, E_VARIANT, P, check_rows, declared_params, header_code
from si_mamba_amd import _lib, corruptions

NAN = float("nan")
NAME = "simamba_corrupt_points"


def par(*v):
    """A host array of four fp32 parameters, as the table passes it (kept alive by the module)."""
    arr = (ctypes.c_float * 4)(*v)
    _KEEP.append(arr)
    return arr


_KEEP = []
OUT = P + (1 << 26)         # far behind points: 4 x 8192 x 12 bytes fit in between
BASE = dict(points=P, lengths=None, out=OUT, out_lengths=P, src=None, state=P, kind=cf.DROP_GLOBAL, flags=0,
            params=par(0.5), B=4, N=1024, K=1024, stream=None)


def kind(k, *v, **more):
    return dict(kind=k, params=par(*v), **more)


ROWS = [
    # shape
    (dict(B=0), E_SHAPE), (dict(B=-1), E_SHAPE), (dict(B=1 << 31), E_SHAPE),
    (dict(N=0, K=0), E_SHAPE), (dict(N=0), E_SHAPE), (dict(N=-1, K=-1), E_SHAPE), (dict(N=8193, K=8193), E_SHAPE),
    (dict(K=8193), E_SHAPE), (dict(K=1023), E_SHAPE), (dict(K=0), E_SHAPE), (dict(N=8192, K=8191), E_SHAPE),
    # null pointers; the limits of B, N and K pass the shape check and end at a null pointer, nothing launched
    (dict(points=None), E_NULLPTR), (dict(out=None), E_NULLPTR), (dict(out_lengths=None), E_NULLPTR),
    (dict(state=None), E_NULLPTR), (dict(params=None), E_NULLPTR),
    (dict(N=1, K=1, state=None), E_NULLPTR), (dict(N=8192, K=8192, state=None), E_NULLPTR),
    (dict(N=1, K=8192, state=None), E_NULLPTR), (dict(B=(1 << 31) - 1, out=None), E_NULLPTR),
    (dict(lengths=P, src=P, state=None), E_NULLPTR),
    # every kind with accepted parameters reaches the null pointer
    *[(dict(**kind(*k), flags=f, state=None), E_NULLPTR)
      for k in ((cf.DROP_GLOBAL, 0.0), (cf.DROP_GLOBAL, 0.75), (cf.DROP_LOCAL, 500, 8), (cf.DROP_LOCAL, 0, 1),
                (cf.ADD_GLOBAL, 50, 1.0), (cf.ADD_GLOBAL, 1e9, NAN), (cf.ADD_LOCAL, 500, 8, 0.075, 0.125),
                (cf.ROTATE3, math.pi / 6), (cf.ROTATE3, NAN), (cf.SCALE_AXES, 1.0), (cf.SCALE_AXES, 2.0),
                (cf.JITTER, 0.05), (cf.JITTER, -1.0))
      for f in (0, cf.RENORM)],
    # the kind, the flags and the parameters
    (dict(kind=0), E_VARIANT), (dict(kind=8), E_VARIANT), (dict(kind=-1), E_VARIANT),
    (dict(flags=2), E_VARIANT), (dict(flags=3), E_VARIANT), (dict(flags=-1), E_VARIANT),
    (kind(cf.DROP_GLOBAL, 1.0), E_VARIANT), (kind(cf.DROP_GLOBAL, -0.25), E_VARIANT), (kind(cf.DROP_GLOBAL, NAN), E_VARIANT),
    (kind(cf.DROP_LOCAL, -1, 8), E_VARIANT), (kind(cf.DROP_LOCAL, NAN, 8), E_VARIANT),
    (kind(cf.DROP_LOCAL, 100, 0), E_VARIANT), (kind(cf.DROP_LOCAL, 100, 9), E_VARIANT),
    (kind(cf.DROP_LOCAL, 100, 2.5), E_VARIANT), (kind(cf.DROP_LOCAL, 100, NAN), E_VARIANT),
    (kind(cf.ADD_GLOBAL, -1, 1.0), E_VARIANT), (kind(cf.ADD_GLOBAL, NAN, 1.0), E_VARIANT),
    (kind(cf.ADD_LOCAL, -1, 8, .1, .2), E_VARIANT), (kind(cf.ADD_LOCAL, 100, 0, .1, .2), E_VARIANT),
    (kind(cf.ADD_LOCAL, 100, 9, .1, .2), E_VARIANT),
    (kind(cf.SCALE_AXES, 0.5), E_VARIANT), (kind(cf.SCALE_AXES, NAN), E_VARIANT), (kind(cf.SCALE_AXES, -2.0), E_VARIANT),
    # out over points: never, not even row for row
    (dict(out=P), E_VARIANT), (dict(out=P + 12), E_VARIANT), (dict(out=P + 4 * 1024 * 12 - 4), E_VARIANT),
    (dict(out=P - 4 * 1024 * 12 + 4), E_VARIANT), (dict(out=P + 4 * 1024 * 12, state=None), E_NULLPTR),
    (dict(K=2048, out=P - 4 * 2048 * 12 + 4), E_VARIANT),
    # two faults: the shape in front of the null pointer, the null pointer in front of the variant, the variant in
    # front of the overlap (either answer is E_VARIANT; the order shows in the rows above)
    (dict(N=0, K=0, points=None), E_SHAPE), (dict(K=1023, state=None), E_SHAPE), (dict(B=0, kind=9), E_SHAPE),
    (dict(kind=9, points=None), E_NULLPTR), (dict(flags=2, out_lengths=None), E_NULLPTR),
    (dict(kind=cf.SCALE_AXES, params=None), E_NULLPTR), (dict(**kind(cf.SCALE_AXES, 0.5), state=None), E_NULLPTR),
    (dict(kind=9, out=P), E_VARIANT), (dict(**kind(cf.DROP_GLOBAL, 1.0), out=P), E_VARIANT),
]


def test_symbol_is_declared_bound_and_exported():
    assert NAME in declared_params()
    assert NAME in _lib.SIGNATURES
    assert set(declared_params()) == set(_lib.SIGNATURES)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert _lib.load().simamba_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert re.search(r"#define\s+SIMAMBA_ABI_VERSION\s+9\b", header_code())
    assert declared_params()[NAME][-1] == "void* stream"
    assert not any(re.match(r"(const\s+)?double\b", p) for p in declared_params()[NAME])


def test_return_codes_without_a_device():
    check_rows(NAME, BASE, ROWS)


def test_opcodes_agree_with_the_binding_and_the_header():
    header = {k: int(v, 0) for k, v in
              re.findall(r"#define\s+SIMAMBA_CORRUPT_([A-Z_0-9]+)\s+(0x[0-9A-Fa-f]+|\d+)", header_code())}
    assert header == dict(DROP_GLOBAL=1, DROP_LOCAL=2, ADD_GLOBAL=3, ADD_LOCAL=4, ROTATE3=5, SCALE_AXES=6, JITTER=7,
                          RENORM=1, MAX_CLUSTERS=8, KEY_TWEAK=0x434F5252)
    for k, v in header.items():
        assert getattr(_lib, "CORRUPT_" + k) == v
        assert getattr(cf, k) == v
    assert {k: (code, names) for k, (code, names, _) in corruptions._SPEC.items()} == cf.KIND


def test_kinds_and_severity_tables():
    import si_mamba_amd as sm
    for name in ("corruptions", "KINDS", "SEVERITY", "corrupt", "evaluate_robustness"):
        assert hasattr(sm, name) and name in sm.__all__, name
    assert sm.KINDS == ("drop_global", "drop_local", "add_global", "add_local", "rotate", "scale", "jitter")
    S = sm.SEVERITY
    assert set(S) == set(sm.KINDS) and all(len(S[k]) == 5 for k in S)
    assert [d["ratio"] for d in S["drop_global"]] == [0.25, 0.375, 0.5, 0.625, 0.75]
    assert [(d["total"], d["max_clusters"]) for d in S["drop_local"]] == [(100 * l, 8) for l in range(1, 6)]
    assert [d["count"] for d in S["add_global"]] == [10 * l for l in range(1, 6)]
    assert [(d["total"], d["max_clusters"], d["sigma_low"], d["sigma_high"]) for d in S["add_local"]] == \
        [(100 * l, 8, 0.075, 0.125) for l in range(1, 6)]
    assert [d["theta"] for d in S["rotate"]] == [math.pi * l / 30 for l in range(1, 6)]
    assert [d["scale"] for d in S["scale"]] == [1.6, 1.7, 1.8, 1.9, 2.0]
    assert [d["sigma"] for d in S["jitter"]] == [0.01 * l for l in range(1, 6)]
    assert [k for k, (_, _, renorm) in corruptions._SPEC.items() if renorm] == ["scale"]
    for k in sm.KINDS:                                        # every set names exactly the kind's parameters
        for d in S[k]:
            assert corruptions.kind_params(k, 1, **d) == d or k == "add_global"
            assert set(corruptions.kind_params(k, 1, **d)) == set(cf.KIND[k][1])
    assert corruptions.kind_params("jitter", 2, sigma=0.5) == dict(sigma=0.5)
    assert corruptions.kind_params("add_global", count=3) == dict(count=3, radius=1.0)
    with pytest.raises(ValueError):
        corruptions.kind_params("melt", 1)
    with pytest.raises(ValueError):
        corruptions.kind_params("jitter", 6)
    with pytest.raises(TypeError):
        corruptions.kind_params("jitter", 1, ratio=0.5)
    with pytest.raises(TypeError):
        corruptions.kind_params("drop_local", total=5)


def test_python_route_refuses_cpu_tensors_and_grad():
    pc = torch.zeros(2, 16, 3)
    for k in corruptions.KINDS:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            corruptions.corrupt(pc, k, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        corruptions.evaluate_robustness(lambda x, lengths=None: x, pc, torch.zeros(2, dtype=torch.long))
    with pytest.raises(ValueError):
        corruptions.corrupt(torch.zeros(2, 16, 4), "jitter", 1)
    with pytest.raises(ValueError):
        corruptions.corrupt(torch.zeros(16, 3), "jitter", 1)
    with pytest.raises(TypeError, match="lengths"):           # before anything else is looked at
        corruptions.evaluate_robustness(lambda x: x, pc, torch.zeros(2, dtype=torch.long))

    class NoLengths(torch.nn.Module):
        def forward(self, x):
            return x

    with pytest.raises(TypeError, match="lengths"):
        corruptions.evaluate_robustness(NoLengths(), pc, torch.zeros(2, dtype=torch.long))


# ---- the restatement itself ------------------------------------------------------------------------------------------
SEED, STEP = 0x299f31d0a4093822, (0x0abcdef1 << 32) | 0x13198a2e


def test_restatement_key_tweak_and_counter_layout():
    """The same [seed, step], cloud and block: other words than augment's at every chain position, and the counter
    where include/simamba.h says."""
    for per_point in (False, True):
        got = cf.block(SEED, STEP, 5, per_point, np.array([7, 9]))
        c3 = 0x0abcdef1 | ((1 << 31) if per_point else 0)
        for k, i in enumerate((7, 9)):
            want = ar.philox4x32_10((0xa4093822, 0x299f31d0 ^ 0x434F5252), (i, 5, 0x13198a2e, c3))
            assert [int(w[k]) for w in got] == [int(v) for v in want]
            mine = tuple(int(w[k]) for w in got)
            for pos in range(8):
                theirs = tuple(int(w) for w in ar.block(SEED, STEP, 5, pos, per_point, i))
                assert mine != theirs and not set(mine) & set(theirs)
    # the tweak is the key's high word only: augment's block under the tweaked seed
    a = cf.block(SEED, STEP, 2, True, 11)
    b = ar.block(SEED ^ (cf.KEY_TWEAK << 32), STEP, 2, 0, True, 11)
    assert [int(v) for v in a] == [int(v) for v in b]


def _cloud(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, size=(n, 3)).astype(np.float32)


NS = [1, 2, 129, 1024]


@pytest.mark.parametrize("n", NS)
def test_restatement_drop_kinds(n):
    pts = _cloud(n, n)
    for ratio in (0.0, 0.25, 0.75, float(np.float32(1 - 2.0 ** -24))):
        r = cf.corrupt_cloud(pts, cf.DROP_GLOBAL, (ratio,), SEED, STEP, 1)
        m = min(int(np.float32(n) * np.float32(ratio)), n - 1)
        assert r["removed"] == m and r["len"] == n - m >= 1
        assert np.all(np.diff(r["src"]) > 0) and r["src"].min() >= 0 and r["src"].max() < n
        assert np.array_equal(r["out"], pts[r["src"]].astype(np.float64))
    for total in (0, 1, 100, 500, 5000):
        for cmax in (1, 3, 8):
            r = cf.corrupt_cloud(pts, cf.DROP_LOCAL, (total, cmax), SEED, STEP, 2)
            Tp = min(total, n - 1)
            assert 1 <= len(r["sizes"]) <= cmax and sum(r["sizes"]) == Tp
            assert max(r["sizes"]) - min(r["sizes"]) <= 1 and r["sizes"] == sorted(r["sizes"], reverse=True)
            assert r["len"] == n - Tp >= 1
            assert np.all(np.diff(r["src"]) > 0) and (n == 1 or r["src"].max() < n)
            assert np.array_equal(r["out"], pts[r["src"]].astype(np.float64))


def test_restatement_drop_local_takes_the_nearest_and_breaks_ties_by_index():
    """One cluster on a line of points: the seed and its nearest neighbours go; at equal distance the lower index."""
    pts = np.zeros((9, 3), dtype=np.float32)
    pts[:, 0] = np.arange(9)
    keep, sizes, seeds = cf.dropped_local(pts, 3, 1, SEED, STEP, 0)
    s = seeds[0]
    assert sizes == [3] and 0 <= s < 9
    gone = sorted(np.nonzero(~keep)[0].tolist())
    want = sorted(sorted(range(9), key=lambda i: (abs(i - s), i))[:3])
    assert gone == want and s in gone
    same = np.ones((5, 3), dtype=np.float32)                       # identical points: every distance ties
    keep, sizes, _ = cf.dropped_local(same, 2, 1, SEED, STEP, 0)
    assert np.nonzero(~keep)[0].tolist() == [0, 1]


@pytest.mark.parametrize("n", NS)
def test_restatement_add_kinds(n):
    pts = _cloud(n, 100 + n)
    for A, R in ((0, 1.0), (50, 1.0), (50, 0.25)):
        r = cf.corrupt_cloud(pts, cf.ADD_GLOBAL, (A, R), SEED, STEP, 3)
        assert r["len"] == n + A and np.array_equal(r["src"][:n], np.arange(n)) and np.all(r["src"][n:] == -1)
        assert np.array_equal(r["out"][:n], pts.astype(np.float64))
        assert np.all(np.linalg.norm(r["out"][n:], axis=1) <= R * (1 + 1e-12))
    r = cf.corrupt_cloud(pts, cf.ADD_GLOBAL, (50, 1.0), SEED, STEP, 3, K=n + 7)          # clamped: K - n rows
    assert r["len"] == n + 7
    for T in (0, 5, 500):
        r = cf.corrupt_cloud(pts, cf.ADD_LOCAL, (T, 8, 0.075, 0.125), SEED, STEP, 4)
        assert r["len"] == n + T and sum(r["sizes"]) == T and 1 <= len(r["sizes"]) <= 8
        assert np.array_equal(r["out"][:n], pts.astype(np.float64))
        assert np.array_equal(r["src"][n:], -1 - np.repeat(np.arange(len(r["sizes"])), r["sizes"]))
        assert all(0 <= s < n for s in r["seeds"])
        assert all(np.float32(0.075) <= s <= np.float32(0.125) for s in r["sigmas"])
        # a Box-Muller radius is below 5.8 (augment_ref), so a point lies within 5.8 sqrt(2) sigma_hi of its seed
        owner = -1 - r["src"][n:]
        far = np.linalg.norm(r["out"][n:] - pts[np.array(r["seeds"], dtype=np.int64)[owner]], axis=1)
        assert np.all(far <= 5.8 * np.sqrt(2) * 0.125)
    r = cf.corrupt_cloud(pts, cf.ADD_LOCAL, (500, 8, 0.075, 0.125), SEED, STEP, 4, K=n + 3)
    assert r["len"] == n + 3 and sum(r["sizes"]) == 3


def test_restatement_rigid_kinds():
    pts = _cloud(129, 7)
    th = math.pi / 6
    r = cf.corrupt_cloud(pts, cf.ROTATE3, (th,), SEED, STEP, 0)
    assert all(abs(float(a)) <= np.float32(th) for a in r["angles"]) and len(set(map(float, r["angles"]))) == 3
    assert np.allclose(np.linalg.norm(r["out"], axis=1), np.linalg.norm(pts.astype(np.float64), axis=1), atol=1e-12)
    r = cf.corrupt_cloud(np.eye(3, dtype=np.float32), cf.ROTATE3, (0.0,), SEED, STEP, 0)
    assert np.array_equal(r["out"], np.eye(3))
    r = cf.corrupt_cloud(pts, cf.SCALE_AXES, (2.0,), SEED, STEP, 0, renorm=True)
    assert all(np.float32(0.5) <= f <= np.float32(2.0) for f in r["factors"])
    assert abs(np.linalg.norm(r["out"], axis=1).max() - 1) < 1e-12 and np.abs(r["out"].mean(0)).max() < 1e-12
    r = cf.corrupt_cloud(pts, cf.SCALE_AXES, (1.0,), SEED, STEP, 0)
    assert np.array_equal(r["out"], pts.astype(np.float64))
    r = cf.corrupt_cloud(pts, cf.JITTER, (0.05,), SEED, STEP, 0)
    z = (r["out"] - pts) / np.float64(np.float32(0.05))
    assert np.allclose(z, cf.normals(SEED, STEP, 0, 129), atol=1e-9) and 0.7 < z.std() < 1.3


# ---- evaluate_robustness' arithmetic -----------------------------------------------------------------------------------
def test_robustness_scores_equal_a_hand_computation():
    """10 clouds, 9 right when clean; two kinds at two severities."""
    res = corruptions.robustness_scores(9, [[8, 6], [5, 5]], 10, ("jitter", "rotate"), (1, 2))
    assert res["total"] == 10 and res["clean_acc"] == 0.9 and abs(res["clean_err"] - 0.1) < 1e-15
    assert res["acc"] == {"jitter": [0.8, 0.6], "rotate": [0.5, 0.5]}
    assert np.allclose(res["err"]["jitter"], [0.2, 0.4]) and np.allclose(res["err"]["rotate"], [0.5, 0.5])
    assert abs(res["mean_acc"] - 0.6) < 1e-15 and "CE" not in res and "mCE" not in res
    base = {"clean": 0.05, "jitter": [0.1, 0.2], "rotate": [0.25, 0.75]}
    res = corruptions.robustness_scores(9, [[8, 6], [5, 5]], 10, ("jitter", "rotate"), (1, 2), base)
    # CE: (0.2 + 0.4) / (0.1 + 0.2) = 2, (0.5 + 0.5) / (0.25 + 0.75) = 1; mCE = 1.5
    assert abs(res["CE"]["jitter"] - 2.0) < 1e-12 and abs(res["CE"]["rotate"] - 1.0) < 1e-12
    assert abs(res["mCE"] - 1.5) < 1e-12
    # RCE: (0.1 + 0.3) / (0.05 + 0.15) = 2, (0.4 + 0.4) / (0.2 + 0.7) = 8 / 9; RmCE = 13 / 9
    assert abs(res["RCE"]["jitter"] - 2.0) < 1e-12 and abs(res["RCE"]["rotate"] - 8 / 9) < 1e-12
    assert abs(res["RmCE"] - 13 / 9) < 1e-12
    with pytest.raises(ValueError):
        corruptions.robustness_scores(9, [[8, 6]], 10, ("jitter",), (1, 2), {"clean": 0.05, "jitter": [0.1]})
