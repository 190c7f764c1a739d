"""CPU: the augmentation entry points (csrc/augment.hip) validate their arguments before touching a device, the host
Philox of the library and the numpy one of augment_ref.py both give the Random123 known answers and agree with each
other, the pointnet2_ops stand-in resolves, the transform classes carry the reference's defaults, and the seed the GPU
distribution test uses meets its bounds under the restatement."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import augment_ref as ar
from abi_tables import E_NULLPTR, E_SHAPE, E_VARIANT, P, check_rows
from si_mamba_amd import _lib


def _philox_lib(key, ctr):
    out = (ctypes.c_uint * 4)()
    seed = (key[1] << 32) | key[0]
    seed = seed - (1 << 64) if seed >= 1 << 63 else seed
    assert _lib.load().simamba_philox4x32_10(seed, *ctr, out) == 0
    return tuple(int(v) for v in out)


def _philox_ref(key, ctr):
    return tuple(int(v) for v in ar.philox4x32_10(key, ctr))


# Random123's known-answer vectors for philox4x32_10 (counter, key, result)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert _philox_lib(key, ctr) == want
    assert _philox_ref(key, ctr) == want


def test_philox_library_and_numpy_agree_on_random_counters():
    rng = np.random.default_rng(0)
    keys = rng.integers(0, 1 << 32, size=(1000, 2), dtype=np.uint64)
    ctrs = rng.integers(0, 1 << 32, size=(1000, 4), dtype=np.uint64)
    want = np.stack(ar.philox4x32_10((keys[:, 0], keys[:, 1]), tuple(ctrs[:, k] for k in range(4))), -1)
    for key, ctr, w in zip(keys.tolist(), ctrs.tolist(), want.tolist()):
        assert _philox_lib(key, ctr) == tuple(w)
    assert _lib.load().simamba_philox4x32_10(0, 0, 0, 0, 0, None) == E_NULLPTR


def _chain(*ops):
    """(ops, op_params) host arrays; ops: (opcode, p0, p1, ...)."""
    n = max(len(ops), 1)
    codes, params = (ctypes.c_int * n)(), (ctypes.c_float * (4 * n))()
    for o, (code, *p) in enumerate(ops):
        codes[o] = code
        for k, v in enumerate(p):
            params[4 * o + k] = v
    return codes, params


OPS1, PAR1 = _chain((ar.SCALE_TRANSLATE, 2 / 3, 3 / 2, 0.2))
OPS9, PAR9 = _chain(*[(ar.ROTATE,)] * 9)
OPS_BAD, PAR_BAD = _chain((ar.ROTATE,), (8,))
OPS_ZERO, PAR_ZERO = _chain((0,))
OPS_AXIS, PAR_AXIS = _chain((ar.FLIP, 3.0))
OPS_ALL, PAR_ALL = _chain((ar.ROTATE,), (ar.SCALE, .5, 2.), (ar.TRANSLATE, .1), (ar.SCALE_TRANSLATE, .5, 2., .1),
                          (ar.JITTER, .01, .05), (ar.DROPOUT, .5), (ar.FLIP, 2.), (ar.FLIP, 0.))

POINTS = dict(points=P, idx=None, idx_is_64=0, sel=None, lengths=None, out=P + (1 << 24), ops=OPS1, op_params=PAR1,
              n_ops=1, state=P, B=4, N=1024, M=1024, K=1024, stream=None)
GATHER = dict(idx=P, M=1200, sel=P)          # on top of POINTS: (B, 1200) indices, 1024 of them selected
POINT_ROWS = [
    (dict(N=0, M=0, K=0), E_SHAPE), (dict(N=8193, M=8193, K=8193), E_SHAPE), (dict(**GATHER, K=8193), E_SHAPE),
    (dict(**GATHER, K=0), E_SHAPE), (dict(idx=P, M=8193, K=8193), E_SHAPE), (dict(idx=P, M=0, K=0), E_SHAPE),
    (dict(**GATHER, N=0), E_SHAPE), (dict(**GATHER, N=8193), E_SHAPE), (dict(N=-1, M=-1, K=-1), E_SHAPE),
    (dict(B=0), E_SHAPE), (dict(B=-1), E_SHAPE), (dict(B=1 << 31), E_SHAPE),
    (dict(n_ops=9, ops=OPS9, op_params=PAR9), E_SHAPE), (dict(n_ops=-1), E_SHAPE),
    (dict(M=1200, K=1200), E_SHAPE),                          # no idx: M is N
    (dict(idx=P, M=1200), E_SHAPE),                           # no sel: K is M
    (dict(sel=P, K=512, M=1200), E_SHAPE),
    # null pointers; the limits of N, M and K pass the shape check and end at a null pointer, nothing launched
    (dict(points=None), E_NULLPTR), (dict(out=None), E_NULLPTR), (dict(state=None), E_NULLPTR),
    (dict(ops=None), E_NULLPTR), (dict(op_params=None), E_NULLPTR),
    (dict(N=1, M=1, K=1, state=None), E_NULLPTR), (dict(N=8192, M=8192, K=8192, state=None), E_NULLPTR),
    (dict(**GATHER, N=8192, state=None), E_NULLPTR), (dict(idx=P, sel=P, N=1, M=8192, K=8192, out=None), E_NULLPTR),
    (dict(n_ops=0, ops=None, op_params=None, points=None), E_NULLPTR),        # an empty chain needs no arrays
    (dict(n_ops=8, ops=OPS_ALL, op_params=PAR_ALL, state=None), E_NULLPTR),   # every opcode, eight ops
    (dict(B=(1 << 31) - 1, out=None), E_NULLPTR),
    # the chain
    (dict(n_ops=2, ops=OPS_BAD, op_params=PAR_BAD), E_VARIANT), (dict(ops=OPS_ZERO, op_params=PAR_ZERO), E_VARIANT),
    (dict(ops=OPS_AXIS, op_params=PAR_AXIS), E_VARIANT),
    # out over points: only row for row, and never with a gather or a subset
    (dict(**GATHER, out=P), E_VARIANT), (dict(idx=P, out=P), E_VARIANT), (dict(sel=P, K=512, out=P), E_VARIANT),
    (dict(out=P + 12), E_VARIANT), (dict(**GATHER, out=P + 4 * 1024 * 12 - 12), E_VARIANT),
    # two faults: the shape in front of the null pointer, the null pointer in front of the chain, the chain in front of
    # the overlap
    (dict(N=0, M=0, K=0, points=None), E_SHAPE), (dict(N=8193, M=8193, K=8193, state=None), E_SHAPE),
    (dict(**GATHER, K=8193, out=None), E_SHAPE), (dict(n_ops=9, ops=None), E_SHAPE),
    (dict(n_ops=2, ops=OPS_BAD, op_params=PAR_BAD, points=None), E_NULLPTR),
    (dict(**GATHER, out=P, ops=OPS_ZERO, op_params=PAR_ZERO), E_VARIANT),
]

PARAMS = dict(lengths=None, ops=OPS1, op_params=PAR1, n_ops=1, state=P, cloud_params=P, noise=None, keep=None, B=4,
              K=1024, stream=None)
PARAM_ROWS = [
    (dict(K=0), E_SHAPE), (dict(K=8193), E_SHAPE), (dict(B=0), E_SHAPE), (dict(B=1 << 31), E_SHAPE),
    (dict(n_ops=9, ops=OPS9, op_params=PAR9), E_SHAPE),
    (dict(state=None), E_NULLPTR), (dict(cloud_params=None), E_NULLPTR), (dict(ops=None), E_NULLPTR),
    (dict(op_params=None), E_NULLPTR), (dict(K=1, state=None), E_NULLPTR), (dict(K=8192, state=None), E_NULLPTR),
    (dict(n_ops=2, ops=OPS_BAD, op_params=PAR_BAD), E_VARIANT), (dict(ops=OPS_AXIS, op_params=PAR_AXIS), E_VARIANT),
    (dict(K=0, state=None), E_SHAPE), (dict(n_ops=2, ops=OPS_BAD, op_params=PAR_BAD, state=None), E_NULLPTR),
]


def test_return_codes_without_a_device():
    check_rows("simamba_augment_points", POINTS, POINT_ROWS)
    check_rows("simamba_augment_params", PARAMS, PARAM_ROWS)


def test_out_over_points_with_a_gather_is_refused():
    """A gather reads rows that other lanes, or other clouds' workgroups, write: with either index width."""
    check_rows("simamba_augment_points", POINTS, [(dict(**GATHER, out=P), E_VARIANT),
                                                  (dict(idx=P, idx_is_64=1, out=P), E_VARIANT)])


def test_opcodes_agree_with_the_binding_and_the_header():
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "simamba.h")).read()
    header = {k: int(v) for k, v in re.findall(r"#define SIMAMBA_AUG_([A-Z_]+)\s+(\d+)", text)}
    assert header == dict(ROTATE=1, SCALE=2, TRANSLATE=3, SCALE_TRANSLATE=4, JITTER=5, DROPOUT=6, FLIP=7, MAX_OPS=8,
                          CLOUD_PARAMS=8)
    for k, v in header.items():
        assert getattr(_lib, "AUG_" + k) == v
        if k not in ("MAX_OPS",):
            assert getattr(ar, k) == v


def test_pointnet2_shim_resolves_and_refuses_to_shadow():
    import types
    from si_mamba_amd import install_shim
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "pointnet2_ops" or k.startswith("pointnet2_ops.")}
    try:
        install_shim()                                       # not asked for: not registered
        assert "pointnet2_ops" not in sys.modules
        install_shim(pointnet2=True)
        from pointnet2_ops import pointnet2_utils
        assert callable(pointnet2_utils.furthest_point_sample) and callable(pointnet2_utils.gather_operation)
        import pointnet2_ops.pointnet2_utils as again
        assert again is pointnet2_utils
        install_shim(pointnet2=True)                         # its own stand-in may be replaced
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pointnet2_utils.furthest_point_sample(torch.zeros(1, 8, 3), 4)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pointnet2_utils.gather_operation(torch.zeros(1, 3, 8), torch.zeros(1, 4, dtype=torch.int32))
        for k in [k for k in sys.modules if k == "pointnet2_ops" or k.startswith("pointnet2_ops.")]:
            del sys.modules[k]
        sys.modules["pointnet2_ops"] = types.ModuleType("pointnet2_ops")        # a "real" package
        with pytest.raises(RuntimeError, match="pointnet2_ops"):
            install_shim(pointnet2=True)
        install_shim()                                       # the plain shim does not care
    finally:
        for k in [k for k in sys.modules if k == "pointnet2_ops" or k.startswith("pointnet2_ops.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_classes_carry_the_reference_defaults():
    import si_mamba_amd as sm
    from si_mamba_amd import transforms as T
    for name in ("PointcloudRotate", "PointcloudScaleAndTranslate", "PointcloudJitter", "PointcloudScale",
                 "PointcloudTranslate", "PointcloudRandomInputDropout", "RandomHorizontalFlip", "Compose",
                 "AugmentState", "sample_and_augment", "vote_logits"):
        assert hasattr(sm, name), name
    st = T.PointcloudScaleAndTranslate()
    assert (st.scale_low, st.scale_high, st.translate_range) == (2. / 3., 3. / 2., 0.2)
    assert st.op() == (ar.SCALE_TRANSLATE, (2. / 3., 3. / 2., 0.2))
    s = T.PointcloudScale()
    assert (s.scale_low, s.scale_high) == (2. / 3., 3. / 2.) and s.op()[0] == ar.SCALE
    t = T.PointcloudTranslate()
    assert t.translate_range == 0.2 and t.op() == (ar.TRANSLATE, (0.2,))
    j = T.PointcloudJitter()
    assert (j.std, j.clip) == (0.01, 0.05) and j.op() == (ar.JITTER, (0.01, 0.05))
    d = T.PointcloudRandomInputDropout()
    assert d.max_dropout_ratio == 0.5 and d.op() == (ar.DROPOUT, (0.5,))
    with pytest.raises(AssertionError):
        T.PointcloudRandomInputDropout(1.0)
    f = T.RandomHorizontalFlip()
    assert f.upright_axis == 2 and f.horz_axes == {0, 1} and f.D == 3 and f.op() == (ar.FLIP, (2.0,))
    assert T.RandomHorizontalFlip("Y").op() == (ar.FLIP, (1.0,))
    with pytest.raises(NotImplementedError):
        T.RandomHorizontalFlip(is_temporal=True)
    assert T.PointcloudRotate().op() == (ar.ROTATE, ())
    # positional construction as the reference's configs do
    assert T.PointcloudScaleAndTranslate(0.9, 1.1, 0.0).op()[1] == (0.9, 1.1, 0.0)


def test_compose_schedules_fused_runs_and_foreign_callables():
    from si_mamba_amd import transforms as T
    a, b, c = T.PointcloudRotate(), T.PointcloudJitter(), T.RandomHorizontalFlip()
    foreign = lambda pc: pc                                                    # noqa: E731
    assert T.Compose([a, b, c]).runs() == [[a, b, c]]
    assert T.Compose([a, foreign, b, c]).runs() == [[a], foreign, [b, c]]
    assert T.Compose([foreign, a]).runs() == [foreign, [a]]
    assert [len(r) for r in T.Compose([a] * 19).runs()] == [8, 8, 3]
    assert T.Compose([]).runs() == []
    with pytest.raises(TypeError):
        T.Compose([a, 3])


def test_python_route_refuses_cpu_tensors_and_grad():
    from si_mamba_amd import transforms as T
    pc = torch.zeros(2, 16, 3)
    for t in (T.PointcloudRotate(), T.PointcloudScaleAndTranslate(), T.PointcloudJitter(), T.PointcloudScale(),
              T.PointcloudTranslate(), T.PointcloudRandomInputDropout(), T.RandomHorizontalFlip(),
              T.Compose([T.PointcloudRotate(), T.PointcloudJitter()])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            t(pc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.sample_and_augment(pc, [T.PointcloudRotate()])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.AugmentState(0, "cpu")
    with pytest.raises(ValueError):
        T.sample_and_augment(torch.zeros(2, 16, 4), [])
    with pytest.raises(ValueError):
        T.sample_and_augment(torch.zeros(16, 3), [])
    from si_mamba_amd import vote_logits
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vote_logits(lambda p: p, pc, 8, point_all=16)


# ---- the restatement itself ------------------------------------------------------------------------------------------
def test_restatement_counter_layout():
    """block() places its arguments where include/simamba.h says."""
    seed, step = 0x299f31d0a4093822, (0x0abcdef1 << 32) | 0x13198a2e
    got = ar.block(seed, step, cloud=5, pos=3, per_point=True, index=np.array([7, 9]))
    c3 = 0x0abcdef1 | (3 << 28) | (1 << 31)
    for k, i in enumerate((7, 9)):
        want = ar.philox4x32_10((0xa4093822, 0x299f31d0), (i, 5, 0x13198a2e, c3))
        assert [int(w[k]) for w in got] == [int(v) for v in want]
    a = ar.block(seed, step, 5, 3, False, 0)
    b = ar.block(seed, step, 5, 4, False, 0)
    c = ar.block(seed, step + 1, 5, 3, False, 0)
    d = ar.block(seed, step, 6, 3, False, 0)
    words = {tuple(int(v) for v in w) for w in (a, b, c, d, [g[0] for g in got])}
    assert len(words) == 5
    assert ar.uniform(0xffffffff) == np.float32(1 - 2.0 ** -24) and ar.uniform(0xff) == 0 and ar.uniform(0x100) == np.float32(2.0 ** -24)
    n0, n1 = ar.normal_pair(0, 0)                       # the largest radius: sqrt(-2 ln 2^-24)
    assert abs(n0 - np.sqrt(48 * np.log(2))) < 1e-12 and n1 == 0 and n0 < 5.8


def test_restatement_on_a_hand_worked_chain():
    pts = np.array([[1., 2., 3.], [-1., 0., 5.], [0., 4., -2.]])
    chain = [(ar.ROTATE, ()), (ar.SCALE_TRANSLATE, (1, 1, 0)), (ar.DROPOUT, (.5,)), (ar.FLIP, (2.,))]
    draws = np.zeros((4, 8))
    draws[0, :3] = np.pi / 2, 0., 1.                    # x' = -z, z' = x
    draws[1, :6] = 2, 1, 1, 0, 0, 10
    draws[2, 0] = .25
    draws[3, :4] = 1, 1, 0, 0                           # flip x only
    got, big = ar.apply_chain(pts, chain, draws, keep=np.array([False, True, False]))
    # rotate: (-3,2,1) (-5,0,-1) (2,4,0); scale x by 2, z + 10: (-6,2,11) (-10,0,9) (4,4,10); rows 0, 2 become row 0:
    # (-6,2,11) (-10,0,9) (-6,2,11); flip x about its maximum -6: (0,2,11) (4,0,9) (0,2,11)
    assert got.tolist() == [[0, 2, 11], [4, 0, 9], [0, 2, 11]] and big == 11


# ---- the seed of the GPU distribution test ---------------------------------------------------------------------------
from augment_ref import DIST_B, DIST_N, DIST_SEED  # noqa: E402


def test_distribution_seed_meets_its_bounds_under_the_restatement():
    """Four standard errors: the mean and variance of the B * N * 3 normals, and every cloud's dropped fraction
    against its ratio (the binomial's standard error at that ratio)."""
    n = DIST_B * DIST_N * 3
    z = np.concatenate([ar.point_normals(DIST_SEED, 0, b, 0, DIST_N).ravel() for b in range(DIST_B)])
    assert abs(z.mean()) <= 4 / np.sqrt(n)
    assert abs(z.var() - 1) <= 4 * np.sqrt(2 / n)
    for b in range(DIST_B):
        ratio = ar.cloud_draw(DIST_SEED, 0, b, 1, ar.DROPOUT, (0.5,))[0]
        frac = 1 - ar.keep_mask(DIST_SEED, 0, b, 1, DIST_N, ratio).mean()
        assert abs(frac - ratio) <= 4 * np.sqrt(max(ratio * (1 - ratio), 1e-12) / DIST_N), (b, ratio, frac)
