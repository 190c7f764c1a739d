"""CPU: simamba_cutmix_points, simamba_mix_draw and simamba_pointwolf_points (csrc/mix.hip) are declared, bound and
exported and refuse every bad argument, in the stated order, before a launch; the constants of the header, the binding
and the restatement agree and the key tweak differs from corrupt's; the Python package is exported and refuses what it
documents.  No device is touched here."""
import ctypes
import math
import re

import pytest
import torch

import corrupt_ref as cf
import mix_ref as mr
from abi_tables import E_NULLPTR, E_SHAPE, E_VARIANT, P, check_rows, declared_params, header_code
from si_mamba_amd import _lib, mixing

NAN, INF = float("nan"), float("inf")
NAMES = ("simamba_cutmix_points", "simamba_mix_draw", "simamba_pointwolf_points")
_KEEP = []


def par(*v):
    """A host array of four fp32 parameters, as the table passes it (kept alive by the module)."""
    arr = (ctypes.c_float * 4)(*v)
    _KEEP.append(arr)
    return arr


OUT = P + (1 << 26)         # far behind points: 4 x 8192 x 12 bytes fit in between
BYTES = 4 * 1024 * 12       # one (4, 1024, 3) fp32 batch
CUT = dict(points=P, lengths=None, partner=None, lam=None, out=OUT, ratio=P, src=None, state=P, mode=mr.CUT_K, B=4,
           N=1024, stream=None)
CUT_ROWS = [
    # shape
    (dict(B=0), E_SHAPE), (dict(B=-1), E_SHAPE), (dict(B=1 << 31), E_SHAPE), (dict(N=0), E_SHAPE), (dict(N=-1), E_SHAPE),
    (dict(N=8193), E_SHAPE),
    # null pointers; the limits of B and N pass the shape check and end at a null pointer, nothing launched
    (dict(points=None), E_NULLPTR), (dict(out=None), E_NULLPTR), (dict(ratio=None), E_NULLPTR),
    (dict(state=None), E_NULLPTR), (dict(N=1, state=None), E_NULLPTR), (dict(N=8192, state=None), E_NULLPTR),
    (dict(B=(1 << 31) - 1, out=None), E_NULLPTR), (dict(B=1, ratio=None), E_NULLPTR),
    (dict(lengths=P, partner=P, lam=P, src=P, state=None), E_NULLPTR), (dict(mode=mr.CUT_R, state=None), E_NULLPTR),
    # the mode
    (dict(mode=0), E_VARIANT), (dict(mode=3), E_VARIANT), (dict(mode=-1), E_VARIANT),
    # out over points: never, not even row for row
    (dict(out=P), E_VARIANT), (dict(out=P + 12), E_VARIANT), (dict(out=P + BYTES - 4), E_VARIANT),
    (dict(out=P - BYTES + 4), E_VARIANT), (dict(out=P + BYTES, state=None), E_NULLPTR),
    (dict(out=P - BYTES, state=None), E_NULLPTR),
    # two faults: the shape in front of the null pointer, the null pointer in front of the mode, the mode in front of
    # the overlap (either answer is E_VARIANT; the order shows in the rows above)
    (dict(N=0, points=None), E_SHAPE), (dict(B=0, mode=9), E_SHAPE), (dict(N=8193, out=P), E_SHAPE),
    (dict(mode=9, points=None), E_NULLPTR), (dict(out=P, ratio=None), E_NULLPTR), (dict(mode=9, out=P), E_VARIANT),
]

DRAW = dict(partner=P, lam=P, state=P, B=4, stream=None)
DRAW_ROWS = [
    (dict(B=0), E_SHAPE), (dict(B=-1), E_SHAPE), (dict(B=1 << 31), E_SHAPE),
    (dict(state=None), E_NULLPTR), (dict(partner=None, lam=None), E_NULLPTR),
    (dict(partner=None, state=None), E_NULLPTR), (dict(lam=None, state=None), E_NULLPTR),
    (dict(B=0, state=None), E_SHAPE),
]

GOOD = (0.5, math.radians(10), 3.0, 0.25)
WOLF = dict(points=P, lengths=None, out=OUT, anchors_out=None, state=P, M=4, params=par(*GOOD), flags=0, B=4, N=1024,
            stream=None)


def wolf(sigma=GOOD[0], rot=GOOD[1], scale=GOOD[2], trans=GOOD[3], **more):
    return dict(params=par(sigma, rot, scale, trans), **more)


WOLF_ROWS = [
    # shape
    (dict(B=0), E_SHAPE), (dict(B=-1), E_SHAPE), (dict(B=1 << 31), E_SHAPE), (dict(N=0), E_SHAPE), (dict(N=8193), E_SHAPE),
    (dict(M=0), E_SHAPE), (dict(M=9), E_SHAPE), (dict(M=-1), E_SHAPE),
    # null pointers; the limits pass the shape check
    (dict(points=None), E_NULLPTR), (dict(out=None), E_NULLPTR), (dict(state=None), E_NULLPTR),
    (dict(params=None), E_NULLPTR), (dict(M=1, N=1, state=None), E_NULLPTR), (dict(M=8, N=8192, state=None), E_NULLPTR),
    (dict(B=(1 << 31) - 1, out=None), E_NULLPTR), (dict(lengths=P, anchors_out=P, state=None), E_NULLPTR),
    # accepted parameters reach the null pointer
    *[(wolf(state=None, flags=f, **kw), E_NULLPTR)
      for kw in (dict(), dict(rot=0.0), dict(scale=1.0), dict(trans=0.0), dict(sigma=1e-3), dict(sigma=1e6))
      for f in (0, mr.WOLF_RENORM)],
    # the flags and the parameters
    (dict(flags=2), E_VARIANT), (dict(flags=3), E_VARIANT), (dict(flags=-1), E_VARIANT),
    (wolf(sigma=0.0), E_VARIANT), (wolf(sigma=-0.5), E_VARIANT), (wolf(sigma=NAN), E_VARIANT),
    (wolf(sigma=1e-30), E_VARIANT),                               # 1 / (2 sigma^2) is not a finite fp32
    (wolf(sigma=INF), E_VARIANT), (wolf(rot=-0.1), E_VARIANT),
    (wolf(rot=NAN), E_VARIANT), (wolf(rot=INF), E_VARIANT),
    (wolf(scale=0.5), E_VARIANT), (wolf(scale=NAN), E_VARIANT), (wolf(scale=INF), E_VARIANT),
    (wolf(trans=-0.1), E_VARIANT), (wolf(trans=NAN), E_VARIANT), (wolf(trans=INF), E_VARIANT),
    # out may be points itself; any other overlap is refused
    (dict(out=P, state=None), E_NULLPTR), (dict(out=P + 12), E_VARIANT), (dict(out=P + BYTES - 4), E_VARIANT),
    (dict(out=P - BYTES + 4), E_VARIANT), (dict(out=P + BYTES, state=None), E_NULLPTR),
    # two faults: shape, null pointer, variant, overlap
    (dict(M=0, points=None), E_SHAPE), (dict(N=0, flags=2), E_SHAPE), (dict(flags=2, state=None), E_NULLPTR),
    (dict(params=None, out=P + 12), E_NULLPTR),
    (wolf(sigma=0.0, out=P + 12), E_VARIANT), (wolf(scale=0.5, state=None), E_NULLPTR),
]


def test_symbols_are_declared_bound_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared_params() and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert declared_params()[name][-1] == "void* stream"
        assert not any(re.match(r"(const\s+)?double\b", p) for p in declared_params()[name])
        assert len(_lib.SIGNATURES[name][1]) == len(declared_params()[name])
    assert set(declared_params()) == set(_lib.SIGNATURES)
    assert _lib.load().simamba_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert re.search(r"#define\s+SIMAMBA_ABI_VERSION\s+9\b", header_code())
    names = [re.search(r"(\w+)$", p).group(1) for p in declared_params()["simamba_cutmix_points"]]
    assert names == ["points", "lengths", "partner", "lam", "out", "ratio", "src", "state", "mode", "B", "N", "stream"]
    names = [re.search(r"(\w+)$", p).group(1) for p in declared_params()["simamba_pointwolf_points"]]
    assert names == ["points", "lengths", "out", "anchors_out", "state", "M", "params", "flags", "B", "N", "stream"]


def test_return_codes_without_a_device():
    check_rows("simamba_cutmix_points", CUT, CUT_ROWS)
    check_rows("simamba_mix_draw", DRAW, DRAW_ROWS)
    check_rows("simamba_pointwolf_points", WOLF, WOLF_ROWS)


def test_constants_agree_and_the_tweaks_are_distinct():
    code = header_code()
    header = {k: int(v.rstrip("u"), 0) for k, v in
              re.findall(r"#define\s+SIMAMBA_((?:MIX|WOLF)_[A-Z_0-9]+)\s+(0x[0-9A-Fa-f]+u?|\d+)", code)}
    assert header == dict(MIX_CUT_R=1, MIX_CUT_K=2, MIX_KEY_TWEAK=0x4D495847, WOLF_RENORM=1, WOLF_MAX_ANCHORS=8)
    for k, v in header.items():
        assert getattr(_lib, k) == v
    assert (mr.CUT_R, mr.CUT_K, mr.KEY_TWEAK, mr.WOLF_RENORM, mr.MAX_ANCHORS) == (1, 2, 0x4D495847, 1, 8)
    assert mixing.MODES == {"r": mr.CUT_R, "k": mr.CUT_K} == mr.MODE
    tweaks = {k: int(v, 0) for k, v in re.findall(r"#define\s+SIMAMBA_([A-Z]+)_KEY_TWEAK\s+(0x[0-9A-Fa-f]+)", code)}
    assert set(tweaks) == {"CORRUPT", "MIX"} and len(set(tweaks.values())) == 2 and 0 not in tweaks.values()
    assert tweaks["CORRUPT"] == cf.KEY_TWEAK == _lib.CORRUPT_KEY_TWEAK and tweaks["MIX"] == _lib.MIX_KEY_TWEAK


def test_package_is_exported():
    import si_mamba_amd as sm
    for name in ("mixing", "cutmix", "pointwolf", "mixup", "mixed_cross_entropy"):
        assert hasattr(sm, name) and name in sm.__all__, name
    assert sm.cutmix is mixing.cutmix and sm.mixing.__file__.endswith("__init__.py")
    for name in ("cutmix", "pointwolf", "mixup", "mixed_cross_entropy", "draw_pairs"):
        assert name in mixing.__all__


def test_python_route_refuses_cpu_tensors_and_bad_arguments():
    pc = torch.zeros(2, 16, 3)
    for call in (lambda: mixing.cutmix(pc), lambda: mixing.cutmix(pc, "r"), lambda: mixing.pointwolf(pc),
                 lambda: mixing.mixup(pc)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for bad in (torch.zeros(2, 16, 4), torch.zeros(16, 3)):
        for fn in (mixing.cutmix, mixing.pointwolf, mixing.mixup):
            with pytest.raises(ValueError):
                fn(bad)


def test_mixed_cross_entropy_is_the_two_term_formula():
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(6, 5, generator=g, dtype=torch.float64, requires_grad=True)
    labels = torch.randint(0, 5, (6,), generator=g)
    partner = torch.randperm(6, generator=g)
    ratio = torch.rand(6, generator=g, dtype=torch.float64)
    ratio[0], ratio[1] = 0.0, 1.0
    logp = torch.log_softmax(logits, -1)
    rows = torch.arange(6)
    want = -((1 - ratio) * logp[rows, labels] + ratio * logp[rows, labels[partner]])
    for red, w in (("none", want), ("sum", want.sum()), ("mean", want.mean())):
        got = mixing.mixed_cross_entropy(logits, labels, partner, ratio, reduction=red)
        assert torch.allclose(got, w, rtol=1e-12, atol=1e-12), red
    got = mixing.mixed_cross_entropy(logits, labels, partner, ratio)
    g1, = torch.autograd.grad(got, logits)
    g2, = torch.autograd.grad(want.mean(), logits)
    assert torch.allclose(g1, g2, rtol=1e-12, atol=1e-12)
    # ratio 0: the plain loss; ratio 1: the partner's
    plain = torch.nn.functional.cross_entropy(logits, labels, reduction="none")
    assert torch.allclose(mixing.mixed_cross_entropy(logits, labels, partner, torch.zeros(6), "none"), plain)
    with pytest.raises(ValueError):
        mixing.mixed_cross_entropy(logits, labels, partner, ratio, reduction="max")
    with pytest.raises(ValueError):
        mixing.mixed_cross_entropy(logits, labels[:5], partner, ratio)
