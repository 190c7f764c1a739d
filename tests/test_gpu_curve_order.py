"""GPU: spectral.curve_order (csrc/curve_order.hip) against the numpy restatement of tests/curve_ref.py.  Every comparison
is exact integer equality, ``order`` and ``codes`` both: the cell is three correctly rounded float64 operations and the
rest is integer arithmetic, so there is no tolerance to state.  The curves themselves are pinned on the CPU
(tests/test_curve_ref.py); the lattice tests below repeat the unit-step walk on the kernel's own orders."""
import numpy as np
import pytest
import torch

import curve_ref as cr
from guarded_alloc import SENTINEL, ZERO, guarded, place, same_bits

pytestmark = pytest.mark.gpu

ALL = ("hilbert", "hilbert-trans", "z", "z-trans")
# one wave and its edges, the 64-lane floor of the workgroup, no power of two, a power of two, 1024 lanes with a padded
# network, the largest cloud (eight cells per lane, 64 KB of keys)
SIZES = [2, 3, 63, 64, 65, 128, 500, 512, 1025, 8192]


def run(c, device, **kw):
    from si_mamba_amd import spectral
    order, codes = spectral.curve_order(torch.from_numpy(np.ascontiguousarray(c)).to(device), return_codes=True, **kw)
    torch.cuda.synchronize()
    return order.cpu().numpy(), codes.cpu().numpy()


def check(c, device, curves=ALL, bits=10, box="cloud"):
    """order and codes equal the restatement; every order row is a permutation."""
    order, codes = run(c, device, curves=curves, bits=bits, box=box)
    want_order, want_codes = cr.order(c, curves, bits, box)
    assert order.dtype == np.int64 and order.shape == (c.shape[0], len(curves), c.shape[1]) == codes.shape
    np.testing.assert_array_equal(np.sort(order, axis=-1), np.broadcast_to(np.arange(c.shape[1]), order.shape))
    np.testing.assert_array_equal(codes, want_codes)
    np.testing.assert_array_equal(order, want_order)
    return order, codes


@pytest.mark.parametrize("b", [3, 4])
def test_full_lattice_fixed_box(device, b):
    """All 8^b cell centres of the lattice, shuffled: every code occurs once, the order is the restatement's, and the
    Hilbert orders walk from face neighbour to face neighbour starting at the origin."""
    side = 1 << b
    c, cell = cr.lattice_centers(side, np.random.default_rng(b))
    order, codes = check(c, device, ALL, b, (0, side))
    for k, name in enumerate(ALL):
        np.testing.assert_array_equal(np.sort(codes[0, k]), np.arange(8 ** b))
        if name.startswith("hilbert"):
            walk = cell[order[0, k]]
            assert (np.abs(np.diff(walk, axis=0)).sum(axis=1) == 1).all()
            np.testing.assert_array_equal(walk[0], [0, 0, 0])


@pytest.mark.parametrize("G", SIZES)
def test_random_clouds(device, G):
    """bits in {1, 10, 16} x k in {1, 4, 8} x B in {1, 5} x both boxes; the fixed box (-1, 1) leaves part of a normal
    cloud outside, where the cell is clamped."""
    rng = np.random.default_rng(G)
    clouds = {B: rng.standard_normal((B, G, 3)).astype(np.float32) for B in (1, 5)}
    n = 0
    for bits in (1, 10, 16):
        for k in (1, 4, 8):
            for B in (1, 5):
                for box in ("cloud", (-1, 1)):
                    curves = tuple(ALL[(n + i) % 4] for i in range(k))          # k = 1 visits every curve in turn
                    check(clouds[B], device, curves, bits, box)
                    n += 1


def test_ties_go_to_the_lower_index(device):
    rng = np.random.default_rng(7)
    c = rng.standard_normal((2, 512, 3)).astype(np.float32)
    order, codes = check(c, device, ALL, 1)                                     # at most 8 distinct codes
    assert len(np.unique(codes)) <= 8
    for b in range(2):
        for k in range(4):
            o = order[b, k]
            assert (np.diff(codes[b, k][o] * 512 + o) > 0).all()
    dup = c.copy()
    dup[:, 256:] = dup[:, :256][:, ::-1]                                        # every centre twice
    order, codes = check(dup, device, ALL, 16)
    np.testing.assert_array_equal(codes[:, :, 256:], codes[:, :, :256][:, :, ::-1])
    check(dup[:, :300], device, ALL, 10, (-2, 2))


def test_degenerate_clouds(device):
    same = np.full((2, 65, 3), -0.3, dtype=np.float32)
    order, codes = check(same, device)
    np.testing.assert_array_equal(order, np.broadcast_to(np.arange(65), order.shape))   # the identity
    assert not codes.any()
    rng = np.random.default_rng(11)
    flat = rng.standard_normal((3, 200, 3)).astype(np.float32)
    flat[0, :, 0] = 0.25                                                        # one axis of zero extent, each axis
    flat[1, :, 1] = -7.0
    flat[2, :, 2] = 0.0
    _, codes = check(flat, device, ALL, 10)
    assert (codes[0, 2] & int("100" * 10, 2) == 0).all()                        # Morton: no x bit set in cloud 0
    check(flat, device, ALL, 16, (-8, 8))
    line = np.zeros((1, 100, 3), dtype=np.float32)
    line[0, :, 1] = np.arange(100, dtype=np.float32)[::-1]                      # two axes of zero extent
    order, _ = check(line, device, ("z", "hilbert"), 16)
    np.testing.assert_array_equal(order[0, 0], np.arange(100)[::-1])


def test_subnormal_extent_and_overflowing_fixed_box(device):
    """The fp32 extent at the ends of its range.  A cloud a few subnormals wide: the extent is a subnormal fp32 and the
    float64 quotient still resolves the lattice.  A fixed box whose width overflows fp32: ext = inf, every cell 0, the
    order the identity."""
    tiny = np.float32(2.0 ** -149)
    rng = np.random.default_rng(37)
    c = (rng.integers(0, 1000, (2, 70, 3)).astype(np.float32) * tiny).astype(np.float32)
    assert 0 < float(c.max()) < 2.0 ** -126
    _, codes = check(c, device, ALL, 10)
    assert len(np.unique(codes[0, 2])) > 32                                     # not collapsed into one cell
    wide = rng.standard_normal((2, 70, 3)).astype(np.float32)
    order, codes = check(wide, device, ALL, 16, (-3e38, 3e38))
    assert not codes.any()
    np.testing.assert_array_equal(order, np.broadcast_to(np.arange(70), order.shape))
    with np.errstate(over="ignore"):
        huge = wide * np.float32(1e38)                                          # up to +-3.4e38: max - min is inf
    check(huge, device, ALL, 16)                                                # a cloud box whose extent overflows


def test_non_finite_coordinates_land_in_the_last_cell(device):
    rng = np.random.default_rng(13)
    c = rng.uniform(0, 1, (3, 130, 3)).astype(np.float32)
    c[0, 17, 0] = np.nan
    c[1, 99, 2] = np.inf
    c[2, 5] = (-np.inf, np.nan, np.inf)
    c[2, 0] = 0.0
    c[2, 1] = 1.0
    for box in ("cloud", (0, 1)):
        order, codes = check(c, device, ("z", "z-trans", "hilbert"), 4, box)
        # the box ignores them (check() holds the finite rows to the restatement) and the cell is 2^bits - 1 on the axis
        assert codes[0, 0, 17] & int("100" * 4, 2) == int("100" * 4, 2)
        assert codes[1, 0, 99] & int("001" * 4, 2) == int("001" * 4, 2)
        assert codes[2, 0, 5] == (1 << 12) - 1 and order[2, 0, -1] in (1, 5)
    every = np.full((1, 9, 3), np.nan, dtype=np.float32)                        # no finite coordinate at all
    order, codes = check(every, device, ("z",), 5)
    assert (codes == (1 << 15) - 1).all()
    np.testing.assert_array_equal(order[0, 0], np.arange(9))


def test_scaling_by_a_power_of_two_changes_no_bit(device):
    rng = np.random.default_rng(17)
    c = rng.standard_normal((4, 128, 3)).astype(np.float32)
    base = run(c, device, curves=ALL, bits=16)
    for e in (-3, 5):
        got = run(c * np.float32(2.0 ** e), device, curves=ALL, bits=16)
        np.testing.assert_array_equal(got[0], base[0])
        np.testing.assert_array_equal(got[1], base[1])


def test_trans_is_the_curve_on_swapped_axes(device):
    rng = np.random.default_rng(19)
    c = rng.standard_normal((3, 500, 3)).astype(np.float32)
    sw = np.ascontiguousarray(c[..., [1, 0, 2]])
    for box in ("cloud", (-1, 1)):
        a = run(c, device, curves=("hilbert-trans", "z-trans"), bits=10, box=box)
        b = run(sw, device, curves=("hilbert", "z"), bits=10, box=box)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])


def test_two_calls_give_the_same_bits_and_order_alone_equals_order_with_codes(device):
    from si_mamba_amd import spectral
    c = torch.from_numpy(np.random.default_rng(23).standard_normal((5, 1025, 3)).astype(np.float32)).to(device)
    a, ca = spectral.curve_order(c, return_codes=True)
    b, cb = spectral.curve_order(c, return_codes=True)
    alone = spectral.curve_order(c)
    assert torch.equal(a, b) and torch.equal(ca, cb) and torch.equal(a, alone)
    assert alone.dtype == torch.int64 and alone.device == c.device and not alone.requires_grad
    # the centres of a model carry a graph; the orders do not
    assert torch.equal(spectral.curve_order(c.clone().requires_grad_(True)), a)
    with pytest.raises(RuntimeError):
        spectral.curve_order(c, bits=17)


def test_graph_capture_and_replay_on_new_centres(device):
    from si_mamba_amd import spectral
    rng = np.random.default_rng(29)
    first = rng.standard_normal((4, 128, 3)).astype(np.float32)
    second = rng.standard_normal((4, 128, 3)).astype(np.float32)
    c = torch.from_numpy(first).to(device)
    spectral.curve_order(c, return_codes=True)                                  # the library is loaded before capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        order, codes = spectral.curve_order(c, return_codes=True)
    for data in (first, second):
        c.copy_(torch.from_numpy(data))
        graph.replay()
        torch.cuda.synchronize()
        want = cr.order(data)
        np.testing.assert_array_equal(order.cpu().numpy(), want[0])
        np.testing.assert_array_equal(codes.cpu().numpy(), want[1])


@pytest.mark.parametrize("with_codes", [False, True])
def test_memory_contract(device, with_codes):
    """G = 65, k = 3 in guard-banded, poisoned buffers: nothing is written outside order / codes, every word of them is
    written, and nothing around the centres is read."""
    from si_mamba_amd import spectral
    c = torch.from_numpy(np.random.default_rng(31).standard_normal((3, 65, 3)).astype(np.float32)).to(device)
    kw = dict(curves=("hilbert", "z-trans", "z"), bits=10, return_codes=with_codes)

    def outs(res):
        return res if with_codes else (res,)
    plain = outs(spectral.curve_order(c, **kw))
    got = []
    for poison in (ZERO, SENTINEL):
        with guarded(poison) as g:
            placed = place(c)
            n_in = len(g.records)
            res = outs(spectral.curve_order(placed, **kw))
            g.verify()
            assert len(g.records) - n_in == len(res) and "spectral.py" in g.modules
        got.append(res)
    for a, b, p in zip(got[0], got[1], plain):
        assert same_bits(a, b) and same_bits(a, p)
    want = cr.order(c.cpu().numpy(), kw["curves"], 10)
    for t, w in zip(plain, want):
        np.testing.assert_array_equal(t.cpu().numpy(), w)
