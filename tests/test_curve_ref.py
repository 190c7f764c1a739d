"""CPU: the curves of tests/curve_ref.py pinned independently of the kernel.  On the full lattice of side 2^b a Hilbert
curve visits every cell once, moves to a face neighbour at every step and starts at the origin; a Morton code is the
bit-by-bit interleave.  The kernel is then held to curve_ref exactly (tests/test_gpu_curve_order.py)."""
import numpy as np
import pytest

import curve_ref as cr

BITS = [1, 2, 3, 4]


@pytest.mark.parametrize("b", BITS)
def test_hilbert_is_a_bijection_onto_the_code_range(b):
    cell = cr.lattice(1 << b)
    code = cr.hilbert(cell[:, 0], cell[:, 1], cell[:, 2], b)
    np.testing.assert_array_equal(np.sort(code), np.arange(8 ** b))


@pytest.mark.parametrize("b", BITS)
def test_consecutive_hilbert_codes_are_face_neighbours(b):
    cell = cr.lattice(1 << b)
    for axes in ((0, 1, 2), (1, 0, 2)):                                   # the curve and its "-trans" form
        code = cr.hilbert(cell[:, axes[0]], cell[:, axes[1]], cell[:, axes[2]], b)
        walk = cell[np.argsort(code)]
        np.testing.assert_array_equal(np.abs(np.diff(walk, axis=0)).sum(axis=1), np.ones(8 ** b - 1, dtype=np.int64))
        np.testing.assert_array_equal(walk[0], [0, 0, 0])


@pytest.mark.parametrize("b", BITS)
def test_morton_is_the_bit_interleave(b):
    cell = cr.lattice(1 << b)
    code = cr.morton(cell[:, 0], cell[:, 1], cell[:, 2], b)
    for (x, y, z), c in zip(cell.tolist(), code.tolist()):
        want = "".join(format(x, f"0{b}b")[i] + format(y, f"0{b}b")[i] + format(z, f"0{b}b")[i] for i in range(b))
        assert c == int(want, 2), (x, y, z)
    np.testing.assert_array_equal(np.sort(code), np.arange(8 ** b))


def test_morton_and_hilbert_at_sixteen_bits_stay_inside_48_bits():
    top = (1 << 16) - 1
    assert cr.morton(top, top, top, 16) == (1 << 48) - 1
    assert cr.morton(top, 0, 0, 16) == int("100" * 16, 2) and cr.morton(0, 0, top, 16) == int("001" * 16, 2)
    rng = np.random.default_rng(0)
    q = rng.integers(0, 1 << 16, (4096, 3))
    h = cr.hilbert(q[:, 0], q[:, 1], q[:, 2], 16)
    assert h.min() >= 0 and h.max() < 1 << 48 and len(np.unique(h)) == len(np.unique(q, axis=0))
    assert cr.hilbert(0, 0, 0, 16) == 0


def test_cells_follow_the_definition():
    c = np.array([[[0.0, 0.0, 0.0], [1.0, 0.5, 0.25], [0.5, 0.5, np.nan], [np.inf, 0.25, 0.0]]], dtype=np.float32)
    # cloud box: lo = (0, 0, 0), ext = 1 over the finite coordinates; the maximum lands in the last cell (clamped)
    np.testing.assert_array_equal(cr.cells(c, 2)[0], [[0, 0, 0], [3, 2, 1], [2, 2, 3], [3, 1, 0]])
    # fixed box (-1, 1): q = floor((x + 1) / 2 * 4), outside the box clamped
    np.testing.assert_array_equal(cr.cells(c, 2, (-1, 1))[0], [[2, 2, 2], [3, 3, 2], [3, 3, 3], [3, 2, 2]])
    np.testing.assert_array_equal(cr.cells(c - 5, 2, (-1, 1))[0][:2], [[0, 0, 0], [0, 0, 0]])
    # zero extent: every finite coordinate in cell 0
    same = np.full((1, 5, 3), 0.7, dtype=np.float32)
    assert not cr.cells(same, 10).any()
    order, codes = cr.order(same, bits=10)
    np.testing.assert_array_equal(order, np.broadcast_to(np.arange(5), (1, 4, 5)))
    assert not codes.any()


def test_order_is_stable_and_trans_swaps_the_first_two_axes():
    rng = np.random.default_rng(1)
    c = rng.standard_normal((3, 200, 3)).astype(np.float32)
    order, codes = cr.order(c, bits=1)
    assert len(np.unique(codes)) <= 8
    for b in range(3):
        for k in range(4):
            o = order[b, k]
            key = codes[b, k][o] * 200 + o
            assert (np.diff(key) > 0).all()
    sw = c[..., [1, 0, 2]]
    np.testing.assert_array_equal(cr.order(c, ("hilbert-trans", "z-trans"), 7, (-4, 4))[0],
                                  cr.order(sw, ("hilbert", "z"), 7, (-4, 4))[0])
