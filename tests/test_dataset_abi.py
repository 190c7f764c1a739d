"""CPU: the keyed bijection of csrc/keyed_perm.h through its host entry point against the numpy restatement of
dataset_ref.py, and the argument checks of simamba_dataset_fetch (csrc/dataset.hip), which all come before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dataset_ref as dr
from abi_tables import E_NULLPTR, E_SHAPE, E_VARIANT, P, check_rows, declared_params, header_code
from conftest import ROOT
from si_mamba_amd import _lib

SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 1000, 9843, 52470, (1 << 20) + 1]
SEEDS = [0, 0xa4093822299f31d0, 20240607]                                   # the second: both key words in use
STREAMS = [dr.stream(dr.STREAM_SHUFFLE, 0, 0), dr.stream(dr.STREAM_ROWS, (1 << 29) - 1, (1 << 31) - 1)]
WHOLE = 1 << 16                                                             # up to here the whole range is compared


def i64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= 1 << 63 else v


def lib_perm(n, seed, stream, first=0, count=None):
    count = n - first if count is None else count
    out = np.full(max(count, 1), -7, dtype=np.int64)
    rc = _lib.load().simamba_keyed_perm(i64(seed), i64(stream), n, first, count, out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, rc
    return out[:count]


@pytest.mark.parametrize("n", SIZES)
def test_keyed_perm_equals_the_restatement(n):
    """Element for element.  Above 2^16 the restatement is computed for the first and last 4096 positions and 4096
    random ones (numpy needs seconds for a million ten-round Philox blocks per network application); the library's
    whole range is checked to be a permutation below."""
    for seed in SEEDS:
        for stream in STREAMS:
            if n <= WHOLE:
                np.testing.assert_array_equal(lib_perm(n, seed, stream), dr.perm(n, seed, stream, np.arange(n)))
                continue
            whole = lib_perm(n, seed, stream)
            at = np.unique(np.concatenate([np.arange(4096), np.arange(n - 4096, n),
                                           np.random.default_rng(n).integers(0, n, 4096)]))
            np.testing.assert_array_equal(whole[at], dr.perm(n, seed, stream, at))
            np.testing.assert_array_equal(lib_perm(n, seed, stream, n - 4096, 4096), whole[-4096:])


@pytest.mark.parametrize("n", SIZES)
def test_keyed_perm_is_a_permutation(n):
    for seed in SEEDS:
        for stream in STREAMS:
            np.testing.assert_array_equal(np.sort(lib_perm(n, seed, stream)), np.arange(n))


@pytest.mark.parametrize("n", [s for s in SIZES if s >= 64])
def test_streams_and_seeds_give_different_orders(n):
    a, b = (lib_perm(n, SEEDS[1], s) for s in STREAMS)
    c = lib_perm(n, SEEDS[2], STREAMS[0])
    d = lib_perm(n, SEEDS[1], dr.stream(dr.STREAM_SHUFFLE, 1, 0))              # the next epoch
    for x, y in ((a, b), (a, c), (a, d), (b, d)):
        # two independent uniform orders agree at about one position; a quarter of them would be a broken key
        assert (x == y).sum() < n // 4
    assert not np.array_equal(a, np.arange(n))


def test_keyed_perm_ranges_and_refusals():
    fn = _lib.load().simamba_keyed_perm
    buf = np.zeros(8, dtype=np.int64)
    out = buf.ctypes.data_as(ctypes.c_void_p)
    whole = lib_perm(1000, 5, 9)
    np.testing.assert_array_equal(lib_perm(1000, 5, 9, 993, 7), whole[993:])
    assert lib_perm(1000, 5, 9, 1000, 0).size == 0
    assert fn(5, 9, 0, 0, 0, out) == E_SHAPE and fn(5, 9, 1 << 31, 0, 1, out) == E_SHAPE
    assert fn(5, 9, 10, -1, 1, out) == E_SHAPE and fn(5, 9, 10, 0, -1, out) == E_SHAPE
    assert fn(5, 9, 10, 8, 3, out) == E_SHAPE and fn(5, 9, 10, 11, 0, out) == E_SHAPE
    assert fn(5, 9, 10, 0, 1, None) == E_NULLPTR and fn(5, 9, 10, 0, 0, None) == 0
    assert fn(5, 9, (1 << 31) - 1, (1 << 31) - 9, 8, out) == 0                # the largest n: 32-bit network
    assert ((0 <= buf) & (buf < (1 << 31) - 1)).all() and len(set(buf.tolist())) == 8
    np.testing.assert_array_equal(buf, dr.perm((1 << 31) - 1, 5, 9, np.arange((1 << 31) - 9, (1 << 31) - 1)))


def test_restatement_layout():
    """The network's size and the stream layout are what include/simamba.h states."""
    assert [dr.half_bits(n) for n in (2, 3, 4, 5, 16, 17, 64, 65, 1 << 20, (1 << 20) + 1, (1 << 31) - 1)] == \
        [1, 1, 1, 2, 2, 3, 3, 4, 10, 11, 16]
    for n in SIZES[1:]:
        assert n <= 1 << (2 * dr.half_bits(n)) < 4 * n
    assert dr.stream(dr.STREAM_CHOICE, (1 << 29) + 5, 77) == (3 << 60) | (5 << 31) | 77
    assert len({dr.stream(u, e, p) for u in (1, 2, 3) for e in (0, 1) for p in (0, 1)}) == 12
    # slot b of a batch of 6 is slot b % 3 of step b // 3 of a batch of 3; three ranks interleave
    a = dr.slot_samples(100, 6, 3, 0, 16)[0]
    b = np.concatenate([dr.slot_samples(100, 3, 3, k, 33)[0] for k in (0, 1)])
    np.testing.assert_array_equal(a, b)
    ranks = np.stack([dr.slot_samples(100, 2, 3, 0, 16, rank=r, world=3)[0] for r in range(3)], 1).ravel()
    np.testing.assert_array_equal(ranks, a)
    # choice stays inside the candidates and uses them all
    rows = dr.slot_rows(100, 4096, 37, dr.CHOICE, 3, 0, 5)
    assert rows.min() == 0 and rows.max() == 36 and len(rows) == 4096
    rows = dr.slot_rows(100, 64, 37, dr.PERMUTE, 3, 0, 5)
    assert len(set(rows.tolist())) == 37 and rows.max() == 36


# ---- simamba_dataset_fetch: every refusal before a launch, in the documented order -----------------------------------
FETCH = dict(points=P, offsets=None, labels=P, point_labels=P, state=P, out=P, label_out=P, point_label_out=P,
             index_out=P, lengths_out=P, total=100 * 2048, S=100, stride=2048, B=4, K=1024, first=0, steps_per_epoch=25,
             rank=0, world=1, order=1, rows=1, norm=1, stream=None)
FETCH_ROWS = [
    # shape
    (dict(S=0), E_SHAPE), (dict(S=1 << 31), E_SHAPE), (dict(B=0), E_SHAPE), (dict(B=1 << 31), E_SHAPE),
    (dict(K=0), E_SHAPE), (dict(K=8193), E_SHAPE), (dict(K=-1), E_SHAPE),
    (dict(rank=-1), E_SHAPE), (dict(rank=1), E_SHAPE), (dict(world=0), E_SHAPE), (dict(rank=3, world=3), E_SHAPE),
    (dict(steps_per_epoch=0), E_SHAPE), (dict(first=-1), E_SHAPE), (dict(total=-1), E_SHAPE),
    (dict(stride=0), E_SHAPE), (dict(stride=2049), E_SHAPE), (dict(total=100 * 2048 - 1), E_SHAPE),
    (dict(steps_per_epoch=1 << 40, B=1 << 20, world=8), E_SHAPE),             # a slot's position would pass 2^62
    # null pointers; the limits pass the shape check and end at a null pointer, nothing launched
    (dict(points=None), E_NULLPTR), (dict(state=None), E_NULLPTR), (dict(out=None), E_NULLPTR),
    (dict(index_out=None), E_NULLPTR), (dict(lengths_out=None), E_NULLPTR),
    (dict(K=1, state=None), E_NULLPTR), (dict(K=8192, state=None), E_NULLPTR),
    (dict(S=(1 << 31) - 1, stride=1, total=1 << 31, state=None), E_NULLPTR),
    (dict(B=(1 << 31) - 1, out=None), E_NULLPTR), (dict(rank=2, world=3, out=None), E_NULLPTR),
    (dict(offsets=P, stride=0, total=0, state=None), E_NULLPTR),              # ragged: stride is not looked at
    (dict(steps_per_epoch=1 << 40, B=1 << 20, world=4, out=None), E_NULLPTR),   # exactly 2^62
    (dict(labels=None, point_labels=None, label_out=None, point_label_out=None, state=None), E_NULLPTR),
    # modes
    (dict(order=2), E_VARIANT), (dict(order=-1), E_VARIANT), (dict(rows=3), E_VARIANT), (dict(rows=-1), E_VARIANT),
    (dict(norm=2), E_VARIANT), (dict(norm=-1), E_VARIANT),
    # two faults: the shape in front of the null pointer, the null pointer in front of the mode
    (dict(K=0, points=None), E_SHAPE), (dict(S=0, rows=3), E_SHAPE), (dict(stride=0, out=None), E_SHAPE),
    (dict(rank=1, norm=2), E_SHAPE), (dict(state=None, order=2), E_NULLPTR), (dict(lengths_out=None, norm=2), E_NULLPTR),
]


def test_fetch_return_codes_without_a_device():
    check_rows("simamba_dataset_fetch", FETCH, FETCH_ROWS)


def test_symbols_and_modes_bound():
    declared = set(declared_params())
    assert declared == set(_lib.SIGNATURES)
    assert {"simamba_dataset_fetch", "simamba_keyed_perm"} <= declared
    header = {k: int(v) for k, v in re.findall(r"#define SIMAMBA_DS_([A-Z_]+)\s+(\d+)", header_code())}
    assert header == dict(SEQUENTIAL=0, SHUFFLE=1, FIRST=0, PERMUTE=1, CHOICE=2, NONE=0, UNIT_SPHERE=1,
                          STREAM_SHUFFLE=1, STREAM_ROWS=2, STREAM_CHOICE=3)
    for k, v in header.items():
        assert getattr(_lib, "DS_" + k) == v and getattr(dr, k) == v


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "si_mamba_amd")
    seen = 0
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                seen += f == "data.py"
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
    assert seen == 1


def test_python_route_refuses_the_cpu_and_bad_arguments():
    import si_mamba_amd as sm
    from si_mamba_amd import data
    assert sm.DeviceDataset is data.DeviceDataset and sm.DeviceLoader is data.DeviceLoader and sm.Batch is data.Batch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.DeviceDataset.from_arrays(np.zeros((4, 8, 3), np.float32), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.DeviceDataset.from_arrays([torch.zeros(5, 3)], device=torch.device("cpu"))
    with pytest.raises(TypeError):
        data.DeviceLoader(np.zeros((4, 8, 3)), 2, 8)
    # the loader's own arithmetic, on a store that never reaches a device
    store = data.DeviceDataset(torch.zeros(10 * 8, 3), None, 8, None, None)
    assert len(store) == 10 and store.nbytes == 10 * 8 * 12
    for kw in (dict(subsample="fps"), dict(normalize="unit"), dict(npoints=0), dict(npoints=8193), dict(batch_size=0),
               dict(rank=2, world=2), dict(first=-1), dict(batch_size=11), dict(batch_size=4, world=3)):
        with pytest.raises(ValueError):
            data.DeviceLoader(store, **{**dict(batch_size=2, npoints=8), **kw})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.DeviceLoader(store, 2, 8)                                         # its state would live on the CPU
    np.testing.assert_array_equal(data.keyed_perm(1000, SEEDS[1], STREAMS[1]), dr.perm(1000, SEEDS[1], STREAMS[1],
                                                                                      np.arange(1000)))
    np.testing.assert_array_equal(data.keyed_perm(1000, 5, 9, 10, 3), lib_perm(1000, 5, 9)[10:13])
