"""CPU: the entry points of csrc/bn_relu.hip -- the fused simamba_bn_relu_fwd / _bwd, the stages nn.SyncBatchNorm's
cross-rank statistics run between collectives, and the group max -- validate their arguments before any launch, all with
the same codes in the same order: dtype (-3), empty problem (0), shape (-2), null pointers (-1).

Every row states what it changes in a call that would otherwise be accepted, and the code the library answers; rows
with two faults pin the order of the checks.  P is an address that is never dereferenced: no row reaches a launch."""
from abi_tables import E_DTYPE, E_NULLPTR, E_SHAPE, OK, P, check_rows
from si_mamba_amd import _lib

_STATS = dict(x=P, gterm=None, group=0, stats=P, stats_ld=0, partial=P, rows=64, C=8, ld=0, io_dtype=0, stream=None)
_MERGE = dict(stats=P, world=2, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, mean=P, invstd=P,
              count=P, C=8, stream=None)
_APPLY = dict(x=P, gterm=None, group=0, weight=None, bias=None, mean=P, invstd=P, y=P, rows=64, C=8, ld=0,
              io_dtype=0, stream=None)
_SUMS = dict(dy=P, x=P, gterm=None, group=0, weight=None, bias=None, mean=P, invstd=P, dweight=P, dbias=P, partial=P,
             rows=64, C=8, ld=0, io_dtype=0, stream=None)
_DX = dict(dy=P, x=P, gterm=None, group=0, weight=None, bias=None, mean=P, invstd=P, sum_dweight=P, sum_dbias=P,
           count=P, dx=P, dgterm=None, dgroup=0, rows=64, C=8, ld=0, io_dtype=0, stream=None)
_FWD = dict(x=P, gterm=None, group=0, weight=None, bias=None, running_mean=None, running_var=None, momentum=0.1,
            eps=1e-5, training=1, y=P, mean=P, invstd=P, partial=P, rows=64, C=8, ld=0, io_dtype=0, stream=None)
_BWD = dict(dy=P, x=P, gterm=None, group=0, weight=None, bias=None, mean=P, invstd=P, dx=P, dgterm=None, dgroup=0,
            dweight=P, dbias=P, partial=P, rows=64, C=8, ld=0, io_dtype=0, training=1, stream=None)
_GMAX_FWD = dict(x=P, out=P, idx=P, groups=4, n=32, C=8, io_dtype=0, stream=None)
_GMAX_BWD = dict(dout=P, idx=P, dx=P, groups=4, n=32, C=8, io_dtype=0, stream=None)

# what the six entry points that walk (rows, C) activations share
_COMMON = [
    (dict(io_dtype=7), E_DTYPE), (dict(io_dtype=-1), E_DTYPE),
    (dict(rows=0), OK), (dict(rows=0, x=None), OK), (dict(rows=0, C=6), OK),              # empty: nothing to check
    (dict(C=6), E_SHAPE), (dict(C=0), E_SHAPE), (dict(C=1028), E_SHAPE), (dict(rows=-1), E_SHAPE),
    (dict(ld=4), E_SHAPE), (dict(ld=10), E_SHAPE),                                        # ld < C, ld % 4
    (dict(gterm=P, group=7), E_SHAPE), (dict(gterm=P, group=0), E_SHAPE), (dict(gterm=P, group=128), E_SHAPE),
    (dict(x=None), E_NULLPTR),
    # two faults: dtype, empty, shape, pointers
    (dict(io_dtype=7, rows=0), E_DTYPE), (dict(io_dtype=7, C=6), E_DTYPE), (dict(C=6, x=None), E_SHAPE),
    (dict(gterm=P, group=7, x=None), E_SHAPE),
]

# ... and the two directions of the group max
_GMAX = [
    (dict(io_dtype=7), E_DTYPE), (dict(io_dtype=-1), E_DTYPE),
    (dict(groups=0), OK), (dict(groups=0, C=6), OK),
    (dict(groups=-1), E_SHAPE), (dict(n=0), E_SHAPE), (dict(n=257), E_SHAPE), (dict(C=0), E_SHAPE), (dict(C=6), E_SHAPE),
    (dict(idx=None), E_NULLPTR),
    # a grid of more than 2^31 - 1 workgroups is refused, after the pointers, not truncated
    (dict(groups=1 << 42), E_SHAPE), (dict(groups=1 << 42, idx=None), E_NULLPTR),
    (dict(io_dtype=7, groups=0), E_DTYPE), (dict(io_dtype=7, C=6), E_DTYPE), (dict(C=6, idx=None), E_SHAPE),
]

ROWS = [
    ("simamba_bn_stats_local", _STATS, _COMMON + [
        (dict(stats=None), E_NULLPTR), (dict(partial=None), E_NULLPTR),
        (dict(stats_ld=4), E_SHAPE), (dict(stats_ld=4, stats=None), E_SHAPE),             # row stride of the (3, C) block
    ]),
    ("simamba_bn_stats_merge", _MERGE, [
        (dict(world=0), E_SHAPE), (dict(world=-3), E_SHAPE), (dict(C=-4), E_SHAPE),
        (dict(C=0), OK), (dict(C=0, world=0, stats=None), OK),                            # empty
        (dict(stats=None), E_NULLPTR), (dict(mean=None), E_NULLPTR), (dict(invstd=None), E_NULLPTR),
        (dict(count=None), E_NULLPTR),
        (dict(world=0, stats=None), E_SHAPE),
    ]),
    ("simamba_bn_relu_apply", _APPLY, _COMMON + [
        (dict(y=None), E_NULLPTR), (dict(mean=None), E_NULLPTR), (dict(invstd=None), E_NULLPTR),
    ]),
    ("simamba_bn_relu_bwd_sums", _SUMS, _COMMON + [
        (dict(dy=None), E_NULLPTR), (dict(mean=None), E_NULLPTR), (dict(invstd=None), E_NULLPTR),
        (dict(dweight=None), E_NULLPTR), (dict(dbias=None), E_NULLPTR), (dict(partial=None), E_NULLPTR),
    ]),
    ("simamba_bn_relu_bwd_dx", _DX, _COMMON + [
        (dict(dy=None), E_NULLPTR), (dict(dx=None), E_NULLPTR), (dict(mean=None), E_NULLPTR),
        (dict(invstd=None), E_NULLPTR), (dict(sum_dweight=None), E_NULLPTR), (dict(sum_dbias=None), E_NULLPTR),
        (dict(count=None), E_NULLPTR),
        # the per-group sums of dx: dgroup divides 256 and the rows, and needs the term it is the gradient of
        (dict(gterm=P, group=32, dgterm=P, dgroup=0), E_SHAPE), (dict(gterm=P, group=32, dgterm=P, dgroup=48), E_SHAPE),
        (dict(gterm=P, group=64, dgterm=P, dgroup=128), E_SHAPE),                         # 64 rows % 128
        (dict(dgterm=P, dgroup=32), E_NULLPTR),
        (dict(gterm=P, group=32, dgterm=P, dgroup=48, dy=None), E_SHAPE),
    ]),
    ("simamba_bn_relu_fwd", _FWD, _COMMON + [
        (dict(y=None), E_NULLPTR), (dict(mean=None), E_NULLPTR), (dict(invstd=None), E_NULLPTR),
        (dict(partial=None), E_NULLPTR),                                                  # batch statistics need it
        (dict(training=0), E_NULLPTR), (dict(training=0, running_mean=P), E_NULLPTR),     # eval: the running ones
        (dict(training=0, running_var=P), E_NULLPTR),
        (dict(C=6, partial=None), E_SHAPE), (dict(io_dtype=7, training=0), E_DTYPE), (dict(rows=0, training=0), OK),
    ]),
    ("simamba_bn_relu_bwd", _BWD, _COMMON + [
        (dict(dy=None), E_NULLPTR), (dict(dx=None), E_NULLPTR), (dict(mean=None), E_NULLPTR),
        (dict(invstd=None), E_NULLPTR), (dict(dweight=None), E_NULLPTR), (dict(dbias=None), E_NULLPTR),
        (dict(partial=None), E_NULLPTR),
        (dict(gterm=P, group=32, dgterm=P, dgroup=0), E_SHAPE), (dict(gterm=P, group=32, dgterm=P, dgroup=48), E_SHAPE),
        (dict(gterm=P, group=64, dgterm=P, dgroup=128), E_SHAPE),
        (dict(dgterm=P, dgroup=32), E_NULLPTR),
        (dict(gterm=P, group=32, dgterm=P, dgroup=48, dy=None), E_SHAPE), (dict(dgterm=P, dgroup=48), E_SHAPE),
        (dict(C=6, dgterm=P, dgroup=32), E_SHAPE),
    ]),
    ("simamba_group_max_fwd", _GMAX_FWD, _GMAX + [
        (dict(x=None), E_NULLPTR), (dict(out=None), E_NULLPTR), (dict(groups=0, x=None), OK),
        (dict(n=0, x=None), E_SHAPE),
    ]),
    ("simamba_group_max_bwd", _GMAX_BWD, _GMAX + [
        (dict(dout=None), E_NULLPTR), (dict(dx=None), E_NULLPTR), (dict(groups=0, dx=None), OK),
        (dict(n=0, dx=None), E_SHAPE),
    ]),
]


def test_staged_symbols_are_bound():
    for name, base, _ in ROWS:
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len(base), name


def test_staged_argument_validation_precedes_any_launch():
    for name, base, rows in ROWS:
        check_rows(name, base, rows)


def test_sync_bn_relu_fn_refuses_what_it_cannot_do():
    import pytest
    import torch
    from si_mamba_amd.encoder_ops import bn_relu_fn, sync_bn_relu_fn
    bn = torch.nn.SyncBatchNorm(8)
    with pytest.raises(ValueError, match="holds 0 rows"):
        sync_bn_relu_fn(torch.zeros(0, 8), bn)
    with pytest.raises(RuntimeError, match="no initialised process group"):
        sync_bn_relu_fn(torch.zeros(4, 8), bn)
    with pytest.raises(TypeError, match="LayerNorm"):
        sync_bn_relu_fn(torch.zeros(4, 8), torch.nn.LayerNorm(8))
    assert int(bn.num_batches_tracked) == 0                        # a refused call leaves the module as it was
    # the kernels have no CPU form, and nn.SyncBatchNorm no longer goes round them
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bn_relu_fn(torch.zeros(4, 8), bn)
    # any other module type still goes through the module itself
    ln = torch.nn.LayerNorm(8)
    x = torch.randn(4, 8)
    assert torch.equal(bn_relu_fn(x, ln), torch.relu(ln(x)))
