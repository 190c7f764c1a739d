"""CPU: add_after_layer=True (the reference's MixerModel_add, models/point_mamba.py:281-428) -- the C ABI of the
gather-sum-scatter kernel (symbol, prototype, argument validation before any launch, the unchanged ABI version), the
index maps against a torch restatement of the reference's merge and re-expansion, and the construction of the model."""
import ctypes

import pytest
import torch

from abi_tables import E_DTYPE, E_NULLPTR, E_SHAPE
from si_mamba_amd import _lib


def restated_merge_expand(hidden, eigvecs, k):
    """Restatement of reference :350-370 (the merge) and :394-409 (the re-expansion, reverse == True), written from the
    line numbers: hidden (B, 2 k G, C) in SAST sequence order, eigvecs (B, G, k) -> (merged (B, G, C), sequence)."""
    B, L, C = hidden.shape
    G = eigvecs.shape[1]
    ranked = torch.sort(eigvecs, dim=1)[1]                              # (B, G, k): patch at every rank    :394
    blocks = hidden.reshape(B, 2 * k, G, C).permute(0, 1, 3, 2)        # (B, 2k, C, G)                     :351
    where = torch.argsort(ranked, 1).permute(0, 2, 1)                  # (B, k, G): rank of every patch    :355
    where = where.unsqueeze(2).expand(-1, -1, C, -1)                   #                                   :356
    first = torch.gather(blocks[:, :k].reshape(B, k, C, -1), -1, where)                     # :357-359
    second = torch.gather(blocks[:, k:].reshape(B, k, C, -1).flip(-1), -1, where)           # :361-362
    both = first + second                                                                   # :364
    total = 0
    for i in range(k):                                                                      # :366-368
        total = total + both[:, i]
    merged = total.permute(0, 2, 1)                                                         # :370
    pieces = []
    for i in range(k):                                                                      # :398-404, :372-381
        by_vec = torch.sort(eigvecs[:, :, i], dim=1)[1]
        pieces.append(torch.gather(merged, 1, by_vec.unsqueeze(-1).expand(-1, -1, C)))
    half = torch.cat(pieces, 1)
    return merged, torch.cat((half, half.flip(1)), 1)                                       # :407-409


def eigvecs_and_order(B, G, k, seed):
    g = torch.Generator().manual_seed(seed)
    vecs = torch.randn(B, G, k, generator=g)
    return vecs, torch.sort(vecs, dim=1)[1].transpose(1, 2).contiguous()     # order (B, k, G)


def test_symbol_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "simamba_gather_sum_scatter")
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["simamba_gather_sum_scatter"] == (I, [P, P, P, P, I, I, I, I, I, I, P])
    assert _lib.load().simamba_abi_version() == 9
    assert _lib.ABI_VERSION == 9


def test_validation_precedes_any_launch():
    gss = _lib.load().simamba_gather_sum_scatter
    one = ctypes.c_void_p(16)                # never dereferenced: every call below returns before a launch
    n = None
    F32 = _lib.F32
    # (x, gather_idx, scatter_idx, y, batch, L, G, M, C, io_dtype, stream)
    assert gss(one, one, one, one, 2, 1000, 128, 8, 384, F32, n) == E_SHAPE        # L != M * G
    assert gss(one, one, one, one, 2, 384, 128, 3, 384, F32, n) == E_SHAPE         # M odd
    assert gss(one, one, one, one, 2, 0, 128, 0, 384, F32, n) == E_SHAPE           # M = 0
    assert gss(one, one, one, one, 2, 18 * 128, 128, 18, 384, F32, n) == E_SHAPE   # M = 18
    assert gss(one, one, one, one, 2, 1024, 128, 8, 6, F32, n) == E_SHAPE          # C = 6
    assert gss(one, one, one, one, 65536, 1024, 128, 8, 384, F32, n) == E_SHAPE    # batch = 65536
    assert gss(one, one, one, one, 2, 1024, 128, 8, 384, 7, n) == E_DTYPE          # bad dtype
    for dt in (_lib.F32, _lib.BF16):
        assert gss(n, one, one, one, 2, 1024, 128, 8, 384, dt, n) == E_NULLPTR     # x
        assert gss(one, n, one, one, 2, 1024, 128, 8, 384, dt, n) == E_NULLPTR     # gather_idx
        assert gss(one, one, n, one, 2, 1024, 128, 8, 384, dt, n) == E_NULLPTR     # scatter_idx
        assert gss(one, one, one, n, 2, 1024, 128, 8, 384, dt, n) == E_NULLPTR     # y
        assert gss(n, n, n, n, 0, 1024, 128, 8, 384, dt, n) == 0                   # empty batch: nothing to do
    # the dtype is looked at first
    assert gss(n, n, n, n, 2, 1000, 128, 3, 6, 7, n) == E_DTYPE


@pytest.mark.parametrize("G,k", [(7, 3), (8, 1), (16, 4)])
def test_maps_match_the_restated_reference(G, k):
    from si_mamba_amd.cross_merge import cross_merge_maps
    B, L = 3, 2 * k * G
    vecs, order = eigvecs_and_order(B, G, k, seed=G * 10 + k)
    src, dst = cross_merge_maps(order)
    assert src.dtype == dst.dtype == torch.int32 and src.shape == dst.shape == (B, 2 * k, G)
    every = torch.arange(L, dtype=torch.int32).expand(B, L)
    assert torch.equal(src.flatten(1).sort(1)[0], every)                # bijections of [0, L) per cloud
    assert torch.equal(dst.flatten(1).sort(1)[0], every)
    # Read the maps off the restatement: on a tensor whose row p is the one-hot of its own position number p, merged[g]
    # marks exactly the positions summed into patch g, and the output row at position p is merged[g] of the patch g
    # written there.  Every G-row segment holds one copy of a patch: ascending positions are segments 0 .. 2k-1.
    onehot = torch.eye(L, dtype=torch.float64).expand(B, L, L).contiguous()
    merged, seq = restated_merge_expand(onehot, vecs, k)                # (B, G, L), (B, L, L)
    assert torch.equal(merged.sum(2), torch.full((B, G), 2.0 * k, dtype=torch.float64))
    read = merged.argsort(dim=2, descending=True, stable=True)[:, :, :2 * k].permute(0, 2, 1)
    assert torch.equal(read.to(torch.int32), src)                       # src[m] lies in segment m
    written = (seq.unsqueeze(1) == merged.unsqueeze(2)).all(-1).to(torch.float64)          # (B, G, L)
    assert torch.equal(written.sum(2), torch.full((B, G), 2.0 * k, dtype=torch.float64))
    read = written.argsort(dim=2, descending=True, stable=True)[:, :, :2 * k].permute(0, 2, 1)
    read = torch.cat((read[:, :k], read[:, k:].flip(1)), 1)             # dst_r[i] lies in segment 2k-1-i
    assert torch.equal(read.to(torch.int32), dst)
    # and values: the formulas reproduce merged and the re-expanded sequence bit for bit, additions in the stated order
    h = torch.randn(B, L, 8, generator=torch.Generator().manual_seed(1))
    merged, seq = restated_merge_expand(h, vecs, k)
    rows = torch.gather(h, 1, src.flatten(1).long().unsqueeze(-1).expand(-1, -1, 8)).view(B, 2 * k, G, 8)
    acc = rows[:, 0] + rows[:, k]
    for i in range(1, k):
        acc = acc + (rows[:, i] + rows[:, k + i])
    assert torch.equal(acc, merged)
    out = torch.empty_like(h)
    out.scatter_(1, dst.flatten(1).long().unsqueeze(-1).expand(-1, -1, 8), acc.repeat(1, 2 * k, 1))
    assert torch.equal(out, seq)


def test_composed_form_is_the_restatement():
    from si_mamba_amd.cross_merge import cross_merge_composed
    B, G, k, C = 2, 7, 3, 8
    vecs, order = eigvecs_and_order(B, G, k, seed=5)
    h = torch.randn(B, 2 * k * G, C, generator=torch.Generator().manual_seed(2))
    assert torch.equal(cross_merge_composed(h, order), restated_merge_expand(h, vecs, k)[1])


def test_op_has_no_cpu_fallback():
    from si_mamba_amd.cross_merge import cross_merge, cross_merge_maps
    _, order = eigvecs_and_order(1, 8, 1, seed=0)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        cross_merge(torch.zeros(1, 16, 4), cross_merge_maps(order))


def test_construction():
    from si_mamba_amd.block import MixerModel, MixerModel_add
    from si_mamba_amd.point_mamba import PointMamba, default_config
    small = dict(trans_dim=64, encoder_dims=64, depth=2, num_group=16, group_size=8)
    assert not hasattr(default_config(), "add_after_layer")             # default_config is left alone
    plain = PointMamba(default_config(**small))
    assert type(plain.blocks) is MixerModel and plain.add_after_layer is False
    assert type(PointMamba(default_config(add_after_layer=False, **small)).blocks) is MixerModel
    m = PointMamba(default_config(add_after_layer=True, **small))
    assert type(m.blocks) is MixerModel_add and MixerModel_add.composed is False
    assert list(m.state_dict()) == list(plain.state_dict())
    assert all(a.shape == b.shape for a, b in zip(m.state_dict().values(), plain.state_dict().values()))
    for bad in (dict(reverse=False), dict(method="HLT")):
        with pytest.raises(ValueError, match="add_after_layer") as e:
            PointMamba(default_config(add_after_layer=True, **small, **bad))
        assert "reverse" in str(e.value) and "method" in str(e.value)
