"""GPU: batches out of a device-resident dataset in one launch (csrc/dataset.hip, si_mamba_amd/data.py) against the numpy
restatement of dataset_ref.py.

The stores of the index tests encode identity in their coordinates, x = sample id, y = row id, z = 0 (all exact in
fp32), so that without normalisation the output names every pick and is compared bit for bit.

UNIT_SPHERE is compared with pc_norm in float64 on the same picks, within the bound dataset_ref.unit_sphere64 derives
from the kernel's order of operations (not fitted to what the kernel gives).  Measured on an MI355X
(profiles/device_loader.json): at most 0.024 of the bound (a worst case over every rounding of the sum).
"""
import numpy as np
import pytest
import torch

import dataset_ref as dr
from helpers import same_bits

pytestmark = pytest.mark.gpu

SEED = 0xa4093822299f31d0            # both key words in use
SIZES_S = [1, 5, 64, 65, 1000]
SIZES_B = [1, 3, 64]
SIZES_K = [1, 63, 64, 65, 1023, 1024, 1025, 8192]   # wave boundary, one row per lane boundary, register limit
RULES = {"first": dr.FIRST, "permute": dr.PERMUTE, "choice": dr.CHOICE}


def D():
    from si_mamba_amd import data
    return data


def cloud_lengths(S, K, ragged):
    """Fixed: K + 3 points each.  Ragged: 1, K - 1 (an empty cloud at K = 1), K, K + 1, 2 K + 1 and 7 in turn."""
    if not ragged:
        return np.full(S, K + 3, dtype=np.int64)
    return np.array([[1, K - 1, K, K + 1, 2 * K + 1, 7][s % 6] for s in range(S)], dtype=np.int64)


_stores = {}


def identity_store(S, K, ragged, device):
    """x = sample id, y = row id, z = 0; label 3 s + 1; point label 7 s + row."""
    key = (S, K, ragged)
    if key not in _stores:
        if len(_stores) >= 6:
            _stores.clear()
        lengths = cloud_lengths(S, K, ragged)
        n = torch.as_tensor(lengths, device=device)
        sid = torch.repeat_interleave(torch.arange(S, device=device), n)
        start = torch.cumsum(n, 0) - n
        row = torch.arange(int(lengths.sum()), device=device) - start[sid]
        flat = torch.stack([sid.float(), row.float(), torch.zeros_like(row).float()], 1)
        plabel = (7 * sid + row).to(torch.int32)
        labels = 3 * torch.arange(S, device=device) + 1
        if ragged:
            cuts = np.cumsum(lengths)[:-1].tolist()
            store = D().DeviceDataset.from_arrays(list(torch.tensor_split(flat, cuts)), labels,
                                                  list(torch.tensor_split(plabel, cuts)), device=device)
            assert store.offsets is not None and store.stride == 0
        else:
            store = D().DeviceDataset.from_arrays(flat.view(S, K + 3, 3), labels, plabel.view(S, K + 3), device=device)
            assert store.offsets is None and store.stride == K + 3
        assert len(store) == S and store.nbytes >= int(lengths.sum()) * 16
        _stores[key] = (store, lengths)
    return _stores[key]


def check_batch(got, lengths, B, K, step, spe, rule, first, shuffle=True, rank=0, world=1, seed=SEED):
    idx, picks, length = dr.batch(lengths, B, K, seed, step, spe, rank, world, shuffle, RULES[rule], first)
    np.testing.assert_array_equal(got.index.cpu().numpy(), idx)
    np.testing.assert_array_equal(got.lengths.cpu().numpy(), length)
    np.testing.assert_array_equal(got.label.cpu().numpy(), np.where(idx >= 0, 3 * idx + 1, -1))
    valid = picks >= 0
    assert (valid == (np.arange(K)[None] < length[:, None])).all()
    want = np.zeros((B, K, 3), dtype=np.float32)
    want[..., 0] = np.where(valid, idx[:, None], 0)
    want[..., 1] = np.where(valid, picks, 0)
    np.testing.assert_array_equal(got.points.cpu().numpy().view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(got.point_label.cpu().numpy(), np.where(valid, 7 * idx[:, None] + picks, -1))
    return idx, picks, length


# ---- picks against the restatement, bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("K", SIZES_K)
def test_picks_against_the_restatement(device, K, rule, ragged):
    """Every S and B, with first = 0, K - 1 (fewer candidates than rows: padding) and K + 1; the last step of epoch 3,
    whose batch runs behind the dataset wherever S is no multiple of B (and is mostly empty slots where S < B)."""
    for S in SIZES_S:
        store, lengths = identity_store(S, K, ragged, device)
        for B in SIZES_B:
            for first in (0, max(K - 1, 1), K + 1):
                loader = D().DeviceLoader(store, B, K, shuffle=True, drop_last=False, subsample=rule, first=first,
                                          seed=SEED)
                spe = len(loader)
                assert spe == -(-S // B)
                step = 3 * spe + spe - 1
                loader.manual_seed(SEED, step)
                idx, _, length = check_batch(loader.fetch(), lengths, B, K, step, spe, rule, first)
                assert (idx < 0).sum() == spe * B - S
                if rule == "choice":
                    assert set(length[idx >= 0].tolist()) <= {0, K}


def test_sequential_without_drop_last_and_reused_outputs(device):
    store, lengths = identity_store(65, 64, True, device)
    loader = D().DeviceLoader(store, 3, 64, shuffle=False, drop_last=False, subsample="first", seed=SEED)
    assert len(loader) == 22
    out = None
    for step, got in enumerate(loader):
        idx, _, _ = check_batch(got, lengths, 3, 64, step, 22, "first", 0, shuffle=False)
        assert idx.tolist() == [s if s < 65 else -1 for s in range(3 * step, 3 * step + 3)]
        out = got
    assert step == 21 and out.index.tolist() == [63, 64, -1] and out.lengths[2].item() == 0
    assert loader.step == 22 and loader.epoch == 1
    # out=: the same storage is written, every element of it
    for t in out:
        t.fill_(-3)
    again = loader.manual_seed(SEED, 21).fetch(out=out)
    assert all(a is b for a, b in zip(again, out))
    check_batch(again, lengths, 3, 64, 21, 22, "first", 0, shuffle=False)
    with pytest.raises(ValueError):
        loader.fetch(out=out._replace(points=out.points[:, :32].contiguous()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loader.fetch(out=out._replace(index=out.index.cpu()))
    # a store without labels gives none
    bare = D().DeviceDataset.from_arrays(np.zeros((4, 9, 3), np.float32), device=device)
    got = D().DeviceLoader(bare, 2, 9, subsample="first").fetch()
    assert got.label is None and got.point_label is None and got.lengths.tolist() == [9, 9]


# ---- epochs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 3])
def test_an_epoch_visits_every_sample_once_across_the_ranks(device, world):
    S, B, K = 100, 4, 8
    store, _ = identity_store(S, K, False, device)
    seen, orders = [], []
    for rank in range(world):
        loader = D().DeviceLoader(store, B, K, seed=SEED, rank=rank, world=world)
        assert len(loader) == S // (B * world)
        mine = torch.cat([b.index for b in loader]).cpu().numpy()
        assert loader.step == len(loader) and loader.epoch == 1
        nxt = torch.cat([b.index for b in loader]).cpu().numpy()
        assert len(set(mine.tolist())) == len(mine) == len(loader) * B and mine.min() >= 0
        assert len(set(nxt.tolist())) == len(nxt) and not np.array_equal(mine, nxt)
        seen.append(mine)
        orders.append(nxt)
    everything = np.concatenate(seen)
    assert len(set(everything.tolist())) == len(everything) == (S // (B * world)) * B * world
    for r in range(world):
        for q in range(r + 1, world):
            assert not set(seen[r].tolist()) & set(seen[q].tolist())
    # the ranks interleave the one order a single process walks
    single = D().DeviceLoader(store, B * world, K, seed=SEED)
    whole = torch.cat([b.index for b in single]).cpu().numpy()
    assert len(single) == len(seen[0]) // B
    np.testing.assert_array_equal(np.stack([m.reshape(-1, B) for m in seen], 2).ravel(), whole)


@pytest.mark.parametrize("rule", list(RULES))
def test_a_slot_does_not_depend_on_the_batch_size(device, rule):
    """B = 6 at step 0 is B = 3 at steps 0 and 1, to the bit: rows, normalisation and labels included."""
    g = torch.Generator().manual_seed(3)
    pts = torch.rand(100, 40, 3, generator=g) * 2 - 1
    store = D().DeviceDataset.from_arrays(pts.numpy(), np.arange(100), np.arange(4000).reshape(100, 40), device=device)
    kw = dict(subsample=rule, normalize="unit_sphere", seed=SEED, first=33)
    six = D().DeviceLoader(store, 6, 32, **kw).fetch()
    three = D().DeviceLoader(store, 3, 32, **kw)
    a, b = three.fetch(), three.fetch()
    for name in ("points", "label", "point_label", "index", "lengths"):
        x, y = getattr(six, name), torch.cat([getattr(a, name), getattr(b, name)])
        assert torch.equal(x, y) and (name != "points" or same_bits(x, y)), name
    assert len(set(six.index.tolist())) == 6


# ---- unit sphere ---------------------------------------------------------------------------------------------------
def random_store(S, n, device, seed=5):
    """Clouds in [-1, 1]^3, every third one moved away from the origin (the mean then costs bits)."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(S, n, 3, generator=g) * 2 - 1
    pts[::3] += torch.tensor([5., -3., 2.])
    return pts


@pytest.mark.parametrize("rule", ["permute", "choice"])
@pytest.mark.parametrize("K", [1, 2, 63, 65, 1024, 1025, 8192])
def test_unit_sphere_against_float64(device, K, rule):
    S, B = 7, 5
    n = K + 3
    pts = random_store(S, n, device)
    store = D().DeviceDataset.from_arrays(pts, device=device)
    loader = D().DeviceLoader(store, B, K, drop_last=False, subsample=rule, normalize="unit_sphere", seed=SEED)
    step = 1                                                   # the last of the epoch: 7 = 5 + 2, three empty slots
    got = loader.manual_seed(SEED, step).fetch()
    idx, picks, length = dr.batch(np.full(S, n), B, K, SEED, step, 2, rows=RULES[rule])
    np.testing.assert_array_equal(got.index.cpu().numpy(), idx)
    out = got.points.cpu().numpy()
    worst = 0.0
    for b in range(B):
        if idx[b] < 0:
            assert not out[b].any()
            continue
        want, bound = dr.unit_sphere64(pts[idx[b]].numpy()[picks[b, :length[b]]])
        err = np.abs(out[b, :length[b]].astype(np.float64) - want).max()
        if bound > 0:
            worst = max(worst, err / bound)
        assert err <= bound, (b, err, bound)
        if bound > 0:                                          # not one row, or one row drawn twice
            norms = np.sqrt((out[b].astype(np.float64) ** 2).sum(1))
            assert abs(norms.max() - 1) < 1e-6
    print(f"unit_sphere K={K} {rule}: largest error / bound = {worst:.3f}")


def test_unit_sphere_of_coinciding_points_is_zero(device):
    """The reference divides by zero here.  0.1 is not representable and 3 x 0.1 / 3 rounds away from it in fp32: the
    kernel takes row 0 off first, so the rows become exact zeros."""
    pts = torch.full((4, 70, 3), 0.1)
    pts[1] = torch.tensor([1e30, -7.3, 0.3])
    pts[2, 1:] = torch.rand(69, 3)                             # an ordinary cloud among them
    store = D().DeviceDataset.from_arrays(pts, device=device)
    for K in (3, 65):
        got = D().DeviceLoader(store, 4, K, shuffle=False, normalize="unit_sphere").fetch()
        out = got.points.cpu().numpy()
        assert not out[0].any() and not out[1].any() and not out[3].any()
        assert np.isfinite(out).all() and abs(np.sqrt((out[2].astype(np.float64) ** 2).sum(1)).max() - 1) < 1e-6


def test_a_nan_stays_in_its_own_slot(device):
    pts = random_store(9, 300, device)
    kw = dict(subsample="permute", normalize="unit_sphere", seed=SEED)
    clean = D().DeviceLoader(D().DeviceDataset.from_arrays(pts, device=device), 9, 300, **kw).fetch()
    pts[4, 17, 1] = float("nan")
    pts[4, 200, 0] = float("inf")
    dirty = D().DeviceLoader(D().DeviceDataset.from_arrays(pts, device=device), 9, 300, **kw).fetch()
    assert torch.equal(clean.index, dirty.index) and sorted(clean.index.tolist()) == list(range(9))
    slot = clean.index.tolist().index(4)
    for b in range(9):
        assert same_bits(clean.points[b], dirty.points[b]) == (b != slot), b


def test_whole_cloud_normalisation_when_the_store_is_built(device):
    g = torch.Generator().manual_seed(8)
    clouds = [torch.rand(n, 3, generator=g) * 4 + 1 for n in (1, 5, 300, 64)]
    clouds.append(torch.full((6, 3), 2.5))
    for ragged in (True, False):
        src = clouds if ragged else [c[:1].expand(5, 3) + torch.rand(5, 3, generator=g) for c in clouds]
        store = D().DeviceDataset.from_arrays(src if ragged else torch.stack(src), device=device).normalize_()
        flat, o = store.points.cpu().numpy(), 0
        for c in src:
            x = c.numpy().astype(np.float64)
            r = x - x.mean(0)
            m = np.sqrt((r * r).sum(1)).max()
            want = r / m if m > 1e-6 else np.zeros_like(r)
            np.testing.assert_allclose(flat[o:o + len(x)], want, atol=1e-5)
            o += len(x)


# ---- state and capture ---------------------------------------------------------------------------------------------
def test_state(device):
    pts = random_store(50, 80, device)
    store = D().DeviceDataset.from_arrays(pts, np.arange(50), device=device)
    loader = D().DeviceLoader(store, 4, 64, normalize="unit_sphere", seed=1234)
    assert (loader.state.seed, loader.step, loader.epoch, len(loader)) == (1234, 0, 0, 12)
    a = loader.fetch()
    assert loader.step == 1
    b = loader.fetch()
    assert loader.step == 2 and loader.state.seed == 1234
    assert not same_bits(a.points, b.points) and not torch.equal(a.index, b.index)
    loader.manual_seed(1234)
    assert same_bits(loader.fetch().points, a.points) and same_bits(loader.fetch().points, b.points)
    other = D().DeviceLoader(store, 4, 64, normalize="unit_sphere", seed=1235).fetch()
    assert not torch.equal(other.index, a.index)
    # the same sample in another epoch: other rows of it
    loader.manual_seed(1234, 12 * 5)
    assert loader.epoch == 5
    e5 = torch.cat([x.index for x in loader])
    assert sorted(e5.tolist()) != list(range(48)) and len(set(e5.tolist())) == 48 and loader.epoch == 6
    # a step beyond 2^32, and one that is negative as an int64
    for step in ((1 << 32) + 5, (1 << 63) + 12 * 7 + 3):
        got = loader.manual_seed(1234, step).fetch()
        idx, picks, _ = dr.batch(np.full(50, 80), 4, 64, 1234, step, 12)
        np.testing.assert_array_equal(got.index.cpu().numpy(), idx)
        assert loader.step == (step + 1) % (1 << 64)


def small_model(device):
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    cfg = default_config(trans_dim=32, encoder_dims=32, depth=2, num_group=16, group_size=8, drop_path=0.,
                         knn_graph=8, cls_dim=5)
    return PointMamba(cfg).to(device).eval()


def test_captured_fetch_yields_the_next_batch_at_every_replay(device):
    from si_mamba_amd import transforms as t
    tr = [t.PointcloudRotate(), t.PointcloudScaleAndTranslate(), t.PointcloudJitter()]
    model = small_model(device)
    store = D().DeviceDataset.from_arrays(random_store(10, 200, device), np.arange(10) % 5, device=device)
    loader = D().DeviceLoader(store, 2, 128, normalize="unit_sphere", seed=77)
    st = t.AugmentState(78, device)
    batch = loader.fetch()
    aug = torch.empty_like(batch.points)

    def step():
        loader.fetch(out=batch)
        return model(t.sample_and_augment(batch.points, tr, state=st, out=aug))

    with torch.no_grad():
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.synchronize()
        start, aug_start = loader.step, st.step
        assert (start, aug_start) == (2, 1)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            logits = step()
        seen, outs = [], []
        for _ in range(3):
            graph.replay()
            seen.append([None if x is None else x.clone() for x in batch] + [aug.clone()])
            outs.append(logits.clone())
        torch.cuda.synchronize()
        assert loader.step == start + 3 and st.step == aug_start + 3
        for i, j in ((0, 1), (1, 2), (0, 2)):
            assert not same_bits(seen[i][0], seen[j][0]) and not torch.equal(seen[i][3], seen[j][3])
        loader.manual_seed(77, start)
        st.manual_seed(78, aug_start)
        for k in range(3):
            eager = loader.fetch()
            assert same_bits(eager.points, seen[k][0]) and torch.equal(eager.label, seen[k][1]), k
            assert torch.equal(eager.index, seen[k][3]) and torch.equal(eager.lengths, seen[k][4]), k
            pts = t.sample_and_augment(eager.points, tr, state=st)
            assert same_bits(pts, seen[k][5]), k
            assert torch.allclose(model(pts), outs[k], rtol=1e-4, atol=1e-4)


def test_loader_inside_a_graphed_train_step(device):
    """The recipe of DeviceLoader's docstring: the loader in place of the static inputs, a dummy for the step."""
    from si_mamba_amd import transforms as t
    from si_mamba_amd.graphed import GraphedTrainStep
    model = small_model(device).train()
    store = D().DeviceDataset.from_arrays(random_store(12, 200, device), np.arange(12) % 5, device=device)
    loader = D().DeviceLoader(store, 4, 128, normalize="unit_sphere", seed=9)
    aug = t.AugmentState(10, device)
    taken = torch.full((4,), -1, device=device, dtype=torch.int64)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, capturable=True)

    def loss_fn(_):
        b = loader.fetch()
        taken.copy_(b.index)
        pts = t.sample_and_augment(b.points, [t.PointcloudScaleAndTranslate()], state=aug)
        return model.get_loss_acc(model(pts), b.label)[0]

    step = GraphedTrainStep(loss_fn, opt, (torch.zeros(1, device=device),), warmup=2)
    assert loader.step == 2
    loader.manual_seed(9)
    got = []
    for _ in range(2 * len(loader)):
        loss = step()
        got.append(taken.clone())
        assert torch.isfinite(loss)
    assert loader.step == 6 and loader.epoch == 2
    for e in range(2):
        assert sorted(torch.cat(got[3 * e:3 * e + 3]).tolist()) == list(range(12))
    want = [dr.slot_samples(12, 4, 9, k, 3)[0] for k in range(6)]
    np.testing.assert_array_equal(torch.stack(got).cpu().numpy(), np.stack(want))
