"""CPU: the segmentation, encoder, transform and scoring restatements against fixtures produced by the REFERENCE'S OWN
CODE (tests/golden/ref_seg_interp, ref_seg_fp, ref_encoder, ref_transforms, ref_part_metrics; written by
oracle/pin_from_reference.py, which runs the reference's files unmodified and keeps inputs, outputs and recorded numbers).

Each float fixture holds a float32 and a float64 run of the reference on the same fp32 inputs and ``ref32_err``, the
fp32 run's error against the float64 run under the metric the assertion uses.  A CPU restatement repeats the
reference's own fp32 calls, so it is held to the fp32 run bit for bit on the fixture's kind of CPU
(``assert_fixture_floats``); against the float64 run the bound is helpers.pinned_bound: 8 x ref32_err.

Where the reference leaves a behaviour open, the test asserts what this project documents ("Where the
reference is unspecified"), and names the fixture entries that differ:
  * ``sequence.idx32`` of ref_seg_interp: the reference's CPU sort does not return the lowest-index copies of a repeated
    centre; oracle/seg_ref.py and the kernel do.
  * ``metric.class_avg_accuracy`` and ``metric.class_avg_iou`` of ref_part_metrics are NaN in the reference (0/0 for a
    label never seen, mean of an empty list for a category without shapes); tests/part_metrics_ref.py keeps the first and
    leaves empty categories out of the second.
"""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_ref as ar
import part_metrics_ref as pm
from conftest import GOLDEN, assert_fixture_floats, load_golden
from helpers import formula_head, formula_parameters, peak_err, pinned_bound
from oracle import seg_ref
from pinned_cases import INTERP_CAP, assert_recorded, encoder_results, lowest_copies
from pinned_cases import tensor as _t

FLOAT_TOL = dict(rtol=1e-5, atol=1e-6)      # off the fixture's kind of CPU


# ---- 3-NN interpolation ----------------------------------------------------------------------------------------------
def test_interp_fixture_is_not_vacuous():
    """``distinct``: at least 95 % of the queries have the third and fourth distance more than 1e-5 apart, and the fp32 and
    float64 runs chose the same neighbours; ``sequence``: at least 90 % of the queries are tied across that boundary, and
    the reference did NOT take the lowest-index copies; coincident points give a negative squared distance."""
    g = load_golden("ref_seg_interp")
    gap = np.abs(g["distinct.d4_32"] - g["distinct.d32"][:, :, 2])
    assert (gap > 1e-5).mean() >= 0.95
    assert np.array_equal(np.sort(g["distinct.idx32"], -1), np.sort(g["distinct.idx64"], -1))
    tied = g["sequence.d4_32"] == g["sequence.d32"][:, :, 2]
    assert tied.mean() >= 0.90
    low = lowest_copies(_t(g["sequence.xyz2"]), _t(g["sequence.idx32"])).numpy()
    assert (np.sort(g["sequence.idx32"], -1) != low).any(-1).mean() > 0.5
    assert g["distinct.d_min32"] < 0 and g["sequence.d_min32"] < 0
    assert g["sequence.xyz2"].shape[1] == 148 and g["three.xyz2"].shape[1] == 3 and g["one.xyz2"].shape[1] == 1


@pytest.mark.parametrize("case", ["distinct", "three"])
def test_seg_ref_interpolation_equals_reference(case):
    """pointnet2_utils.py:293-300 as the reference ran it vs seg_ref.three_nn_interpolate: neighbours bit for bit (no
    query of these cases is tied across the third / fourth distance), distances, weights and output as fixture floats."""
    g = load_golden("ref_seg_interp")
    xyz1, xyz2, feats = _t(g["xyz1"]), _t(g[f"{case}.xyz2"]), _t(g[f"{case}.feats"])
    out, idx, w = seg_ref.three_nn_interpolate(xyz1, xyz2, feats)
    assert np.array_equal(idx.numpy(), g[f"{case}.idx32"])
    d = seg_ref.square_distance(xyz1, xyz2).sort(dim=-1, stable=True)[0][:, :, :3]
    assert_fixture_floats(d.numpy(), g[f"{case}.d32"], **FLOAT_TOL)
    assert_fixture_floats(w.numpy(), g[f"{case}.w32"], **FLOAT_TOL)
    assert_fixture_floats(out.numpy(), g[f"{case}.out32"], **FLOAT_TOL)
    assert peak_err(out, _t(g[f"{case}.out64"])) <= pinned_bound(g[f"{case}.ref32_err.out"], INTERP_CAP)


def test_seg_ref_interpolation_on_a_model_sequence_takes_the_lowest_copies():
    """Case ``sequence`` (every centre four times, as SAST / HLT lay the centres out): distances and weights are the
    reference's (they do not depend on which copy is taken); the chosen centres' coordinates are the reference's; the
    copies are the three LOWEST slots -- the documented convention, where ``sequence.idx32`` shows the reference's sort
    returning others -- and the output is the interpolation over those."""
    g = load_golden("ref_seg_interp")
    xyz1, xyz2, feats = _t(g["xyz1"]), _t(g["sequence.xyz2"]), _t(g["sequence.feats"])
    out, idx, w = seg_ref.three_nn_interpolate(xyz1, xyz2, feats)
    d = seg_ref.square_distance(xyz1, xyz2).sort(dim=-1, stable=True)[0][:, :, :3]
    assert_fixture_floats(d.numpy(), g["sequence.d32"], **FLOAT_TOL)
    assert_fixture_floats(w.numpy(), g["sequence.w32"], **FLOAT_TOL)
    ref_idx = _t(g["sequence.idx32"])
    assert torch.equal(seg_ref.index_points(xyz2, idx), seg_ref.index_points(xyz2, ref_idx))
    assert torch.equal(idx, lowest_copies(xyz2, ref_idx))
    want = (seg_ref.index_points(feats.double(), idx) * _t(g["sequence.w64"]).unsqueeze(-1)).sum(2)
    assert peak_err(out, want) <= pinned_bound(g["distinct.ref32_err.out"], INTERP_CAP)


@pytest.mark.parametrize("case", ["distinct", "sequence", "three", "one"])
def test_seg_ref_bare_propagation_equals_reference(case):
    """feature_propagation with an empty MLP and points1 = None, S = 1 (the ``repeat`` branch) included.  On ``sequence``
    the comparison is against the interpolation over the lowest copies (see above)."""
    g = load_golden("ref_seg_interp")
    xyz1, xyz2, feats = _t(g["xyz1"]), _t(g[f"{case}.xyz2"]), _t(g[f"{case}.feats"])
    fp = SimpleNamespace(mlp_convs=[], mlp_bns=[])
    out = seg_ref.feature_propagation(fp, xyz1.transpose(1, 2), xyz2.transpose(1, 2), None, feats.transpose(1, 2))
    out = out.transpose(1, 2)
    if case == "sequence":
        idx = lowest_copies(xyz2, _t(g["sequence.idx32"]))
        want = (seg_ref.index_points(feats.double(), idx) * _t(g["sequence.w64"]).unsqueeze(-1)).sum(2)
        assert peak_err(out, want) <= pinned_bound(g["distinct.ref32_err.out"], INTERP_CAP)
    else:
        assert_fixture_floats(out.numpy(), g[f"{case}.out32"], **FLOAT_TOL)


# ---- feature propagation with its MLP --------------------------------------------------------------------------------
def fp_case(g, mode, module, dtype=torch.float32):
    """The module (this package's or the restatement's carrier) with the fixture's formula parameters, in ``mode``."""
    formula_parameters(module, int(g["salt"]), running=(mode == "eval"))
    return module.to(dtype).train(mode == "train")


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_seg_ref_feature_propagation_equals_reference(mode):
    """PointNetFeaturePropagation.forward :273-312 with MLP [32, 16] and points1 = the points, as the reference ran it,
    vs seg_ref.feature_propagation on a module with the same formula parameters: forward as fixture floats, running
    statistics and every gradient (the reference's own autograd, float64) within 8 x ref32_err."""
    from si_mamba_amd.seg import PointNetFeaturePropagation
    g = load_golden("ref_seg_fp")
    fp = fp_case(g, mode, PointNetFeaturePropagation(3 + g["points2"].shape[-1], [int(v) for v in g["mlp"]]))
    x1 = _t(g["xyz1"]).transpose(1, 2)
    p2 = _t(g["points2"]).transpose(1, 2).contiguous().requires_grad_(True)
    out = seg_ref.feature_propagation(fp, x1, _t(g["xyz2"]).transpose(1, 2), x1, p2)
    out.backward(_t(g["dout"]))
    assert_fixture_floats(out.detach().transpose(1, 2).numpy(), g[f"{mode}.out32"], **FLOAT_TOL)
    got = {"out": out.detach().transpose(1, 2)}
    got.update({"grad." + k: p.grad for k, p in fp.named_parameters()})
    got["grad.points2"] = p2.grad.transpose(1, 2)
    got.update({"stat." + k: b for k, b in fp.named_buffers() if "running" in k})
    assert_recorded(g, mode, got)


# ---- segmentation taps and head --------------------------------------------------------------------------------------
def head_carrier(g, mode, fp_cls):
    """A module tree with the names seg_ref.seg_head reads, formula parameters of the fixture's salt."""
    from oracle.pin_from_reference import HEAD_DIMS as D
    nn = torch.nn
    nf = len(D["fetch_idx"]) * D["d"]
    m = nn.Module()
    m.norm = nn.LayerNorm(D["d"])
    m.label_conv = nn.Sequential(nn.Conv1d(16, 64, kernel_size=1, bias=False), nn.BatchNorm1d(64), nn.LeakyReLU(0.2))
    m.propagation_0 = fp_cls(nf + 3, list(D["fp_mlp"]))
    m.convs1 = nn.Conv1d(D["fp_mlp"][-1] + 2 * nf + 64, D["c1"], 1)
    m.bns1 = nn.BatchNorm1d(D["c1"])
    m.convs2 = nn.Conv1d(D["c1"], D["c2"], 1)
    m.bns2 = nn.BatchNorm1d(D["c2"])
    m.convs3 = nn.Conv1d(D["c2"], D["cls_dim"], 1)
    m.dp1 = nn.Dropout(0.5 if mode == "eval" else 0.0)      # train mode is pinned with the dropout off
    formula_head(m, int(g["salt"]), running=(mode == "eval"))
    return m.train(mode == "train")


def test_seg_ref_taps_equal_reference_mixer_model_for_segmentation():
    """MixerModelForSegmentation.forward (pt_mamba.py:390-416) over the reference's own Block / create_block, MambaRef as
    the mixer, vs seg_ref.mixer_taps on the same weights: the three taps as fixture floats."""
    from oracle import scan_ref
    from oracle.pin_from_reference import HEAD_DIMS as D
    from si_mamba_amd.seg import MixerModelForSegmentation
    g = load_golden("ref_seg_head")
    blocks = MixerModelForSegmentation(d_model=D["d"], n_layer=D["n_layer"], rms_norm=False, drop_path=0.0,
                                       fetch_idx=D["fetch_idx"])
    assert list(blocks.state_dict().keys()) == [str(n) for n in g["param_names"]]
    blocks.load_state_dict({str(n): _t(g["param." + str(n)]) for n in g["param_names"]})
    mixers = []
    for layer in blocks.layers:
        r = scan_ref.MambaRef(D["d"])
        r.load_state_dict(layer.mixer.state_dict())
        mixers.append(r.eval())
    with torch.no_grad():
        taps = seg_ref.mixer_taps(blocks.eval(), mixers, _t(g["x"]), _t(g["pos"]))
    assert len(taps) == 3
    for i, t in enumerate(taps):
        assert_fixture_floats(t.numpy(), g[f"tap{i}.32"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_seg_ref_head_equals_reference_head_statements(mode):
    """get_model.forward :768-787 as the reference ran it (its own PointNetFeaturePropagation inside) vs seg_ref.seg_head
    on modules with the same formula parameters: log-probabilities as fixture floats, running statistics within bound."""
    from si_mamba_amd.seg import PointNetFeaturePropagation
    g = load_golden("ref_seg_head")
    m = head_carrier(g, mode, PointNetFeaturePropagation)
    with torch.no_grad():
        out = seg_ref.seg_head(m, _t(g["pts"]).transpose(1, 2), _t(g["cls_label"]), _t(g["sorted_center"]),
                               [_t(g[f"tap{i}.32"]) for i in range(3)])
    assert_fixture_floats(out.numpy(), g[f"{mode}.out32"], **FLOAT_TOL)
    got = {"out": out}
    got.update({"stat." + k: b for k, b in m.named_buffers() if "running" in k})
    assert_recorded(g, mode, got)


# ---- MAE masking and token layout ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rand", "block"])
def test_mae_ref_flow_equals_reference_index_maps(kind):
    """The ``orders`` branch of MaskMamba_2.forward (:2453-2538) and the restore loop / final mask / ground-truth
    selection of Point_MAE_Mamba.forward (:3139-3202) as the reference ran them on index-coded tokens, vs
    mae_ref.encoder_flow / restore_tokens on the reference's own masks: every index map bit for bit.  k = 4 (the reference
    hard-codes ``cnt = 4`` at :3174; mae_ref takes the number of orderings, the same number here).  Chamfer stays
    unpinned (pytorch3d is absent)."""
    from oracle import mae_ref
    from pinned_cases import mae_coded
    g = load_golden("ref_mae_flow")
    B, G, k, M, C = (int(v) for v in g["dims"])
    c = mae_coded(g)
    mask = _t(g[f"mask_{kind}"])
    assert mask.dtype == torch.bool and (mask.sum(1) == int(float(g["mask_ratio"]) * G)).all()
    P = mae_ref.permutation_matrices(_t(g["orders"]), G)
    x_vis, mlist, pos_mask, pos_full, mtensor, nbh = mae_ref.encoder_flow(
        c["tokens"], c["pos"], c["neighborhood"], c["center"], mask, P, True, lambda x, p: x, lambda x: x)
    assert np.array_equal(x_vis[:, :, 0].long().numpy(), g[f"{kind}.x_vis_index"])
    assert np.array_equal(pos_mask[:, :, 0].long().numpy(), g[f"{kind}.pos_mask_index"])
    assert np.array_equal(pos_full[:, :, 0].long().numpy(), g[f"{kind}.pos_full_index"])
    assert np.array_equal(torch.stack(mlist, 1).numpy(), g[f"{kind}.sorted_mask"])
    assert np.array_equal(mtensor.numpy(), g[f"{kind}.sorted_mask_flipped"])
    assert np.array_equal(nbh[:, :, 0, 0].long().numpy(), g[f"{kind}.neighborhood_index"])
    nm = int(float(g["mask_ratio"]) * G)
    x_full = mae_ref.restore_tokens(x_vis, torch.full((1, 1, C), -1.0), mlist, mtensor, nm, G - nm, G)
    assert np.array_equal(x_full[:, :, 0].long().numpy(), g[f"{kind}.x_full_index"])
    final = torch.cat((torch.cat(mlist, 1), mtensor), 1)
    assert np.array_equal(final.numpy(), g[f"{kind}.final_mask"])
    assert np.array_equal(nbh[final].reshape(B * 2 * k * nm, -1, 3)[:, 0, 0].long().numpy(), g[f"{kind}.gt_index"])


def test_reference_block_mask_is_the_nearest_patches_of_the_drawn_seed():
    """_mask_center_block (:2203-2230) as the reference ran it: the mask_ratio * G patches nearest to the patch its
    random.randint drew (recorded).  The product's _mask_center_block draws the seed patch from torch instead; given the
    same seed patch it must mask the same set, which the GPU test asserts."""
    g = load_golden("ref_mae_flow")
    geo, seed = _t(g["geometry"]), g["block_seed_index"]
    G = geo.shape[1]
    for b in range(geo.shape[0]):
        d = (geo[b] - geo[b, int(seed[b])]).norm(dim=-1)
        want = torch.zeros(G, dtype=torch.bool)
        want[d.argsort()[:int(float(g["mask_ratio"]) * G)]] = True
        assert np.array_equal(want.numpy(), g["mask_block"][b])


# ---- encoder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("name", ["n32", "n16"])
def test_composed_encoder_equals_reference_encoder(name, mode):
    """models/point_mamba.py Encoder :42-73 as the reference ran it vs this package's Encoder on its composed torch route
    (the yardstick of tests/test_gpu_encoder.py::test_encoder_fused_matches_composed), same formula parameters: output,
    running statistics, parameter-gradient norms and samples, and the point gradients summed over the duplicated point."""
    from si_mamba_amd.point_mamba import Encoder
    g = load_golden("ref_encoder")
    enc = formula_parameters(Encoder(int(g["encoder_channel"])), int(g["salt"]), running=(mode == "eval"))
    enc.fused = False
    enc.train(mode == "train")
    res = encoder_results(enc, _t(g[f"{name}.points"]), _t(g[f"{name}.dout"]), g["dup"])
    assert_recorded(g, f"{name}.{mode}", res)


# ---- transforms ------------------------------------------------------------------------------------------------------
def transform_draws(name, draws, b, n):
    """The recorded draws of cloud ``b`` as augment_ref.apply_chain takes them: (chain, draws (1, 8), keep)."""
    d, keep = np.zeros(ar.CLOUD_PARAMS), None
    f32 = np.float32
    if name == "PointcloudRotate":
        th = draws[b] * 2 * np.pi
        d[:3] = th, f32(np.cos(th)), f32(np.sin(th))               # the reference rounds the matrix to float32
        chain = [(ar.ROTATE, [])]
    elif name == "PointcloudScaleAndTranslate":
        d[:6] = draws[6 * b:6 * b + 6].astype(f32)                  # scale (3), then translate (3), each .float()
        chain = [(ar.SCALE_TRANSLATE, [2 / 3, 3 / 2, 0.2])]
    elif name == "PointcloudScale":
        d[:3] = draws[3 * b:3 * b + 3].astype(f32)
        chain = [(ar.SCALE, [2 / 3, 3 / 2])]
    elif name == "PointcloudTranslate":
        d[:3] = draws[3 * b:3 * b + 3].astype(f32)
        chain = [(ar.TRANSLATE, [0.2])]
    elif name == "PointcloudJitter":
        chain = [(ar.JITTER, [1.0, 0.05])]                          # the recorded noise is already times std
    elif name == "PointcloudRandomInputDropout":
        ratio, u = draws[(n + 1) * b] * 0.5, draws[(n + 1) * b + 1:(n + 1) * (b + 1)]   # draw times max_dropout_ratio
        keep = ~(u <= ratio)
        chain = [(ar.DROPOUT, [0.5])]
    else:
        raise ValueError(name)
    return chain, d[None], keep


def flip_draws(draws, B):
    """random.random() in call order: per cloud the gate (< 0.95), then one draw per horizontal axis (0, then 1) if the
    gate let the cloud through."""
    out, i = [], 0
    for _ in range(B):
        d = np.zeros(ar.CLOUD_PARAMS)
        d[0] = draws[i] < 0.95
        i += 1
        if d[0]:
            d[1], d[2] = draws[i] < 0.5, draws[i + 1] < 0.5
            i += 2
        out.append(d[None])
    assert i == len(draws)
    return out


def test_augment_ref_equals_reference_transforms():
    """datasets/data_transforms.py, its seven classes run with recorded draws, vs augment_ref.apply_chain given the same
    draws: pins the rotation's sign and axis, scale before translate, flip = max - x on the horizontal axes of an upright
    z, dropout to the cloud's FIRST point and the jitter's clamp.  The reference works in float32, apply_chain in float64
    on the same float32 parameters: each output coordinate goes through at most three roundings of 2^-24 relative to the
    largest magnitude met (two products and a sum in the rotation), so the bound is 4 x 2^-24 x that magnitude."""
    g = load_golden("ref_transforms")
    assert len(g["classes"]) == 7
    for name in (str(c) for c in g["classes"]):
        x, want = g[f"{name}.in"], g[f"{name}.out"]
        B, n, _ = x.shape
        flips = flip_draws(g[f"{name}.draws"], B) if name == "RandomHorizontalFlip" else None
        for b in range(B):
            if flips is not None:
                chain, d, keep = [(ar.FLIP, [2.0])], flips[b], None
            else:
                chain, d, keep = transform_draws(name, g[f"{name}.draws"], b, n)
            noise = g[f"{name}.noise"][b] if name == "PointcloudJitter" else None
            got, big = ar.apply_chain(x[b], chain, d, noise=noise, keep=keep)
            assert np.abs(got - want[b]).max() <= 4 * 2.0 ** -24 * big, (name, b)
            if flips is None:
                assert np.abs(want[b] - x[b]).max() > 1e-3, (name, b)         # every cloud was changed
        if flips is not None:
            on = np.array([f[0, 1:3] for f in flips])
            assert on.any() and not on.all()                                  # the flip both fires and does not


# ---- part-segmentation scoring ---------------------------------------------------------------------------------------
def test_part_metrics_ref_equals_reference_evaluation_loop():
    """part_segmentation/main.py:270-334 as the reference ran it over two batches vs part_metrics_ref.Pass: per-label seen /
    correct counts and accuracy bit for bit, every shape's IoU (absent-and-unpredicted part = 1.0, predicted-but-absent
    part = 0), instance mIoU.  Divergent entries: the reference's ``class_avg_accuracy`` is NaN here (labels never seen:
    0/0) and so is Pass's; its ``class_avg_iou`` is NaN too (np.mean of an empty list for a category without shapes)
    where Pass documents the mean over the categories that have shapes."""
    g = load_golden("ref_part_metrics")
    with open(os.path.join(GOLDEN, "shapenetpart_seg_classes.json")) as fh:
        seg_classes = json.load(fh)
    run = pm.Pass(pm.Table(seg_classes))
    first = run.add(g["batch0.logits"], g["batch0.target"])
    run.add(g["batch1.logits"], g["batch1.target"])
    res = run.result()
    assert np.array_equal(run.seen_class, g["seen_class"]) and np.array_equal(run.correct_class, g["correct_class"])
    assert (g["seen_class"] == 0).any()
    assert res["accuracy"] == float(g["metric.accuracy"])
    cats = [str(c) for c in g["categories"]]
    ref_ious = g["all_shape_ious"]                                   # category by category in seg_classes' order
    mine = np.array([v for c in cats for v in run.shape_ious[c]])
    assert np.array_equal(mine, ref_ious)
    assert res["inctance_avg_iou"] == float(g["metric.inctance_avg_iou"])
    for c, v in zip(cats, g["category_iou"]):
        assert (np.isnan(v) and np.isnan(res["category_iou"][c])) or res["category_iou"][c] == v, c
    # shape 0 of batch 0: part 35 absent and unpredicted; shape 1: part 15 predicted (on 8 points at least) but absent
    assert first["uni"][0, 5] == 0 and first["inter"][1, 3] == 0 and first["uni"][1, 3] >= 8
    assert np.isnan(float(g["metric.class_avg_accuracy"])) and np.isnan(res["class_avg_accuracy"])
    assert np.isnan(float(g["metric.class_avg_iou"]))
    have = g["category_iou"][~np.isnan(g["category_iou"])]
    assert res["class_avg_iou"] == float(np.mean(have))
