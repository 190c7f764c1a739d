"""GPU parity against fixtures produced by the REFERENCE'S OWN CODE (tests/golden/ref_*.npz, written by
oracle/pin_from_reference.py from /root/reference/models/point_mamba.py and models/block.py; the reference itself is
not on the GPU box -- only these files travel).

The graph / eigen / ordering kernels are held to the ref_spectral_* files by tests/test_gpu_spectral.py (every test
there runs against both fixture families).  Here: the token assembly (SAST index map, HLT order + slot map) and the
block stack -- the reference's Block / MixerModel / create_block / _init_weights around the oracle mixer -- against the
product's Block / MixerModel on the HIP kernels.  The mixer's scan / conv arithmetic is upstream mamba-ssm's (absent):
that part of the comparison is against the oracle's restatement, "parity unpinned" (oracle/__init__.py).

Second half: the 3-NN interpolation, PointNetFeaturePropagation, the segmentation taps and head, the patch Encoder and the
MAE token layout against ref_seg_interp / ref_seg_fp / ref_seg_head / ref_encoder / ref_mae_flow.  Every fp32 bound is
helpers.pinned_bound: 8 x the error of the reference's own fp32 run against its float64 run, read from the fixture.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import clouds, nerr

pytestmark = pytest.mark.gpu

NAMES = ["spectral_g64", "spectral_g128", "spectral_g128_surface"]


@pytest.mark.parametrize("name", NAMES)
def test_sast_assembly_equals_reference_index_map(name, device):
    """models/point_mamba.py:889-898 + :982-989 as the reference ran them (index-coded tokens) vs spectral.sast_gather
    and sast_index_map on the reference's orders: index work, bit-exact."""
    from si_mamba_amd import spectral
    from oracle.gen_golden import SPECTRAL_COMBOS
    g = load_golden("ref_" + name)
    B, G = g["centers"].shape[:2]
    tok = torch.arange(G, dtype=torch.float32, device=device)[None, :, None].expand(B, G, 384).contiguous()
    for cb in SPECTRAL_COMBOS:
        t = cb["tag"]
        order = torch.from_numpy(g[f"{t}.order"]).to(device)
        want = torch.from_numpy(g[f"{t}.sast_index"])
        assert torch.equal(spectral.sast_index_map(order, reverse=True).cpu(), want)
        x, p = spectral.sast_gather(tok, tok + 1000.0, order, reverse=True)
        assert torch.equal(x[:, :, 0].long().cpu(), want) and torch.equal(x[:, :, 383].long().cpu(), want)
        assert torch.equal(p[:, :, 5].long().cpu(), want + 1000)
        # sort_points_by_fiedler (:817-826) on the reference's eigenvectors reproduces the reference's orders
        vecs = torch.from_numpy(g[f"{t}.vecs"]).to(device)
        for i in range(4):
            got = spectral.sort_points_by_fiedler(tok, vecs[:, :, i].contiguous())[:, :, 0].long().cpu()
            assert torch.equal(got, torch.from_numpy(g[f"{t}.order"])[:, i]), (t, i)


@pytest.mark.parametrize("name", NAMES)
def test_hlt_equals_reference_outputs(name, device):
    """models/point_mamba.py:1059-1112 as the reference ran it (its own torch.rand tie-break redrawn from the recorded
    seed) vs spectral.multilevel_travers / hlt_assemble: codes, order and the overlapping block assembly, bit-exact."""
    from si_mamba_amd import spectral
    g = load_golden("ref_" + name)
    centers = torch.from_numpy(g["centers"]).to(device)
    vecs = torch.from_numpy(g["hlt.vecs"]).to(device)
    B, G = centers.shape[:2]
    assert torch.equal(spectral.multilevel_travers(vecs, 3).cpu(), torch.from_numpy(g["hlt.codes"]))
    torch.manual_seed(int(g["hlt.rand_seed"]))
    rand = torch.rand(B, G).to(device)                       # the CPU generator the reference's run drew from
    tok = (1.0 + torch.arange(G, dtype=torch.float32, device=device))[None, :, None].expand(B, G, 8).contiguous()
    out_t, out_p, out_c, order = spectral.hlt_assemble(tok, tok + 1000.0, centers, vecs, 3, rand)
    assert torch.equal(order.cpu(), torch.from_numpy(g["hlt.order"]))
    np.testing.assert_array_equal(out_t[:, :, 0].cpu().numpy(), g["hlt.tokens_index"])
    np.testing.assert_array_equal(out_p[:, :, 0].cpu().numpy(), g["hlt.pos_index"])
    np.testing.assert_array_equal(out_c.cpu().numpy(), g["hlt.center"])


def test_block_stack_on_hip_equals_reference_block_and_mixermodel(device):
    """The reference's MixerModel / Block / create_block / _init_weights (models/point_mamba.py:115-272,
    models/block.py:17-76), run from its own files around the oracle mixer, vs this package's MixerModel and Block with
    the same weights on the HIP kernels: forward, input gradients, every parameter gradient, and both Block call forms."""
    from si_mamba_amd.block import MixerModel
    g = load_golden("ref_stack")
    d, n_layer, B, L = (int(v) for v in g["dims"])
    model = MixerModel(d_model=d, n_layer=n_layer, rms_norm=False, drop_path=0.0).to(device)
    sd = {k[len("param."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param.")}
    assert list(model.state_dict().keys()) == [str(n) for n in g["param_names"]]
    model.load_state_dict(sd)
    x = torch.from_numpy(g["x"]).to(device).requires_grad_(True)
    pos = torch.from_numpy(g["pos"]).to(device).requires_grad_(True)
    out = model(x, pos)
    out.backward(torch.from_numpy(g["dout"]).to(device))
    assert nerr(out, torch.from_numpy(g["out"])) < 1e-3
    assert nerr(x.grad, torch.from_numpy(g["grad_x"])) < 1e-3
    assert nerr(pos.grad, torch.from_numpy(g["grad_pos"])) < 1e-3
    for k, p in model.named_parameters():
        assert nerr(p.grad, torch.from_numpy(g["grad." + k])) < 1e-3, k
    blk = model.layers[0]
    h, r = torch.from_numpy(g["block.h"]).to(device), torch.from_numpy(g["block.r"]).to(device)
    h1, r1 = blk(h, None)
    assert nerr(h1, torch.from_numpy(g["block.first.h"])) < 1e-3 and torch.equal(r1.detach().cpu(), torch.from_numpy(g["block.first.r"]))
    h2, r2 = blk(h, r)
    assert nerr(h2, torch.from_numpy(g["block.next.h"])) < 1e-3
    np.testing.assert_allclose(r2.detach().cpu().numpy(), g["block.next.r"], rtol=0, atol=1e-6)


# ---- the segmentation head and the encoder against the reference's own runs ------------------------------------------
# Fixtures ref_seg_interp / ref_seg_fp / ref_encoder hold a float32 and a float64 run of the reference's code and
# ``ref32_err``, the former's error against the latter.  fp32 bound of every assertion: helpers.pinned_bound = 8 x
# ref32_err under the same metric, capped by what tests/test_gpu_seg.py / tests/test_gpu_encoder.py allow.
@pytest.mark.parametrize("case", ["distinct", "sequence", "three", "one"])
def test_three_nn_equals_reference_propagation(case, device):
    """csrc/interp.hip against pointnet2_utils.PointNetFeaturePropagation (empty MLP) as the reference ran it.
      * the three distances (float64, to the centres the kernel chose) and the weights, each sorted, equal the reference's;
      * the chosen centres' coordinates equal the reference's as a multiset -- whichever copy of a repeated centre;
      * where no query is tied across the third / fourth distance (``distinct``, ``three``) the index sets are equal and
        the end-to-end output is the reference's;
      * three_interpolate fed the reference's OWN idx and weights reproduces its output, and its dfeats is the float64
        scatter of the recorded weights;
      * ``sequence`` (every centre four times, as in a model sequence): the reference's sort leaves open which copies it
        returns and its CPU run did not return the lowest; the kernel documents lowest-index, so its end-to-end output is
        held to the float64 interpolation over the three lowest copies;
      * ``one``: S = 1, the reference's ``repeat`` branch against the kernel's S < 3 branch.  (S = 2 cannot run in the
        reference -- weight.view(B, N, 3, 1) -- and stays with tests/test_gpu_seg.py.)"""
    from helpers import peak_err, pinned_bound
    from pinned_cases import INTERP_CAP, gather_interp, lowest_copies, same_multiset, scatter_interp, tensor
    from si_mamba_amd.interp import three_interpolate, three_nn
    g = load_golden("ref_seg_interp")
    xyz1, dout, xyz2, feats = tensor(g["xyz1"]), tensor(g["dout"]), tensor(g[f"{case}.xyz2"]), tensor(g[f"{case}.feats"])
    B, N, _ = xyz1.shape
    S = xyz2.shape[1]
    bound = lambda k, c=case: pinned_bound(g[f"{c}.ref32_err.{k}"], INTERP_CAP)      # noqa: E731
    idx, w = three_nn(xyz1.to(device), xyz2.to(device))
    f = feats.to(device).requires_grad_(True)
    out = three_interpolate(f, idx, w)
    out.backward(dout.to(device))
    idx_c, w_c = idx.cpu().long(), w.cpu()
    figures = {}
    if case == "one":
        figures["out"] = (peak_err(out, tensor(g["one.out64"])), bound("out"))
        figures["dfeats"] = (peak_err(f.grad, tensor(g["one.dfeats64"])), bound("dfeats"))
    else:
        chosen = torch.stack([xyz2[b][idx_c[b]] for b in range(B)])                    # (B, N, 3, 3)
        ref_chosen = torch.stack([xyz2[b][tensor(g[f"{case}.idx32"])[b]] for b in range(B)])
        assert bool(same_multiset(chosen, ref_chosen).all())
        dk = (xyz1.double()[:, :, None, :] - chosen.double()).square().sum(-1).sort(-1)[0]
        figures["d"] = (peak_err(dk, tensor(g[f"{case}.d64"]).sort(-1)[0]), bound("d"))
        figures["w"] = (peak_err(w_c.sort(-1)[0], tensor(g[f"{case}.w64"]).sort(-1)[0]), bound("w"))
        if case == "sequence":
            low = lowest_copies(xyz2, tensor(g["sequence.idx32"]))
            assert torch.equal(idx_c.sort(-1)[0], low)
            figures["out"] = (peak_err(out, gather_interp(feats, low, tensor(g["sequence.w64"]))), bound("out"))
            figures["dfeats"] = (peak_err(f.grad, scatter_interp(dout, low, tensor(g["sequence.w64"]), S)),
                                 bound("dfeats"))
        else:
            assert torch.equal(idx_c.sort(-1)[0], tensor(g[f"{case}.idx32"]).sort(-1)[0])
            figures["out"] = (peak_err(out, tensor(g[f"{case}.out64"])), bound("out"))
            figures["dfeats"] = (peak_err(f.grad, tensor(g[f"{case}.dfeats64"])), bound("dfeats"))
        # the gather and the scatter alone, on what the reference held
        ridx, rw = tensor(g[f"{case}.idx32"]), tensor(g[f"{case}.w32"])
        f2 = feats.to(device).requires_grad_(True)
        out2 = three_interpolate(f2, ridx.to(device).int(), rw.to(device))
        out2.backward(dout.to(device))
        figures["fed.out"] = (peak_err(out2, gather_interp(feats, ridx, rw)), bound("out"))
        figures["fed.out_vs_ref"] = (peak_err(out2, tensor(g[f"{case}.out64"])), bound("out"))
        figures["fed.dfeats"] = (peak_err(f2.grad, scatter_interp(dout, ridx, rw, S)), bound("dfeats"))
    for k, (err, b) in figures.items():
        print(f"PINNED interp.{case} {k}: err {err:.3e} bound {b:.3e}")
    assert all(err <= b for err, b in figures.values()), figures


def test_three_nn_bf16_features_equal_reference_propagation(device):
    """bf16 features through three_interpolate on the ``distinct`` case, against the float64 run: the project's 2e-2."""
    from helpers import peak_err
    from pinned_cases import BF16_INTERP, tensor
    from si_mamba_amd.interp import three_interpolate, three_nn
    g = load_golden("ref_seg_interp")
    idx, w = three_nn(tensor(g["xyz1"], device), tensor(g["distinct.xyz2"], device))
    out = three_interpolate(tensor(g["distinct.feats"], device).bfloat16(), idx, w)
    assert peak_err(out.float(), tensor(g["distinct.out64"])) < BF16_INTERP


def _fp_module(g, mode, device):
    from helpers import formula_parameters
    from si_mamba_amd.seg import PointNetFeaturePropagation
    fp = PointNetFeaturePropagation(3 + g["points2"].shape[-1], [int(v) for v in g["mlp"]])
    formula_parameters(fp, int(g["salt"]), running=(mode == "eval"))
    return fp.to(device).train(mode == "train")


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_feature_propagation_on_hip_equals_reference_module(mode, device):
    """si_mamba_amd.seg.PointNetFeaturePropagation (interp.hip, token GEMMs, bn_relu.hip) against the reference's module
    with the same formula parameters, MLP [32, 16], points1 = the points: forward, updated running statistics and every
    gradient of the reference's own float64 autograd (points2, conv weights and biases, BatchNorm weight and bias)."""
    from pinned_cases import assert_recorded, tensor
    g = load_golden("ref_seg_fp")
    fp = _fp_module(g, mode, device)
    B, N, _ = g["xyz1"].shape
    x1 = tensor(g["xyz1"], device)
    p2 = tensor(g["points2"], device).requires_grad_(True)
    out = fp(x1, tensor(g["xyz2"], device), x1, p2).view(B, N, -1)
    out.backward(tensor(g["dout"], device).transpose(1, 2).contiguous())
    got = {"out": out.detach(), "grad.points2": p2.grad}
    got.update({"grad." + k: p.grad for k, p in fp.named_parameters()})
    got.update({"stat." + k: b for k, b in fp.named_buffers() if "running" in k})
    assert_recorded(g, mode, got, report="fp." + mode)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_feature_propagation_bf16_equals_reference_module(mode, device):
    """The same forward under bf16 autocast against the float64 run: the project's 1e-2 on the normalised error."""
    from pinned_cases import BF16_HEAD, tensor
    g = load_golden("ref_seg_fp")
    fp = _fp_module(g, mode, device)
    B, N, _ = g["xyz1"].shape
    x1 = tensor(g["xyz1"], device)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = fp(x1, tensor(g["xyz2"], device), x1, tensor(g["points2"], device)).view(B, N, -1)
    err = nerr(out.float(), tensor(g[f"{mode}.out64"]))
    print(f"PINNED fp.{mode}.bf16 out: err {err:.3e}")
    assert err < BF16_HEAD


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("name", ["n32", "n16"])
def test_encoder_on_hip_equals_reference_encoder(name, mode, fused, device, monkeypatch):
    """si_mamba_amd.point_mamba.Encoder against the reference's Encoder (models/point_mamba.py:42-73) with the same formula
    parameters, 320 / 160 rows (more than one tile, no multiple of 256), one patch with a duplicated point: the fused
    route (bn_relu.hip, group max, the sparse last layer; asserted to have run) and the composed route.  Output, running
    statistics, parameter-gradient norms and samples, point gradients summed over the duplicated point."""
    from helpers import formula_parameters
    from pinned_cases import assert_recorded, encoder_results, tensor
    from si_mamba_amd import point_mamba
    g = load_golden("ref_encoder")
    calls = []
    real = point_mamba.token_linear_group_max
    monkeypatch.setattr(point_mamba, "token_linear_group_max", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    enc = formula_parameters(point_mamba.Encoder(int(g["encoder_channel"])), int(g["salt"]), running=(mode == "eval"))
    enc = enc.to(device).train(mode == "train")
    enc.fused = fused
    res = encoder_results(enc, tensor(g[f"{name}.points"], device), tensor(g[f"{name}.dout"], device), g["dup"])
    assert len(calls) == (1 if fused else 0)
    assert_recorded(g, f"{name}.{mode}", res, report=f"encoder.{name}.{mode}.{'fused' if fused else 'composed'}")


def test_encoder_bf16_equals_reference_encoder(device):
    """The fused encoder under bf16 autocast against the float64 run: the project's 1e-2."""
    from helpers import formula_parameters
    from pinned_cases import BF16_HEAD, tensor
    from si_mamba_amd.point_mamba import Encoder
    g = load_golden("ref_encoder")
    enc = formula_parameters(Encoder(int(g["encoder_channel"])), int(g["salt"]), running=True).to(device).eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = enc(tensor(g["n32.points"], device))
    err = nerr(out.float(), tensor(g["n32.eval.out64"]))
    print(f"PINNED encoder.n32.eval.bf16 out: err {err:.3e}")
    assert err < BF16_HEAD


def _partseg_from_fixture(g, mode, device):
    from helpers import formula_head
    from oracle.pin_from_reference import HEAD_DIMS as D
    from si_mamba_amd.seg import PartSegMamba, default_seg_config
    from pinned_cases import tensor
    cfg = default_seg_config(trans_dim=D["d"], depth=D["n_layer"], fetch_idx=D["fetch_idx"], num_group=D["L"],
                             group_size=8, drop_path=0., drop_path_rate=0.)
    m = PartSegMamba(D["cls_dim"], cfg)
    assert list(m.blocks.state_dict().keys()) == [str(n) for n in g["param_names"]]
    m.blocks.load_state_dict({str(n): tensor(g["param." + str(n)]) for n in g["param_names"]})
    formula_head(m, int(g["salt"]), running=(mode == "eval"))
    if mode == "train":
        m.dp1 = torch.nn.Dropout(0.0)                        # the fixture's train run has the dropout off
    return m.to(device).train(mode == "train")


def test_segmentation_taps_on_hip_equal_reference_mixer_model(device):
    """seg.MixerModelForSegmentation on the HIP mixers and add+norm kernels against the reference's
    MixerModelForSegmentation.forward (pt_mamba.py:390-416) over its own Block / create_block, MambaRef as the mixer
    (float64 run), same weights: the three taps."""
    from pinned_cases import assert_recorded, tensor
    g = load_golden("ref_seg_head")
    m = _partseg_from_fixture(g, "eval", device)
    with torch.no_grad():
        taps = m.blocks(tensor(g["x"], device), tensor(g["pos"], device))
    assert len(taps) == 3
    for i, t in enumerate(taps):
        assert_recorded(g, f"tap{i}", {"out": t}, report=f"head.tap{i}")


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_partseg_head_on_hip_equals_reference_head_statements(mode, device):
    """PartSegMamba.head (interp.hip, token GEMMs, bn_relu.hip with the per-sample additive term, N = 128 divides 256)
    against get_model.forward :768-787 as the reference ran it on the fixture's taps, formula parameters, distinct
    centres: log-probabilities and every BatchNorm's running statistics."""
    from pinned_cases import assert_recorded, tensor
    g = load_golden("ref_seg_head")
    m = _partseg_from_fixture(g, mode, device)
    taps = [tensor(g[f"tap{i}.32"], device) for i in range(3)]
    with torch.no_grad():
        out = m.head(tensor(g["pts"], device), tensor(g["cls_label"], device), tensor(g["sorted_center"], device), taps)
    got = {"out": out}
    heads = ("label_conv", "propagation_0", "bns1", "bns2")
    got.update({"stat." + k: b for k, b in m.named_buffers() if "running" in k and k.startswith(heads)})
    assert_recorded(g, mode, got, report="head." + mode)


def test_partseg_head_bf16_equals_reference_head_statements(device):
    """The head under bf16 autocast (eval) against the float64 run: the project's 1e-2.  The autocast roundings themselves
    stay unpinned (the reference's CUDA autocast cannot run here)."""
    from pinned_cases import BF16_HEAD, tensor
    g = load_golden("ref_seg_head")
    m = _partseg_from_fixture(g, "eval", device)
    taps = [tensor(g[f"tap{i}.32"], device) for i in range(3)]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = m.head(tensor(g["pts"], device), tensor(g["cls_label"], device), tensor(g["sorted_center"], device), taps)
    err = nerr(out.float(), tensor(g["eval.out64"]))
    print(f"PINNED head.eval.bf16 out: err {err:.3e}")
    assert err < BF16_HEAD


@pytest.mark.parametrize("kind", ["rand", "block"])
def test_mae_positions_equal_reference_index_maps(kind, device):
    """mae.masked_positions / sequence_positions on the device against the index maps the reference's own statements
    left on index-coded tokens (MaskMamba_2.forward :2453-2538, Point_MAE_Mamba.forward :3139-3202): the sorted masks,
    the visible / masked / full gathers with their reverse halves, where the visible tokens go back and where mask tokens
    stand, the final mask and the ground-truth patches -- bit for bit."""
    from si_mamba_amd import mae
    from pinned_cases import tensor
    g = load_golden("ref_mae_flow")
    B, G, k, M, C = (int(v) for v in g["dims"])
    orders, mask = tensor(g["orders"], device), tensor(g[f"mask_{kind}"], device)
    vis_pos, msk_pos, smask = mae.masked_positions(orders, mask)
    assert torch.equal(smask.cpu(), tensor(g[f"{kind}.sorted_mask"]))
    flipcat = lambda t: torch.cat([t, t.flip(1)], 1)                                   # noqa: E731
    vis_src = flipcat(torch.gather(orders, 2, vis_pos).reshape(B, -1))
    msk_src = flipcat(torch.gather(orders, 2, msk_pos).reshape(B, -1))
    full_src = flipcat(orders.reshape(B, k * G))
    assert torch.equal(vis_src.cpu() + 1, tensor(g[f"{kind}.x_vis_index"]))
    assert torch.equal(msk_src.cpu() + 1001, tensor(g[f"{kind}.pos_mask_index"]))
    assert torch.equal(full_src.cpu() + 1001, tensor(g[f"{kind}.pos_full_index"]))
    assert torch.equal(full_src.cpu() + 2001, tensor(g[f"{kind}.neighborhood_index"]))
    vis_seq = mae.sequence_positions(vis_pos, G, True)
    msk_seq = mae.sequence_positions(msk_pos, G, True)
    x_full = torch.full((B, 2 * k * G), -1, dtype=torch.int64, device=device).scatter(1, vis_seq, vis_src + 1)
    assert torch.equal(x_full.cpu(), tensor(g[f"{kind}.x_full_index"]))
    final = torch.zeros(B, 2 * k * G, dtype=torch.bool, device=device).scatter(1, msk_seq, True)
    assert torch.equal(final.cpu(), tensor(g[f"{kind}.final_mask"]))
    assert torch.equal(msk_seq.cpu(), torch.nonzero(tensor(g[f"{kind}.final_mask"]))[:, 1].view(B, -1))   # ascending
    assert torch.equal(msk_src.reshape(-1).cpu() + 2001, tensor(g[f"{kind}.gt_index"]))


def test_mae_block_mask_equals_reference_for_the_drawn_seed_patch(device, monkeypatch):
    """MaskMamba_2._mask_center_block on the device, its seed patch set to the one the reference's random.randint drew
    (:2217, recorded): the same mask_ratio * G nearest patches."""
    from si_mamba_amd.mae import MaskMamba_2, default_mae_config
    from pinned_cases import tensor
    g = load_golden("ref_mae_flow")
    B, G = g["mask_block"].shape
    enc = MaskMamba_2(default_mae_config(trans_dim=64, encoder_dims=64, depth=1, num_group=G, group_size=4,
                                         mask_ratio=float(g["mask_ratio"])))
    seed = tensor(g["block_seed_index"])
    monkeypatch.setattr(torch, "randint", lambda *a, **k: seed.clone())
    got = enc._mask_center_block(tensor(g["geometry"], device))
    assert torch.equal(got.cpu(), tensor(g["mask_block"]))


def test_mae_model_token_layout_equals_reference_index_maps(device):
    """Point_MAE_Mamba.forward on the device, given the fixture's orders and mask: the encoder / decoder token layout it
    builds (where visible tokens return, where mask tokens stand, which patches are rebuilt against which ground truth)
    equals the reference's index maps, and x_full holds the mask token exactly where the reference put one."""
    from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
    from pinned_cases import tensor
    g = load_golden("ref_mae_flow")
    B, G, k, M, C = (int(v) for v in g["dims"])
    torch.manual_seed(0)
    cfg = default_mae_config(trans_dim=64, encoder_dims=64, depth=1, decoder_depth=1, num_group=G, group_size=8,
                             k_top_eigenvectors=k, drop_path=0., mask_ratio=float(g["mask_ratio"]))
    m = Point_MAE_Mamba(cfg).to(device).eval()
    with torch.no_grad():
        m.mask_token.normal_(std=0.5)
        _, parts = m(clouds(B, 128, 3).to(device), orders=tensor(g["orders"], device),
                     mask=tensor(g["mask_rand"], device), return_parts=True)
    ref_full = tensor(g["rand.x_full_index"])
    assert torch.equal(parts["sorted_mask"].cpu(), tensor(g["rand.sorted_mask"]))
    assert torch.equal(parts["msk_src"].cpu() + 1001, tensor(g["rand.pos_mask_index"]))
    assert torch.equal(parts["vis_seq"].cpu(), torch.nonzero(ref_full != -1)[:, 1].view(B, -1))
    assert torch.equal(parts["msk_seq"].cpu(), torch.nonzero(tensor(g["rand.final_mask"]))[:, 1].view(B, -1))
    is_token = (parts["x_full"] == m.mask_token.to(parts["x_full"].dtype)).all(-1).cpu()
    assert torch.equal(is_token, ref_full == -1)
    # the rebuilt patches face the neighbourhoods of the reference's ground-truth selection
    nb = parts["neighborhood"]
    want_gt = torch.stack([nb[b, tensor(g["rand.gt_index"]).view(B, -1)[b].to(device) - 2001] for b in range(B)])
    assert torch.equal(parts["gt"], want_gt.reshape(parts["gt"].shape))
