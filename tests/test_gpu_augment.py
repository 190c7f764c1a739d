"""GPU: sampling + augmentation in one launch (csrc/augment.hip, si_mamba_amd/transforms.py) against the numpy
restatement of augment_ref.py.

Bounds (none of them fitted to what the kernel gives):
  * every value derived from uniforms by single fp32 operations -- theta, s, t, ratio, the flip bits, the keep mask --
    equals the restatement bit for bit;
  * cos / sin agree with float64 of the same fp32 theta within 1e-6 (an accurate sincosf is a few ulp of a value <= 1,
    about 2.4e-7: 4x margin);
  * the normals agree within 1e-5 (|n| <= 5.8; about ten fp32 roundings plus the cosine's error is 3.5e-6: 3x margin);
  * the points of a chain of T ops agree with the float64 chain, applied with the kernel's own emitted fp32 parameters,
    within 4 T 2^-24 max|value met in the float64 chain|: four roundings per op.
Measured on an MI355X (profiles/augment.json): cos / sin 4.44e-8, normals 5.20e-7, points at most 0.359 of their bound.
"""
import numpy as np
import pytest
import torch

import augment_ref as ar
from augment_ref import DIST_B, DIST_N, DIST_SEED
from helpers import same_bits

pytestmark = pytest.mark.gpu

SEED = 0xa4093822299f31d0            # both key words in use
STEP = (0x0123456 << 32) | 0xfffffffe   # both step words in use, and the low word wraps within a few calls
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 8192]   # wave boundary, one point per lane boundary, register limit


def T():
    from si_mamba_amd import transforms
    return transforms


def all_ops():
    t = T()
    return [t.PointcloudRotate(), t.PointcloudScale(), t.PointcloudTranslate(), t.PointcloudScaleAndTranslate(),
            t.PointcloudJitter(), t.PointcloudRandomInputDropout(), t.RandomHorizontalFlip(),
            t.RandomHorizontalFlip("x")]


def five():
    t = T()
    return [t.PointcloudRotate(), t.PointcloudScaleAndTranslate(), t.PointcloudJitter(),
            t.PointcloudRandomInputDropout(), t.RandomHorizontalFlip()]


def chains():
    t = T()
    singles = {type(x).__name__: [x] for x in all_ops()[:7]}
    singles["flip_y_up"] = [t.RandomHorizontalFlip("y")]
    return {**singles,
            "finetune": [t.PointcloudScaleAndTranslate()],                                  # runner_finetune.py:23-33
            "scale_then_translate": [t.PointcloudScale(), t.PointcloudTranslate()],
            "rotate_scale_translate": [t.PointcloudRotate(), t.PointcloudScaleAndTranslate()],
            "five": five()}


def ref_chain(transforms):
    return [t.op() for t in transforms]


def uniform_clouds(B, N, seed, device):
    """Points uniform in the cube [-1, 1)^3."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, N, 3, generator=g) * 2 - 1).to(device)


def state_at(device, seed=SEED, step=STEP):
    return T().AugmentState(seed, device).manual_seed(seed, step)


def run(points, transforms, step=STEP, seed=SEED, **kw):
    return T().sample_and_augment(points, transforms, state=state_at(points.device, seed, step), **kw)


# ---- the drawn parameters --------------------------------------------------------------------------------------------
UNIFORM_DERIVED = {ar.ROTATE: [0], ar.SCALE: [0, 1, 2], ar.TRANSLATE: [0, 1, 2], ar.SCALE_TRANSLATE: [0, 1, 2, 3, 4, 5],
                   ar.JITTER: [0, 1], ar.DROPOUT: [0], ar.FLIP: [0, 1, 2, 3]}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", SIZES)
def test_parameters_against_the_restatement(device, N, B):
    tr = all_ops()
    chain = ref_chain(tr)
    cloud, noise, keep = T().augment_params(tr, B, N, state=state_at(device), noise=True, keep=True)
    cloud, noise, keep = cloud.cpu().numpy(), noise.cpu().numpy(), keep.cpu().numpy()
    want = ar.cloud_params(SEED, STEP, B, chain)
    assert cloud.shape == want.shape == (B, 8, 8)
    for o, (op, _) in enumerate(chain):
        cols = UNIFORM_DERIVED[op]
        assert np.array_equal(cloud[:, o, cols].view(np.uint32), want[:, o, cols].astype(np.float32).view(np.uint32)), op
        rest = [c for c in range(8) if c not in cols and not (op == ar.ROTATE and c in (1, 2))]
        assert not cloud[:, o, rest].any()
    trig = np.abs(cloud[:, 0, 1:3].astype(np.float64) - want[:, 0, 1:3]).max()
    normals = np.stack([ar.point_normals(SEED, STEP, b, 4, N) for b in range(B)])
    nerr = np.abs(noise.astype(np.float64) - normals).max()
    print(f"augment N={N} B={B}: cos/sin deviation {trig:.3e} (bound 1e-6), normals {nerr:.3e} (bound 1e-5)")
    assert trig <= 1e-6
    assert nerr <= 1e-5
    for b in range(B):
        assert np.array_equal(keep[b], ar.keep_mask(SEED, STEP, b, 5, N, cloud[b, 5, 0]))


def test_parameters_do_not_advance_the_step_and_skip_the_padding(device):
    tr = five()
    st = state_at(device)
    lengths = torch.tensor([1, 40, 65], device=device)
    cloud, noise, keep = T().augment_params(tr, 3, 65, state=st, lengths=lengths, noise=True, keep=True)
    full = T().augment_params(tr, 3, 65, state=st, noise=True, keep=True)
    assert st.step == STEP and st.seed == SEED
    assert same_bits(cloud, full[0])
    for b, n in enumerate([1, 40, 65]):
        assert same_bits(noise[b, :n], full[1][b, :n]) and not noise[b, n:].any()
        assert torch.equal(keep[b, :n], full[2][b, :n]) and not keep[b, n:].any()


# ---- the points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", SIZES)
def test_points_against_the_float64_chain(device, N, B):
    pts = uniform_clouds(B, N, N, device)
    host = pts.cpu().numpy()
    worst = 0.0
    for name, tr in chains().items():
        chain = ref_chain(tr)
        cloud, noise, keep = T().augment_params(tr, B, N, state=state_at(device), noise=True, keep=True)
        got = run(pts, tr).cpu().numpy()
        cloud, noise, keep = cloud.cpu().numpy(), noise.cpu().numpy(), keep.cpu().numpy()
        ops = [op for op, _ in chain]
        for b in range(B):
            want, big = ar.apply_chain(host[b], chain, cloud[b], noise[b], keep[b])
            bound = 4 * len(chain) * 2.0 ** -24 * big
            err = np.abs(got[b].astype(np.float64) - want).max()
            worst = max(worst, err / bound)
            assert err <= bound, (name, b, err, bound)
            if ar.DROPOUT in ops:
                # dropped rows ARE row 0 (whatever follows treats equal rows equally), and row 0 was its own source
                assert (got[b][~keep[b]].view(np.uint32) == got[b][0].view(np.uint32)[None, :]).all(), name
            if ops == [ar.DROPOUT]:
                assert np.array_equal(got[b][0].view(np.uint32), host[b][0].view(np.uint32))
                assert np.array_equal(got[b][keep[b]].view(np.uint32), host[b][keep[b]].view(np.uint32))
    print(f"augment N={N} B={B}: largest point deviation / bound {worst:.3f}")


def test_points_agree_with_the_restatements_own_draws(device):
    """End to end with nothing taken from the library: the restatement draws, the kernel draws, the clouds agree within
    the chain's bound plus what the 1e-5 of the normals and the 1e-6 of cos / sin can move a point."""
    tr, B, N = five(), 2, 200
    pts = uniform_clouds(B, N, 3, device)
    got = run(pts, tr).cpu().numpy()
    for b in range(B):
        want, big = ar.reference_cloud(pts[b].cpu().numpy(), ref_chain(tr), SEED, STEP, b)
        bound = 4 * 5 * 2.0 ** -24 * big + 1.5 * (0.01 * 1e-5 + 2 * 1e-6 * big)   # scale <= 1.5 behind both
        assert np.abs(got[b] - want).max() <= bound


# ---- layout independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [65, 1025])
def test_a_cloud_does_not_depend_on_the_batch(device, N):
    tr = five()
    pts = uniform_clouds(3, N, 5, device)
    whole = run(pts, tr)
    for b in range(3):
        assert same_bits(run(pts[:b + 1].contiguous(), tr)[b], whole[b])
        poisoned = torch.full_like(pts, float("nan"))
        poisoned[b] = pts[b]
        assert same_bits(run(poisoned, tr)[b], whole[b])


# ---- lengths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [float("nan"), 1e30])
def test_lengths(device, fill):
    tr, N = five(), 1025
    lens = [1, 700, 1025]
    pts = uniform_clouds(3, N, 6, device)
    padded = pts.clone()
    for b, n in enumerate(lens):
        padded[b, n:] = fill                                 # flip's maximum must not see it
    lengths = torch.tensor(lens, device=device)
    got = run(padded, tr, lengths=lengths)
    for b, n in enumerate(lens):
        alone = run(pts[:b + 1, :n].contiguous(), tr)        # the same cloud index, the cloud at its true size
        assert same_bits(got[b, :n], alone[b])
        assert not got[b, n:].any() and not torch.isnan(got[b]).any()
    # the same through a gather: padded index slots are never looked up (they point outside the cloud here)
    idx = torch.arange(N, device=device).expand(3, N).clone()
    for b, n in enumerate(lens):
        idx[b, n:] = 1 << 40
    assert same_bits(run(padded, tr, idx=idx, lengths=lengths), got)
    assert same_bits(run(padded, tr, lengths=lengths.int()), got)


# ---- fusion ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,K", [(2048, 1200, 1024), (65, 65, 65), (300, 65, 65)])
def test_fused_gather_and_subset(device, N, M, K):
    tr, B = five(), 3
    pts = uniform_clouds(B, N, 7, device)
    g = torch.Generator().manual_seed(N + M)
    idx = torch.stack([torch.randperm(N, generator=g)[:M] for _ in range(B)]).to(device)
    sel = torch.randperm(M, generator=g)[:K].to(device)
    gathered = torch.gather(pts, 1, idx[:, sel].unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    want = run(gathered, tr)
    assert same_bits(run(pts, tr, idx=idx, sel=sel), want)
    assert same_bits(run(pts, tr, idx=idx.int(), sel=sel.int()), want)
    # each alone: idx without sel takes every column, sel without idx selects rows of the cloud
    assert same_bits(run(pts, tr, idx=idx[:, sel].contiguous()), want)
    rows = torch.gather(pts, 1, sel.view(1, -1, 1).expand(B, -1, 3)).contiguous()
    assert same_bits(run(pts, tr, sel=sel), run(rows, tr))
    # no chain: the plain gather, and the step still advances
    st = state_at(device)
    assert same_bits(T().sample_and_augment(pts, None, idx=idx, sel=sel, state=st), gathered) and st.step == STEP + 1
    with pytest.raises(ValueError):
        T().sample_and_augment(pts, tr, sel=torch.arange(N, device=device), out=pts)


@pytest.mark.parametrize("N", [65, 8192])
def test_in_place_equals_out_of_place(device, N):
    tr = five()
    pts = uniform_clouds(2, N, 8, device)
    want = run(pts, tr)
    work = pts.clone()
    assert run(work, tr, out=work) is work and same_bits(work, want)
    out = torch.empty_like(pts)
    assert run(pts, tr, out=out) is out and same_bits(out, want)
    # the classes work in place and return their argument, as the reference's do; Compose is one launch
    work = pts.clone()
    st = state_at(device)
    assert T().Compose(tr)(work, state=st) is work and same_bits(work, want) and st.step == STEP + 1
    work, st = pts.clone(), state_at(device)
    assert tr[1](work, state=st) is work and same_bits(work, run(pts, [tr[1]]))
    # a strided view goes through a copy and lands in the view
    wide = torch.zeros(2, N, 6, device=device)
    wide[..., :3] = pts
    view = wide[..., :3]
    assert run(view, tr, out=view) is view and same_bits(wide[..., :3].contiguous(), want) and not wide[..., 3:].any()


def test_compose_runs_foreign_callables_between_launches(device):
    t = T()
    pts = uniform_clouds(2, 100, 9, device)
    calls = []

    def foreign(pc):
        calls.append(pc.data_ptr())
        return pc * 2

    st = state_at(device)
    work = pts.clone()
    got = t.Compose([t.PointcloudRotate(), foreign, t.PointcloudJitter(), t.RandomHorizontalFlip()])(work, state=st)
    assert got is work and len(calls) == 1 and st.step == STEP + 2           # two launches, two steps
    a = run(pts, [t.PointcloudRotate()], step=STEP)
    want = run(a * 2, [t.PointcloudJitter(), t.RandomHorizontalFlip()], step=STEP + 1)
    assert same_bits(got, want)
    with pytest.raises(RuntimeError, match="require grad"):
        t.PointcloudRotate()(pts.clone().requires_grad_(True))
    with pytest.raises(TypeError):
        t.sample_and_augment(pts, [foreign])
    with pytest.raises(ValueError):
        t.sample_and_augment(pts, [t.PointcloudRotate()] * 9)


# ---- state -----------------------------------------------------------------------------------------------------------
def test_state(device):
    t = T()
    tr = five()
    pts = uniform_clouds(2, 130, 10, device)
    st = t.AugmentState(1234, device)
    assert (st.seed, st.step) == (1234, 0)
    a = t.sample_and_augment(pts, tr, state=st)
    assert st.step == 1
    b = t.sample_and_augment(pts, tr, state=st)
    assert st.step == 2 and st.seed == 1234
    assert not same_bits(a, b)
    st.manual_seed(1234)
    assert (st.seed, st.step) == (1234, 0)
    assert same_bits(t.sample_and_augment(pts, tr, state=st), a)
    assert same_bits(t.sample_and_augment(pts, tr, state=st), b)
    assert not same_bits(t.sample_and_augment(pts, tr, state=t.AugmentState(1235, device)), a)
    # the step is 64 bits wide: the low word carries into the high one, which is part of the counter
    st.manual_seed(1234, (1 << 32) - 1)
    c = t.sample_and_augment(pts, tr, state=st)
    assert st.step == 1 << 32
    d = t.sample_and_augment(pts, tr, state=st)
    st.manual_seed(1234, 0)
    assert not same_bits(t.sample_and_augment(pts, tr, state=st), d) and not same_bits(c, d)
    # the default state: one per device, used when none is given
    dflt = t.default_state(device)
    before = dflt.step
    t.PointcloudScale()(pts.clone())
    assert dflt.step == before + 1 and t.default_state(device) is dflt


# ---- capture ---------------------------------------------------------------------------------------------------------
def small_model(device):
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    cfg = default_config(trans_dim=32, encoder_dims=32, depth=2, num_group=16, group_size=8, drop_path=0.,
                         knn_graph=8, cls_dim=5)
    return PointMamba(cfg).to(device).eval()


def test_captured_graph_draws_anew_at_every_replay(device):
    t = T()
    tr = five()
    model = small_model(device)
    pts = uniform_clouds(2, 128, 11, device)
    st = t.AugmentState(77, device)
    aug = torch.empty_like(pts)

    def step():
        return model(t.sample_and_augment(pts, tr, state=st, out=aug))

    with torch.no_grad():
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.synchronize()
        start = st.step
        assert start == 1
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            logits = step()
        seen, outs = [], []
        for _ in range(3):
            graph.replay()
            seen.append(aug.clone())
            outs.append(logits.clone())
        torch.cuda.synchronize()
        assert st.step == start + 3
        assert not same_bits(seen[0], seen[1]) and not same_bits(seen[1], seen[2]) and not same_bits(seen[0], seen[2])
        st.manual_seed(77, start)
        for k in range(3):
            eager = t.sample_and_augment(pts, tr, state=st)
            assert same_bits(eager, seen[k]), k
            assert torch.allclose(model(eager), outs[k], rtol=1e-4, atol=1e-4)
        assert st.step == start + 3


# ---- distribution: a sanity net, not a proof -------------------------------------------------------------------------
def test_distribution(device):
    """Four standard errors; test_augment_abi.py confirms on the CPU that this seed meets them under the restatement."""
    t = T()
    tr = [t.PointcloudJitter(), t.PointcloudRandomInputDropout()]
    _, noise, keep = t.augment_params(tr, DIST_B, DIST_N, state=t.AugmentState(DIST_SEED, device), noise=True, keep=True)
    cloud = t.augment_params(tr, DIST_B, DIST_N, state=t.AugmentState(DIST_SEED, device))[0]
    z = noise.double().flatten()
    n = z.numel()
    assert n == 196608
    assert abs(z.mean().item()) <= 4 / np.sqrt(n)
    assert abs(z.var(unbiased=False).item() - 1) <= 4 * np.sqrt(2 / n)
    ratio = cloud[:, 1, 0].double().cpu().numpy()
    frac = 1 - keep.double().mean(1).cpu().numpy()
    assert (ratio >= 0).all() and (ratio < 0.5).all()
    assert (np.abs(frac - ratio) <= 4 * np.sqrt(np.maximum(ratio * (1 - ratio), 1e-12) / DIST_N)).all()


# ---- voting ----------------------------------------------------------------------------------------------------------
def test_vote_logits_equals_the_loop_written_out(device):
    from si_mamba_amd import grouping, vote_logits
    t = T()
    model = small_model(device)
    raw = uniform_clouds(2, 300, 12, device)
    npoints, point_all, times = 128, 160, 3
    st = t.AugmentState(5, device)
    torch.manual_seed(21)
    got = vote_logits(model, raw, npoints, times=times, point_all=point_all, state=st)
    assert got.shape == (2, 5) and st.step == times

    st.manual_seed(5)
    torch.manual_seed(21)
    with torch.no_grad():
        fps_idx = grouping.sample_farthest_points(raw, point_all)[1]
        total = None
        for _ in range(times):
            sel = torch.randperm(point_all, device=device)[:npoints]
            pts = torch.gather(raw, 1, fps_idx[:, sel].unsqueeze(-1).expand(-1, -1, 3)).contiguous()
            pts = t.PointcloudScaleAndTranslate()(pts, state=st)
            logits = model(pts)
            total = logits if total is None else total + logits
        want = total / times
    assert same_bits(got, want)
    # the reference's table, capped at the cloud: 1024 -> 1200 of a cloud of 1100 is all 1100
    from si_mamba_amd.vote import POINT_ALL
    assert POINT_ALL == {1024: 1200, 2048: 2400, 4096: 4800, 8192: 8192}
    with pytest.raises(NotImplementedError):
        vote_logits(model, raw, 100)
    with pytest.raises(ValueError):
        vote_logits(model, raw, 1024)                        # 300 points cannot give 1024


# ---- the pointnet2_ops stand-in --------------------------------------------------------------------------------------
def test_pointnet2_stand_in(device):
    import sys
    from si_mamba_amd import grouping, install_shim
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] == "pointnet2_ops"}
    try:
        install_shim(pointnet2=True)
        from pointnet2_ops import pointnet2_utils
        pts = uniform_clouds(2, 300, 13, device)
        fps = pointnet2_utils.furthest_point_sample(pts, 40)
        assert fps.dtype == torch.int32 and fps.shape == (2, 40)
        assert torch.equal(fps.long(), grouping.sample_farthest_points(pts, 40)[1])
        # the runner's three lines, against the fused call
        sel = torch.randperm(40, device=device)[:32]
        picked = pointnet2_utils.gather_operation(pts.transpose(1, 2).contiguous(), fps[:, sel].contiguous())
        picked = picked.transpose(1, 2).contiguous()
        assert same_bits(picked, T().sample_and_augment(pts, None, idx=fps, sel=sel))
        # gather_operation and its gradient against torch.gather, (2, 3, 65) -> K = 17, with repeated indices
        g = torch.Generator().manual_seed(0)
        feats = torch.randn(2, 3, 65, generator=g).to(device)
        idx = torch.randint(0, 65, (2, 17), generator=g).to(device)
        idx[:, 1] = idx[:, 0]
        w = torch.randn(2, 3, 17, generator=g).to(device)
        a = feats.clone().requires_grad_(True)
        b = feats.clone().requires_grad_(True)
        ya = pointnet2_utils.gather_operation(a, idx.int())
        yb = torch.gather(b, 2, idx.unsqueeze(1).expand(-1, 3, -1))
        assert torch.equal(ya, yb)
        (ya * w).sum().backward()
        (yb * w).sum().backward()
        # sums of at most 17 fp32 terms of |w| < 6 in a different order: 17 * 2^-24 * 6 * 17 < 2e-4; equal in practice
        assert torch.allclose(a.grad, b.grad, rtol=0, atol=2e-4)
        dense = torch.zeros_like(feats)
        for k in range(17):
            dense[torch.arange(2, device=device), :, idx[:, k]] += w[:, :, k]
        assert torch.allclose(a.grad, dense, rtol=0, atol=2e-4)
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] == "pointnet2_ops"]:
            del sys.modules[k]
        sys.modules.update(saved)
