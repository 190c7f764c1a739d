"""GPU: the mixing kernels (csrc/mix.hip, si_mamba_amd.mixing) against their numpy restatement (tests/mix_ref.py).

cutmix: everything is discrete and compared exactly -- the partner, the ratio, src, the order of the rows, the zero
tail -- and copied rows bit for bit.  pointwolf: the anchors exactly; the coordinates against float64 under the bound
mix_ref.pointwolf_cloud derives (u = 2^-24, V = max |f (p - a)|, Q = max |q_j|):
    8e-6 V + 2 sqrt(3) u V + 2 u Q      the project's 1e-6 bound on cos / sin and the 8e-6 max|v| rotation bound of
                                        test_gpu_corrupt.py, and the four roundings of the affine part
    Q (2 EPS_EXP + (M + 2) u)           the convex blend
EPS_EXP = 2 x 8.41e-8 = 1.682e-7: no bound for expf is documented in the toolchain's files, so tools/bench_mix.py
measured the largest relative error of the device library's expf against float64 on [-80, 0], the range the arguments
here stay in (asserted): 8.41e-8 (0.84 ulp) over 2^24 uniform and 2^22 log-uniform arguments; the figure is in
profiles/mix.json ("expf") and is doubled here.  The unit-sphere normalisation behind it is held to
dataset_ref.unit_sphere64's bound, as test_gpu_corrupt.py holds it.
The largest error / bound ratios are printed (run with -s) and recorded in profiles/mix.json by tools/bench_mix.py."""
import math

import numpy as np
import pytest
import torch

import mix_ref as mr
from dataset_ref import unit_sphere64
from guarded_alloc import SENTINEL, ZERO, guarded, place
from helpers import same_bits

pytestmark = pytest.mark.gpu

SEED, STEP = mr.SEED, mr.STEP
NAN = float("nan")
# lengths from {1, 7, 8, 9, 511, 512, 513, 8191, 8192}: the 8-row lane boundary, the wave boundary, the block limit.
# (lengths, partner or None, lam or None): None is drawn by the kernel.
CUT_CASES = {
    # m = 1 = n | m = 0 | the partner (7 rows) is shorter than (int)(8 * 1) | the partner has one row
    "lane": ((1, 7, 8, 9), (3, 0, 1, 0), (1.0, 0.0, 1.0, 1.0)),
    # m = 255 | m = 512 = n | (int)(513 * 0.999) = 512 > the partner's 511 rows
    "wave": ((511, 512, 513), (1, 2, 0), (0.5, 1.0, 0.999)),
    # m = 8191 = n | m = 4096 | a cloud with itself
    "block": ((8191, 8192, 9), (1, 0, 2), (1.0, 0.5, 0.5)),
    "lane-drawn": ((1, 7, 8, 9), None, None),
    "wave-drawn": ((511, 512, 513), None, None),
    "block-drawn": ((8191, 8192, 9), None, None),
    # B = 1: the cloud is its own partner, drawn and with everything replaced
    "alone": ((513,), None, None),
    "alone-all": ((513,), None, (1.0,)),
    # out-of-range partners and lambdas are clamped on the device: partner -> 0, 2, 1; lambda -> 0, 1, 0
    "clamped": ((9, 8, 7), (-5, 99, 1), (NAN, 2.0, -1.0)),
}
WOLF_PARAMS = dict(sigma=0.5, rot=math.radians(10), scale=3.0, trans=0.25)
WOLF_LENGTHS = [(1, 7, 8, 9), (511, 512, 513), (8191, 8192, 9)]
MEASURED = {}                        # "pointwolf" / "renorm" -> the largest error / bound seen


def M():
    from si_mamba_amd import mixing
    return mixing


def state_at(device, seed=SEED, step=STEP):
    from si_mamba_amd.transforms import AugmentState
    return AugmentState(seed, device).manual_seed(seed, step)


def padded(lengths, seed, fill=NAN, N=None):
    """(B, N, 3) float32 on the CPU: uniform in [-1, 1)^3, ``fill`` behind every length."""
    g = torch.Generator().manual_seed(seed)
    N = max(lengths) if N is None else N
    pts = torch.rand(len(lengths), N, 3, generator=g) * 2 - 1
    for b, n in enumerate(lengths):
        pts[b, n:] = fill
    return pts


def cut_inputs(case, device):
    lengths, partner, lam = CUT_CASES[case]
    pts = padded(lengths, seed=sum(lengths))
    kw = dict(lengths=torch.tensor(lengths, device=device))
    if partner is not None:
        kw["partner"] = torch.tensor(partner, device=device)
    if lam is not None:
        kw["lam"] = torch.tensor(lam, device=device, dtype=torch.float32)
    return pts, kw


def expected_cut(pts, lengths, partner, lam, mode, step=STEP):
    """The restatement of every cloud of the batch: (partners, [cutmix_cloud dict])."""
    B = len(lengths)
    q = [mr.clamp_partner(v, B) for v in partner] if partner is not None else mr.partner_map(B, SEED, step).tolist()
    res = [mr.cutmix_cloud(pts[b, :lengths[b]].numpy(), pts[q[b], :lengths[q[b]]].numpy(), mr.MODE[mode],
                           None if lam is None else lam[b], SEED, step, b) for b in range(B)]
    return q, res


def check_cut(pts, lengths, partner, lam, mode, got, step=STEP):
    out, prt, ratio, src = (t.cpu() for t in got)
    B, N = len(lengths), pts.shape[1]
    assert out.shape == (B, N, 3) and prt.dtype == torch.int64 and ratio.dtype == torch.float32
    assert src.dtype == torch.int32 and src.shape == (B, N)
    q, want = expected_cut(pts, lengths, partner, lam, mode, step)
    assert prt.tolist() == q, (prt.tolist(), q)
    for b, (n, r) in enumerate(zip(lengths, want)):
        assert ratio[b].numpy().view(np.uint32) == np.float32(r["ratio"]).view(np.uint32), (mode, b, n, r["m"])
        assert np.array_equal(src[b, :n].numpy(), r["src"]), (mode, b, n, r["m"])
        assert bool((src[b, n:] == mr.INT_MIN).all()), (mode, b, n)
        assert same_bits(out[b, :n], torch.from_numpy(r["out"])), (mode, b, n, r["m"])       # copies: bit for bit
        assert same_bits(out[b, n:], torch.zeros(N - n, 3)), (mode, b, n)
    return q, want


@pytest.mark.parametrize("mode", ["r", "k"])
@pytest.mark.parametrize("case", list(CUT_CASES))
def test_cutmix_against_the_restatement(device, case, mode):
    lengths, partner, lam = CUT_CASES[case]
    pts, kw = cut_inputs(case, device)
    dev_pts = pts.to(device)
    before = dev_pts.clone()
    st = state_at(device)
    got = M().cutmix(dev_pts, mode, state=st, return_src=True, **kw)
    q, want = check_cut(pts, lengths, partner, lam, mode, got)
    assert same_bits(dev_pts, before)                                # points is untouched
    assert st.step == STEP + 1 and st.seed == SEED
    print(f"cutmix-{mode} {case}: partners {q}, m = {[r['m'] for r in want]} of {list(lengths)}")
    if case == "alone":
        assert q == [0]
    if case == "alone-all":                                          # everything replaced by the cloud itself, in order
        assert same_bits(got[0][0, :513].cpu(), pts[0, :513]) and got[3][0, :513].tolist() == [-1 - i for i in range(513)]


def test_cutmix_cases_cover_the_edges():
    """Together the cases have m = 0, m = 1, m = n, a partner shorter than (int)(n lambda), a partner other than the
    cloud itself and a cloud that is its own partner -- by the restatement, which the test above holds the kernel to."""
    seen = set()
    for case, (lengths, partner, lam) in CUT_CASES.items():
        pts = padded(lengths, seed=sum(lengths))
        q, want = expected_cut(pts, lengths, partner, lam, "k")
        for b, (n, r) in enumerate(zip(lengths, want)):
            m, nq = r["m"], lengths[q[b]]
            seen |= {"m=0"} if m == 0 else set()
            seen |= {"m=1"} if m == 1 else set()
            seen |= {"m=n"} if m == n and n > 1 else set()
            seen |= {"short partner"} if m == nq < min(n, int(np.float32(n) * r["lam"])) else set()
            seen |= {"other"} if q[b] != b else {"self"}
            seen |= {"0<m<n"} if 0 < m < n else set()
    assert seen == {"m=0", "m=1", "m=n", "short partner", "other", "self", "0<m<n"}, seen


@pytest.mark.parametrize("mode", ["r", "k"])
def test_cutmix_exact_ties_go_to_the_lower_row(device, mode):
    """Three 5 x 5 x 5 lattices: test_mix_ref.py shows that the selection boundary of mode K cuts through a shell of
    equal distances on both sides of every cloud."""
    L = torch.from_numpy(mr.lattice(5))
    pts = torch.stack([L, L, L])
    partner, lam = (1, 2, 0), mr.LATTICE_LAM
    got = M().cutmix(pts.to(device), mode, state=state_at(device), return_src=True,
                     partner=torch.tensor(partner, device=device), lam=torch.tensor(lam, device=device))
    _, want = check_cut(pts, (125, 125, 125), partner, lam, mode, got)
    assert [r["m"] for r in want] == [25, 62, 87]


def wolf_run(pts, lengths, anchors, step=STEP, **kw):
    kw = {**WOLF_PARAMS, "renorm": False, **kw}
    return M().pointwolf(pts, anchors=anchors, lengths=lengths, state=state_at(pts.device, SEED, step),
                         return_anchors=True, **kw)


def check_wolf(pts, lengths, anchors, got, step=STEP, **kw):
    """``got`` = (out, anchor rows) of the un-normalised call against the restatement, cloud by cloud."""
    kw = {**WOLF_PARAMS, **kw}
    out, rows = (t.cpu() for t in got)
    N = pts.shape[1]
    assert rows.dtype == torch.int32 and rows.shape == (len(lengths), anchors)
    worst = 0.0
    for b, n in enumerate(lengths):
        r = mr.pointwolf_cloud(pts[b, :n].numpy(), anchors, [kw[k] for k in ("sigma", "rot", "scale", "trans")], SEED,
                               step, b)
        assert rows[b].tolist() == r["anchors"], (b, n, rows[b].tolist(), r["anchors"])
        assert r["args"].min() >= mr.EXP_ARG_MIN                     # the range EPS_EXP was measured on
        err = np.abs(out[b, :n].double().numpy() - r["out"]).max()
        assert err <= r["bound"], (b, n, anchors, err, r["bound"])
        worst = max(worst, err / r["bound"])
        assert same_bits(out[b, n:], torch.zeros(N - n, 3)), (b, n)
    MEASURED["pointwolf"] = max(MEASURED.get("pointwolf", 0.0), worst)
    print(f"pointwolf: lengths {tuple(lengths)}, {anchors} anchors, {kw}: worst error / bound = {worst:.3f}")
    return worst


@pytest.mark.parametrize("lengths", WOLF_LENGTHS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("anchors,sigma", [(1, 0.5), (4, 0.5), (8, 0.3)])
def test_pointwolf_against_the_restatement(device, lengths, anchors, sigma):
    pts = padded(lengths, seed=sum(lengths) + anchors)
    ln = torch.tensor(lengths, device=device)
    got = wolf_run(pts.to(device), ln, anchors, sigma=sigma)
    assert check_wolf(pts, lengths, anchors, got, sigma=sigma) <= 1.0


def test_pointwolf_anchor_ties_go_to_the_lower_row(device):
    """5 x 5 x 5 lattices and identical points: the farthest rows tie exactly at every step of the sampling."""
    pts = torch.full((3, 125, 3), NAN)
    pts[0] = torch.from_numpy(mr.lattice(5))
    pts[1] = torch.from_numpy(mr.lattice(5, 0.125))
    pts[2, :100] = torch.tensor([0.5, -0.25, 0.125])
    lengths = (125, 125, 100)
    got = wolf_run(pts.to(device), torch.tensor(lengths, device=device), 8)
    check_wolf(pts, lengths, 8, got)
    assert got[1][2].tolist() == [got[1][2, 0].item()] + [0] * 7     # identical points: every distance is 0, row 0 wins


@pytest.mark.parametrize("lengths", WOLF_LENGTHS[:2], ids=lambda v: "-".join(map(str, v)))
def test_pointwolf_renorm_within_the_dataset_routine_bound(device, lengths):
    """RENORM is pc_norm of the call's own result: the un-normalised call at the same [seed, step] gives its input bit
    for bit, unit_sphere64 the float64 answer and the bound of the fp32 routine."""
    pts = padded(lengths, seed=5).to(device)
    ln = torch.tensor(lengths, device=device)
    raw, rows = wolf_run(pts, ln, 4)
    out, rows2 = wolf_run(pts, ln, 4, renorm=True)
    assert torch.equal(rows, rows2)
    worst = 0.0
    for b, n in enumerate(lengths):
        want, bound = unit_sphere64(raw[b, :n].double().cpu().numpy())
        err = np.abs(out[b, :n].double().cpu().numpy() - want).max()
        assert err <= bound, (b, n, err, bound)
        worst = max(worst, err / bound if bound > 0 else 0.0)        # a single row: zeros, and a bound of zero
        assert same_bits(out[b, n:].cpu(), torch.zeros(out.shape[1] - n, 3))
    MEASURED["renorm"] = max(MEASURED.get("renorm", 0.0), worst)
    print(f"renorm after pointwolf, lengths {tuple(lengths)}: worst error / bound = {worst:.3f}")
    dflt = M().pointwolf(pts, lengths=ln, state=state_at(device))    # renorm is the default, 4 anchors too
    assert same_bits(dflt, out)


def test_pointwolf_in_place_equals_out_of_place(device):
    lengths = (511, 512, 513)
    pts = padded(lengths, seed=17, fill=7.0).to(device)
    ln = torch.tensor(lengths, device=device)
    for renorm in (False, True):
        want, rows = wolf_run(pts, ln, 4, renorm=renorm)
        mine = pts.clone()
        st = state_at(device)
        back = M().pointwolf(mine, lengths=ln, state=st, out=mine, renorm=renorm)
        assert back is mine and same_bits(mine, want) and st.step == STEP + 1
        assert not same_bits(want, pts)


def test_same_state_same_bits_and_the_step_advances(device):
    lengths = (200, 129, 64, 250)
    pts = padded(lengths, seed=12).to(device)
    ln = torch.tensor(lengths, device=device)
    st = state_at(device)
    calls = {
        "cutmix-r": lambda: M().cutmix(pts, "r", lengths=ln, state=st, return_src=True),
        "cutmix-k": lambda: M().cutmix(pts, "k", lengths=ln, state=st, return_src=True),
        "pointwolf": lambda: M().pointwolf(pts, lengths=ln, state=st, return_anchors=True),
    }
    for name, call in calls.items():
        st.manual_seed(SEED, STEP)
        first = call()
        assert st.step == STEP + 1 and st.seed == SEED, name
        later = call()                                               # the next step: other draws
        assert st.step == STEP + 2 and not same_bits(later[0], first[0]), name
        st.manual_seed(SEED, STEP)
        for a, b in zip(first, call()):
            assert same_bits(a, b), name
    # the partner map and lambdas of draw_pairs are the kernel's, and drawing them moves nothing
    st.manual_seed(SEED, STEP)
    prt, lam = M().draw_pairs(4, st)
    assert st.step == STEP and prt.tolist() == mr.partner_map(4, SEED, STEP).tolist()
    assert lam.cpu().numpy().view(np.uint32).tolist() == \
        [int(np.float32(mr.lam_of(None, SEED, STEP, b)).view(np.uint32)) for b in range(4)]
    a = M().cutmix(pts, "k", lengths=ln, state=st, return_src=True)
    st.manual_seed(SEED, STEP)
    b = M().cutmix(pts, "k", lengths=ln, state=st, return_src=True, partner=prt, lam=lam)
    for x, y in zip(a, b):
        assert same_bits(x, y)
    # corrupt and augment draw from other streams at the same state
    from si_mamba_amd import corruptions
    st.manual_seed(SEED, STEP)
    _, _, csrc = corruptions.corrupt(pts, "drop_global", ratio=0.5, lengths=ln, state=st, return_src=True)
    st.manual_seed(SEED, STEP)
    lam_half = torch.full((4,), 0.5, device=device)
    _, _, _, msrc = M().cutmix(pts, "r", lengths=ln, state=st, return_src=True, lam=lam_half,
                               partner=torch.arange(4, device=device))
    kept_c = [set(csrc[b][csrc[b] >= 0].tolist()) for b in range(4)]
    kept_m = [set(msrc[b][msrc[b] >= 0].tolist()) for b in range(4)]
    assert all(len(kept_c[b]) == len(kept_m[b]) for b in range(4)) and kept_c != kept_m


def test_captured_graph_draws_anew_at_every_replay(device):
    lengths = (256, 200, 129, 256)
    pts = padded(lengths, seed=30).to(device)
    ln = torch.tensor(lengths, device=device)
    st = state_at(device)
    out = torch.empty(4, 256, 3, device=device)
    wolf = torch.empty(4, 256, 3, device=device)

    def step():
        mixed = M().cutmix(pts, "k", lengths=ln, state=st, out=out, return_src=True)
        return mixed + (M().pointwolf(mixed[0], lengths=ln, state=st, out=wolf),)

    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize()
    st.manual_seed(SEED, STEP)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = step()
    seen = []
    for _ in range(2):
        graph.replay()
        seen.append([t.clone() for t in res])
    torch.cuda.synchronize()
    assert st.step == STEP + 4                                       # two calls per replay, one step each
    assert not same_bits(seen[0][1], seen[1][1]) and not same_bits(seen[0][3], seen[1][3])
    st.manual_seed(SEED, STEP)
    for k in range(2):
        mixed = M().cutmix(pts, "k", lengths=ln, state=st, return_src=True)
        eager = mixed + (M().pointwolf(mixed[0], lengths=ln, state=st),)
        for a, b in zip(eager, seen[k]):
            assert same_bits(a, b), k
    assert st.step == STEP + 4


@pytest.mark.parametrize("what", ["cutmix-r", "cutmix-k", "pointwolf"])
def test_memory_contract(device, what):
    """Guard bands around every output stay intact, every element is written, and neither what lies behind an input
    cloud's length nor what the outputs held before is read: two poisons, the same bits."""
    lengths = (1024, 65, 1023)
    got = []
    for poison, fill in ((ZERO, NAN), (SENTINEL, 7.0)):
        pts = padded(lengths, seed=21, fill=fill).to(device)
        with guarded(poison) as g:
            p, ln = place(pts), place(torch.tensor(lengths, device=device))
            if what == "pointwolf":
                res = M().pointwolf(p, lengths=ln, state=state_at(device), return_anchors=True)
                assert len(g.records) == 4                           # the two placed inputs, out, the anchor rows
            else:
                res = M().cutmix(p, what[-1], lengths=ln, state=state_at(device), return_src=True)
                assert len(g.records) == 6                           # the two placed inputs, partner, out, ratio, src
            g.verify()
        got.append(res)
    for a, b in zip(*got):
        assert same_bits(a, b)
    assert bool(torch.isfinite(got[0][0]).all())


def test_python_route_refuses_what_it_documents(device):
    pts = padded((16, 16), seed=1).to(device)
    with pytest.raises(ValueError, match="mode"):
        M().cutmix(pts, "x")
    with pytest.raises(RuntimeError, match="SIMAMBA_E_VARIANT|variant"):
        M().cutmix(pts, "k", out=pts)                                # out over points
    with pytest.raises(TypeError, match="lam"):
        M().cutmix(pts, "k", lam=0.5)
    with pytest.raises(ValueError, match="lam"):
        M().cutmix(pts, "k", lam=torch.zeros(3, device=device))
    with pytest.raises(ValueError, match="anchors"):
        M().pointwolf(pts, anchors=9)
    with pytest.raises(ValueError, match="sigma"):
        M().pointwolf(pts, sigma=0.0)
    with pytest.raises(RuntimeError, match="grad"):
        M().cutmix(pts.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="1024"):
        M().mixup(torch.zeros(2, 1025, 3, device=device))
    with pytest.raises(TypeError, match="state"):
        M().pointwolf(pts, state=object())


def test_mixup_is_gather_and_lerp_of_a_permutation(device):
    g = torch.Generator().manual_seed(4)
    pts = (torch.rand(5, 200, 3, generator=g) * 2 - 1).to(device)
    st = state_at(device)
    out, partner, lam = M().mixup(pts, state=st)
    assert st.step == STEP + 1
    assert partner.tolist() == mr.partner_map(5, SEED, STEP).tolist()
    assert lam.cpu().numpy().view(np.uint32).tolist() == \
        [int(np.float32(mr.lam_of(None, SEED, STEP, b)).view(np.uint32)) for b in range(5)]
    from si_mamba_amd import earth_movers_distance
    b = pts[partner]
    _, assign, _, _ = earth_movers_distance(pts, b, return_assignment=True)
    assert all(sorted(assign[k].tolist()) == list(range(200)) for k in range(5))
    want = pts + lam.view(5, 1, 1) * (torch.gather(b, 1, assign.long().unsqueeze(-1).expand(5, 200, 3)) - pts)
    assert same_bits(out, want)
    # given partners and lambdas: clamped as the kernels clamp them; lambda 0 is the cloud, lambda 1 its partner's rows
    lam2 = torch.tensor([0.0, 1.0, NAN, 2.0, 0.5], device=device)
    prt2 = torch.tensor([1, 2, 3, 99, -1], device=device)
    out2, p2, l2 = M().mixup(pts, state=st, lam=lam2, partner=prt2)
    assert st.step == STEP + 2 and p2.tolist() == [1, 2, 3, 4, 0] and l2.tolist() == [0.0, 1.0, 0.0, 1.0, 0.5]
    assert same_bits(out2[0], pts[0]) and same_bits(out2[2], pts[2])
    moved = out2[1].cpu()
    assert sorted(map(tuple, moved.tolist())) == pytest.approx(sorted(map(tuple, pts[2].cpu().tolist())), abs=1e-6)


def test_mixed_cross_entropy_and_its_gradient(device):
    g = torch.Generator().manual_seed(6)
    logits = torch.randn(8, 5, generator=g).to(device).requires_grad_(True)
    labels = torch.randint(0, 5, (8,), generator=g).to(device)
    pts = padded((64,) * 8, seed=2).to(device)
    _, partner, ratio = M().cutmix(pts, "k", state=state_at(device))
    loss = M().mixed_cross_entropy(logits, labels, partner, ratio)
    F = torch.nn.functional
    want = ((1 - ratio) * F.cross_entropy(logits, labels, reduction="none")
            + ratio * F.cross_entropy(logits, labels[partner], reduction="none")).mean()
    assert same_bits(loss.detach(), want.detach())
    g1, = torch.autograd.grad(loss, logits)
    g2, = torch.autograd.grad(want, logits)
    assert same_bits(g1, g2)
    # against float64 on the host: the formula itself
    lp = torch.log_softmax(logits.detach().double().cpu(), -1)
    r, y, q = ratio.double().cpu(), labels.cpu(), partner.cpu()
    ref = -((1 - r) * lp[torch.arange(8), y] + r * lp[torch.arange(8), y[q]]).mean()
    assert abs(loss.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
