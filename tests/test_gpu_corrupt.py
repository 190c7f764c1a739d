"""GPU: the corruption kernel (csrc/corrupt.hip, si_mamba_amd.corruptions) against its numpy restatement
(tests/corrupt_ref.py).

What is discrete -- the output lengths, which rows go, in which order the rest stands, which cluster an added point
belongs to, the zero tail -- is compared exactly, and copied rows bit for bit.  What passes through cos / sin / cbrt /
log is compared with float64 under bounds that are derived, not fitted (u = 2^-24):
  add_global   2e-6 R            the project's 1e-6 bound on cos / sin, plus cbrt, sqrt and four roundings
  add_local    sigma 1e-5 + 4 u max|value|      1e-5: the project's bound on the Box-Muller normals (test_gpu_augment.py)
  jitter       the same
  rotate       8e-6 max|p|       three rotations of two products and a sum each, on 1e-6 cos / sin
  scale        2 u max|p'|       one product
  renorm       dataset_ref.unit_sphere64's bound (SUM_DEPTH), as test_gpu_dataset.py holds the same routine to
The measured maxima are printed (run with -s) and recorded in profiles/corrupt.json by tools/bench_corrupt.py."""
import math

import numpy as np
import pytest
import torch

import corrupt_ref as cf
from dataset_ref import unit_sphere64
from guarded_alloc import SENTINEL, ZERO, guarded, place
from helpers import same_bits

pytestmark = pytest.mark.gpu

SEED = 0xa4093822299f31d0            # both key words in use (test_gpu_augment.py's)
STEP = (0x0123456 << 32) | 0xfffffffe   # both step words in use, and the low word wraps within a few calls
# every size of {1, 63, 64, 65, 1023, 1024, 1025, 8192}: wave boundary, lane boundary (8 rows), block limit
LENGTH_SETS = [(1, 64, 63), (1024, 65, 1023), (8192, 1025, 1)]
U = 2.0 ** -24
# severity 5 of every kind
PARAMS = {
    "drop_global": dict(ratio=0.75),
    "drop_local": dict(total=500, max_clusters=8),
    "add_global": dict(count=50, radius=1.0),
    "add_local": dict(total=500, max_clusters=8, sigma_low=0.075, sigma_high=0.125),
    "rotate": dict(theta=math.pi / 6),
    "scale": dict(scale=2.0),
    "jitter": dict(sigma=0.05),
}
KINDS = tuple(PARAMS)
MEASURED = {}                        # kind -> the largest error / bound seen


def C():
    from si_mamba_amd import corruptions
    return corruptions


def state_at(device, seed=SEED, step=STEP):
    from si_mamba_amd.transforms import AugmentState
    return AugmentState(seed, device).manual_seed(seed, step)


def run(pts, kind, step=STEP, **kw):
    kw = {**PARAMS[kind], **kw}
    kw.setdefault("renorm", False)
    return C().corrupt(pts, kind, state=state_at(pts.device, SEED, step), return_src=True, **kw)


def padded(lengths, seed, fill=float("nan"), N=None):
    """(B, N, 3) float32 on the CPU: uniform in [-1, 1)^3, ``fill`` behind every length."""
    g = torch.Generator().manual_seed(seed)
    N = max(lengths) if N is None else N
    pts = torch.rand(len(lengths), N, 3, generator=g) * 2 - 1
    for b, n in enumerate(lengths):
        pts[b, n:] = fill
    return pts


def lattice(side, step=0.25):
    """side^3 points on a cubic lattice, multiples of ``step``: every distance repeats many times, exactly."""
    a = torch.arange(side, dtype=torch.float32) * step - step * (side // 2)
    return torch.stack(torch.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)


def abi_params(kind, kw):
    return [kw[k] for k in cf.KIND[kind][1]]


def check(pts, lengths, kind, got, step=STEP, **kw):
    """``got`` = (out, out_lengths, src) of the batch against the restatement, cloud by cloud."""
    kw = {**PARAMS[kind], **kw}
    out, out_len, src = (t.cpu() for t in got)
    K = out.shape[1]
    assert out_len.dtype == torch.int64 and src.dtype == torch.int32 and src.shape == out.shape[:2]
    code = cf.KIND[kind][0]
    worst = 0.0
    for b, n in enumerate(lengths):
        p = pts[b, :n].numpy()
        r = cf.corrupt_cloud(p, code, abi_params(kind, kw), SEED, step, b, K=K)
        ln = int(out_len[b])
        assert ln == r["len"], (kind, b, n, ln, r["len"])
        assert np.array_equal(src[b, :ln].numpy(), r["src"]), (kind, b, n)
        assert bool((src[b, ln:] == cf.INT_MIN).all()), (kind, b, n)
        assert same_bits(out[b, ln:], torch.zeros(K - ln, 3)), (kind, b, n)
        g = out[b, :ln].double().numpy()
        own = r["src"] >= 0
        if kind in ("drop_global", "drop_local", "add_global", "add_local"):      # copied rows: bit for bit
            assert same_bits(out[b, :ln][torch.from_numpy(own)], pts[b, torch.from_numpy(r["src"][own])]), (kind, b, n)
        err = np.abs(g - r["out"])
        big = max(np.abs(r["out"]).max(), np.abs(p).max())
        if kind == "add_global":
            bound = np.full(ln, 2e-6 * kw["radius"])
        elif kind == "add_local":
            sig = np.array([0.0] + [float(s) for s in r["sigmas"]])
            bound = sig[np.where(own, 0, -r["src"])] * 1e-5 + 4 * U * big
        elif kind == "jitter":
            bound = np.full(ln, float(np.float32(kw["sigma"])) * 1e-5 + 4 * U * big)
        elif kind == "rotate":
            bound = np.full(ln, 8e-6 * np.abs(p).max())
        elif kind == "scale":
            bound = np.full(ln, 2 * U * np.abs(r["out"]).max())
        else:
            bound = np.zeros(ln)
        bound = np.where(own & (kind in ("add_global", "add_local")), 0.0, bound)
        ratio = np.where(err.max(1) > 0, err.max(1) / np.maximum(bound, 1e-300), 0.0).max() if ln else 0.0
        worst = max(worst, float(ratio))
        assert np.all(err.max(1) <= bound), (kind, b, n, float(err.max()), float(bound.min()))
    MEASURED[kind] = max(MEASURED.get(kind, 0.0), worst)
    print(f"{kind}: lengths {tuple(lengths)}, K = {K}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("lengths", LENGTH_SETS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("kind", KINDS)
def test_against_the_restatement(device, kind, lengths):
    pts = padded(lengths, seed=sum(lengths))
    ln = torch.tensor(lengths)
    got = run(pts.to(device), kind, lengths=ln.to(device))
    check(pts, lengths, kind, got)
    if kind in ("drop_global", "drop_local"):
        for b, n in enumerate(lengths):
            if n == 1:                                           # nothing to remove from a single point
                assert int(got[1][b]) == 1 and int(got[2][b, 0]) == 0 and same_bits(got[0][b, 0].cpu(), pts[b, 0])


TIE_LENGTHS = (343, 100, 1000)


def tie_clouds():
    """A 7^3 lattice, 100 identical points and a 10^3 lattice: exact distance ties throughout."""
    pts = torch.full((3, 1000, 3), float("nan"))
    pts[0, :343] = lattice(7)
    pts[1, :100] = torch.tensor([0.5, -0.25, 0.125])
    pts[2, :1000] = lattice(10, 0.125)
    return pts


@pytest.mark.parametrize("kind", KINDS)
def test_exact_ties_go_to_the_lower_index(device, kind):
    pts = tie_clouds()
    kw = dict(total=90) if kind in ("drop_local", "add_local") else {}
    got = run(pts.to(device), kind, lengths=torch.tensor(TIE_LENGTHS).to(device), **kw)
    check(pts, TIE_LENGTHS, kind, got, **kw)
    if kind in ("drop_global", "drop_local"):                    # identical points under the normalisation: exact zeros
        out, ln, _ = run(pts.to(device), kind, lengths=torch.tensor(TIE_LENGTHS).to(device), renorm=True, **kw)
        assert same_bits(out[1].cpu(), torch.zeros(1000, 3)) and int(ln[1]) == int(got[1][1])


@pytest.mark.parametrize("kind", KINDS)
def test_renorm_within_the_dataset_routine_bound(device, kind):
    """RENORM is pc_norm of the call's own result: the un-normalised call at the same [seed, step] gives its input bit
    for bit, unit_sphere64 the float64 answer and the bound of the fp32 routine."""
    lengths = (1024, 65, 1023)
    pts = padded(lengths, seed=5).to(device)
    ln = torch.tensor(lengths, device=device)
    raw, raw_len, raw_src = run(pts, kind, lengths=ln)
    out, out_len, src = run(pts, kind, lengths=ln, renorm=True)
    assert torch.equal(out_len, raw_len) and torch.equal(src, raw_src)
    worst = 0.0
    for b in range(3):
        n = int(out_len[b])
        want, bound = unit_sphere64(raw[b, :n].double().cpu().numpy())
        err = np.abs(out[b, :n].double().cpu().numpy() - want).max()
        assert err <= bound, (kind, b, err, bound)
        worst = max(worst, err / bound if bound > 0 else 0.0)    # a single row left: zeros, and a bound of zero
        assert same_bits(out[b, n:].cpu(), torch.zeros(out.shape[1] - n, 3))
    MEASURED["renorm"] = max(MEASURED.get("renorm", 0.0), worst)
    print(f"renorm after {kind}: worst error / bound = {worst:.3f}")
    if kind == "scale":                                          # the kind's own default
        dflt = C().corrupt(pts, "scale", 5, lengths=ln, state=state_at(device))
        assert same_bits(dflt[0], out)


@pytest.mark.parametrize("kind", ["add_global", "add_local"])
def test_added_points_stop_at_the_output_rows(device, kind):
    """K < n + A: exactly K - n rows are added."""
    lengths = (200, 193, 150)
    pts = padded(lengths, seed=8)
    out = torch.empty(3, 207, 3, device=device)
    got = run(pts.to(device), kind, lengths=torch.tensor(lengths).to(device), out=out)
    assert got[0] is out
    want = [207, 207, 200 if kind == "add_global" else 207]     # 50 global outliers fit behind 150 rows, 500 do not
    assert got[1].tolist() == want
    assert [(got[2][b] < 0).sum().item() - (207 - want[b]) for b in range(3)] == [7, 14, want[2] - 150]
    check(pts, lengths, kind, got)
    # the default K leaves room for all of them
    full = run(pts.to(device), kind, lengths=torch.tensor(lengths).to(device))
    adds = 50 if kind == "add_global" else 500
    assert full[0].shape[1] == 200 + adds and full[1].tolist() == [n + adds for n in lengths]


@pytest.mark.parametrize("kind", KINDS)
def test_a_cloud_depends_on_nothing_but_itself_and_the_state(device, kind):
    lengths = (300, 129, 64, 250, 300)
    pts = padded(lengths, seed=12)
    pts[4] = pts[0]                                              # the same rows as another cloud of the batch
    pts = pts.to(device)
    ln = torch.tensor(lengths, device=device)
    kw = {**PARAMS[kind], **(dict(total=90) if kind in ("drop_local", "add_local") else {})}
    st = state_at(device)

    def call(p, l):
        return C().corrupt(p, kind, lengths=l, state=st, return_src=True, **kw)

    five = call(pts, ln)
    assert st.step == STEP + 1 and st.seed == SEED
    st.manual_seed(SEED, STEP)
    three = call(pts[:3].contiguous(), ln[:3])
    assert st.step == STEP + 1
    for a, b in zip(five, three):
        assert same_bits(a[:3], b)
    later = call(pts, ln)                                        # the next step: other draws
    assert st.step == STEP + 2 and not same_bits(later[0], five[0])
    st.manual_seed(SEED, STEP)
    for a, b in zip(five, call(pts, ln)):
        assert same_bits(a, b)
    assert not same_bits(five[0][0], five[0][4])                 # the same rows at another place in the batch: other draws


@pytest.mark.parametrize("kind", KINDS)
def test_memory_contract(device, kind):
    """Guard bands around out, out_lengths and src stay intact, every element of the three is written, and neither what
    lies behind an input cloud's length nor what the outputs held before is read: two poisons, the same bits."""
    lengths = (1024, 65, 1023)
    got = []
    for poison, fill in ((ZERO, float("nan")), (SENTINEL, 7.0)):
        pts = padded(lengths, seed=21, fill=fill).to(device)
        with guarded(poison) as g:
            res = run(place(pts), kind, lengths=place(torch.tensor(lengths, device=device)), renorm=(kind == "scale"))
            g.verify()
            assert len(g.records) == 5                           # the two placed inputs, out, out_lengths, src
        got.append(res)
    for a, b in zip(*got):
        assert same_bits(a, b)
    assert bool(torch.isfinite(got[0][0]).all())


def small_model(device):
    from si_mamba_amd.point_mamba import PointMamba, default_config
    from test_gpu_curve_models import SMALL
    torch.manual_seed(0)
    return PointMamba(default_config(method="CURVE", drop_path=0., cls_dim=5, **SMALL)).to(device).eval()


def test_captured_graph_draws_anew_at_every_replay(device):
    lengths = (256, 200, 129)
    pts = padded(lengths, seed=30).to(device)
    ln = torch.tensor(lengths, device=device)
    st = state_at(device)
    out = torch.empty(3, 256, 3, device=device)

    def step():
        return C().corrupt(pts, "drop_local", total=60, max_clusters=8, lengths=ln, state=st, out=out, return_src=True)

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
    assert st.step == STEP + 2
    assert not same_bits(seen[0][2], seen[1][2])
    st.manual_seed(SEED, STEP)
    for k in range(2):
        eager = C().corrupt(pts, "drop_local", total=60, max_clusters=8, lengths=ln, state=st, return_src=True)
        for a, b in zip(eager, seen[k]):
            assert same_bits(a, b), k
    assert st.step == STEP + 2


def test_pointmamba_on_corrupted_clouds_equals_every_cloud_alone(device):
    """The ragged route's own comparison (test_gpu_ragged_clouds.py, 1e-3 on the normalised logits) with corrupt as the
    producer of the lengths."""
    m = small_model(device)
    lengths = (256, 200, 129)
    pts = padded(lengths, seed=31).to(device)
    x, xl = C().corrupt(pts, "drop_local", total=60, max_clusters=8, lengths=torch.tensor(lengths, device=device),
                        state=state_at(device))
    assert xl.tolist() == [196, 140, 69] and bool(torch.isfinite(x).all())
    with torch.no_grad():
        got = m(x, lengths=xl)
        assert got.shape == (3, 5) and bool(torch.isfinite(got).all())
        worst = 0.0
        for b, n in enumerate(xl.tolist()):
            want = m(x[b:b + 1, :n].contiguous())
            err = ((got[b:b + 1] - want).abs().max() / max(1.0, want.abs().max().item())).item()
            print(f"cloud {b}: {n} points, logits error {err:.3e}")
            worst = max(worst, err)
        assert worst <= 1e-3, worst


def test_evaluate_robustness_equals_accuracies_counted_on_the_host(device):
    m = small_model(device)
    g = torch.Generator().manual_seed(40)
    pts = (torch.rand(6, 1024, 3, generator=g) * 2 - 1).to(device)
    labels = torch.randint(0, 5, (6,), generator=g).to(device)
    kinds, sevs = ("drop_local", "add_global"), (2, 5)
    base = {"clean": 0.5, "drop_local": [0.5, 0.75], "add_global": [0.625, 0.875]}
    res = C().evaluate_robustness(m, pts, labels, kinds=kinds, severities=sevs, batch_size=4, state=state_at(device),
                                  baseline=base)
    st = state_at(device)                                        # the same calls in the same order, counted one by one
    clean, hits = 0, {k: [0, 0] for k in kinds}
    with torch.no_grad():
        for lo in (0, 4):
            x, y = pts[lo:lo + 4].contiguous(), labels[lo:lo + 4].cpu()
            clean += int((m(x).argmax(-1).cpu() == y).sum())
            for k in kinds:
                for s, sev in enumerate(sevs):
                    cx, cl = C().corrupt(x, k, sev, state=st)
                    hits[k][s] += int((m(cx, lengths=cl).argmax(-1).cpu() == y).sum())
    assert res["total"] == 6 and res["clean_acc"] == clean / 6
    for k in kinds:
        assert res["acc"][k] == [h / 6 for h in hits[k]]
        err = [1 - h / 6 for h in hits[k]]
        assert abs(res["CE"][k] - sum(err) / sum(base[k])) < 1e-12
        assert abs(res["RCE"][k] - sum(e - (1 - clean / 6) for e in err) / sum(v - 0.5 for v in base[k])) < 1e-12
    assert abs(res["mCE"] - sum(res["CE"].values()) / 2) < 1e-12
    assert abs(res["RmCE"] - sum(res["RCE"].values()) / 2) < 1e-12
    with pytest.raises(TypeError, match="lengths"):
        C().evaluate_robustness(lambda x: x, pts, labels)
