"""GPU: si_mamba_amd.optim.AdamW (csrc/optim.hip) against the float64 restatement of tests/optim_ref.py.

The shared case: tensors of 1, 3, 5, 127, C-1, C, C+1, 2C+7, (96, 40) and 384 elements (C = SIMAMBA_OPTIM_CHUNK) in two
groups (weight decay 0 and 0.05), lr = 0.05 on parameters of 0.02 * N(0, 1) so that the updates dominate the values,
five steps of fresh gradients scaled by 1, 0.01, 3, 1e-4, 0.5 under clip = 10 (active at steps 0, 2, 4), one tensor with
every second gradient zero and one with gradients of order 1e-9.  Bounds: helpers.pinned_bound of torch's own fp32 tail
on the CPU against its float64 tail (computed here, once), capped at 1e-5."""
import copy

import pytest
import torch

import optim_ref
from guarded_alloc import SENTINEL, ZERO, guarded, place
from guarded_alloc import same_bits as same_bytes
from helpers import same_bits
from si_mamba_amd import _lib, optim
from si_mamba_amd.dist import FlatGradients

pytestmark = pytest.mark.gpu
C = _lib.OPTIM_CHUNK
DEV = "cuda:0"


@pytest.fixture(scope="module")
def case():
    return optim_ref.Case(C)


@pytest.fixture(scope="module")
def ref(case):
    r = optim_ref.ref_run(case)
    r["bounds"], r["ref32_err"] = optim_ref.bounds(case)
    print("reference fp32 errors", r["ref32_err"], "bounds", r["bounds"])
    return r


def device_params(case, offset=None):
    """The case's parameters on the device as leaves: separate allocations, or (``offset`` = k) views of one flat buffer
    laid back to back from element k, so that they sit at every 4-byte alignment."""
    if offset is None:
        return [p.to(DEV).requires_grad_(True) for p in case.params]
    flat = torch.zeros(offset + sum(p.numel() for p in case.params) + 4, device=DEV)
    out, o = [], offset
    for p in case.params:
        view = flat[o:o + p.numel()].view(p.shape)
        view.copy_(p)
        out.append(view.detach().requires_grad_(True))
        o += p.numel()
    return out


def set_grads(params, grads):
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = g.to(DEV).clone()
        else:
            p.grad.copy_(g)


def state_lists(opt, params):
    return ([opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params],
            [opt.state[p]["step"] for p in params])


def run_hip(case, steps=5, clip=optim_ref.CLIP, offset=None, flat_grads=False, **step_kw):
    params = device_params(case, offset)
    opt = optim.AdamW(case.groups(params))
    if flat_grads:
        for p in params:
            p.grad = torch.zeros_like(p)
        flat = FlatGradients(params)
        assert len(flat.buffers) == 1
    norms = []
    for k in range(steps):
        set_grads(params, case.grads[k])
        opt.step(clip=clip, **step_kw)
        norms.append(opt.grad_norm.clone())
    m, v, t = state_lists(opt, params)
    return dict(p=params, m=m, v=v, t=t, norms=[float(n) for n in norms], opt=opt)


def check_parity(got, ref):
    err = dict(p=optim_ref.worst(got["p"], ref["p"]), m=optim_ref.worst(got["m"], ref["m"]),
               v=optim_ref.worst(got["v"], ref["v"]), norm=optim_ref.norm_err(got["norms"], ref["norms"]))
    print("errors", err, "bounds", ref["bounds"])
    for k, e in err.items():
        assert e <= ref["bounds"][k], (k, e, ref["bounds"][k])
    assert [float(t) for t in got["t"]] == [float(t) for t in ref["t"]]


def test_float64_parity_over_five_steps(case, ref):
    got = run_hip(case)
    check_parity(got, ref)
    assert got["opt"].update_count() == 5


@pytest.mark.parametrize("k", [1, 2, 3])
def test_every_alignment(case, ref, k):
    """Parameters as views flat[k : k + n] laid back to back and gradients as slices of a FlatGradients buffer: every
    4-byte alignment of p and g, independently; the state sits where the allocator puts it (16-byte aligned)."""
    got = run_hip(case, offset=k, flat_grads=True)
    seen = {(p.data_ptr() % 16, p.grad.data_ptr() % 16) for p in got["p"]}
    # back to back, the case's sizes put three of the four residues under the parameters (k, k + 1, k + 3 elements;
    # the three values of k cover all four) and three under the gradients, and no pair in step with one another
    assert {a // 4 for a, _ in seen} == {k % 4, (k + 1) % 4, (k + 3) % 4}, seen
    assert {b // 4 for _, b in seen} == {0, 1, 3}, seen
    assert all(a != b for a, b in seen) or k == 0, seen
    check_parity(got, ref)


def test_more_tensors_than_one_launch_carries():
    """The first kernel takes the gradient addresses as arguments, 448 to a launch: 451 tensors take two launches, the
    second with a tensor of more than one chunk; and the gradients are fresh tensors at every step."""
    case2 = optim_ref.Case(C, seed=7, shapes=[(16 + i % 7,) for i in range(449)] + [(C + 1,), (3,)])
    want = optim_ref.ref_run(case2, steps=2)
    want["bounds"], err = optim_ref.bounds(case2, steps=2)
    print("reference fp32 errors", err)
    params = device_params(case2)
    opt = optim.AdamW(case2.groups(params))
    norms = []
    for k in range(2):
        for p, g in zip(params, case2.grads[k]):
            p.grad = g.to(DEV)                                       # another address than the step before
        opt.step(clip=optim_ref.CLIP)
        norms.append(opt.grad_norm.clone())
    m, v, t = state_lists(opt, params)
    check_parity(dict(p=params, m=m, v=v, t=t, norms=[float(n) for n in norms]), want)


def test_captured_schedule_changes_the_rate_without_recapture(case, ref):
    values = [0.05, 0.02, 0.01]
    params = device_params(case)
    opt = optim.AdamW(case.groups(params, lr=123.0))           # the float is not read once a schedule is attached
    opt.set_schedule(values, steps_per_epoch=2, lr_scale=[1.0, 0.5])
    set_grads(params, case.grads[0])
    opt.prepare()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph):
            opt.step(clip=optim_ref.CLIP)
    torch.cuda.current_stream().wait_stream(side)
    lrs, norms = [], []
    for k in range(5):
        set_grads(params, case.grads[k])
        graph.replay()
        lrs.append(opt.device_lr().clone())
        norms.append(opt.grad_norm.clone())
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))          # the device rate is fp32: feed the same
    want_lrs = [(f32(values[k // 2]), f32(0.5 * values[k // 2])) for k in range(5)]
    for got_lr, want in zip(lrs, want_lrs):
        assert got_lr.tolist() == list(want)
    assert want_lrs[1] != want_lrs[2] and want_lrs[3] != want_lrs[4]
    want = optim_ref.ref_run(case, lrs=want_lrs)
    m, v, t = state_lists(opt, params)
    got = dict(p=params, m=m, v=v, t=t, norms=[float(n) for n in norms])
    check_parity(got, dict(want, bounds=ref["bounds"]))
    assert opt.update_count() == 5
    # inside a capture a stale table raises instead of being used
    opt.state[params[0]]["exp_avg"] = opt.state[params[0]]["exp_avg"].clone()
    with pytest.raises(RuntimeError, match="stale"):
        with torch.cuda.stream(side):
            with torch.cuda.graph(torch.cuda.CUDAGraph()):
                opt.step(clip=optim_ref.CLIP)
    torch.cuda.synchronize()


def test_parameter_without_a_gradient_is_untouched(case):
    params = device_params(case)
    extra = torch.full((7,), 0.5, device=DEV, requires_grad=True)     # never takes a gradient: no state either
    groups = case.groups(params)
    groups[1]["params"].append(extra)
    opt = optim.AdamW(groups)
    set_grads(params, case.grads[0])
    opt.step(clip=optim_ref.CLIP)
    j = 5                                                             # C elements, a whole chunk, between C-1 and C+1
    before = [[t.clone() for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], opt.state[p]["step"])]
              for p in params]
    set_grads(params, case.grads[1])
    params[j].grad = None
    opt.step(clip=optim_ref.CLIP)
    for i, p in enumerate(params):
        now = (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], opt.state[p]["step"])
        if i == j:
            assert all(same_bits(a, b) for a, b in zip(now, before[i])) and float(now[3]) == 1.0
        else:
            assert not any(same_bits(a, b) for a, b in zip(now, before[i])), i
            assert float(now[3]) == 2.0
    assert same_bits(extra, torch.full((7,), 0.5)) and extra not in opt.state
    # the norm leaves the missing gradient out
    want = sum(float(g.double().square().sum()) for i, g in enumerate(case.grads[1]) if i != j) ** 0.5
    assert abs(float(opt.grad_norm) - want) <= 1e-6 * want


def test_zero_grads_in_the_same_pass(case):
    keep = run_hip(case, steps=2)
    zero = run_hip(case, steps=2, offset=1, flat_grads=True, zero_grads=True)
    plain = run_hip(case, steps=2, zero_grads=True)
    for got in (zero, plain):
        assert all(float(p.grad.abs().max()) == 0.0 for p in got["p"])
        for k in "pmv":
            assert all(same_bits(a, b) for a, b in zip(got[k], keep[k])), k
        assert got["norms"] == keep["norms"]
    assert all(same_bits(p.grad, g) for p, g in zip(keep["p"], case.grads[1]))       # the raw gradients, not clipped


def test_same_bits_on_two_runs(case):
    a, b = run_hip(case), run_hip(case)
    for k in "pmv":
        assert all(same_bits(x, y) for x, y in zip(a[k], b[k])), k
    assert a["norms"] == b["norms"]


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_gradients_follow_torch_clamp(case, bad):
    """One NaN / one inf in a single gradient element: torch.clamp(coef, max=1) keeps a NaN coefficient (every
    parameter NaN), and an infinite norm gives coef = 0 (inf * 0 = NaN in that one element)."""
    grads = [[g.clone() for g in case.grads[0]]]
    grads[0][7][C + 3] = bad
    want = optim_ref.torch_tail(case, torch.float32, steps=1, grads=grads)
    params = device_params(case)
    opt = optim.AdamW(case.groups(params))
    set_grads(params, grads[0])
    opt.step(clip=optim_ref.CLIP)
    for i, (p, w) in enumerate(zip(params, want["p"])):
        p = p.detach().cpu()
        assert torch.equal(torch.isnan(p), torch.isnan(w)), i
        assert torch.equal(torch.isinf(p), torch.isinf(w)), i
    n_nan = sum(int(torch.isnan(w).sum()) for w in want["p"])
    assert n_nan == (sum(p.numel() for p in case.params) if bad != bad else 1)


def test_state_dict_interchange_on_the_device(case, ref):
    bound = ref["bounds"]["p"]

    def torch_opt(params):
        return torch.optim.AdamW(case.groups(params), capturable=True, foreach=True)

    def one_more(ours, po, theirs, pt, k):
        set_grads(po, case.grads[k])
        set_grads(pt, case.grads[k])
        ours.step(clip=optim_ref.CLIP)
        torch.nn.utils.clip_grad_norm_(pt, optim_ref.CLIP, foreach=True)
        theirs.step()
        assert optim_ref.worst(po, pt) <= bound
        for a, b in zip(po, pt):
            assert float(ours.state[a]["step"]) == float(theirs.state[b]["step"]) == 3.0

    # ours for two steps -> torch's
    got = run_hip(case, steps=2)
    ours, po = got["opt"], got["p"]
    sd = ours.state_dict()
    assert all(g["updates"] == 2 for g in sd["param_groups"])
    pt = [p.detach().clone().requires_grad_(True) for p in po]
    theirs = torch_opt(pt)
    theirs.load_state_dict(copy.deepcopy(sd))           # as after a save and a load: no tensor shared
    one_more(ours, po, theirs, pt, 2)
    # the update count survives torch's optimizer and comes back
    back = optim.AdamW(case.groups(device_params(case)))
    back.load_state_dict(copy.deepcopy(theirs.state_dict()))
    assert back.update_count() == 2 and ours.update_count() == 3

    # torch's for two steps -> ours
    pt = device_params(case)
    theirs = torch_opt(pt)
    for k in range(2):
        set_grads(pt, case.grads[k])
        torch.nn.utils.clip_grad_norm_(pt, optim_ref.CLIP, foreach=True)
        theirs.step()
    po = [p.detach().clone().requires_grad_(True) for p in pt]
    ours = optim.AdamW(case.groups(po))
    ours.load_state_dict(copy.deepcopy(theirs.state_dict()))
    assert ours.update_count() == 2
    one_more(ours, po, theirs, pt, 2)
    assert ours.update_count() == 3


def test_memory_contract(case):
    """Guard bands intact around every buffer the step allocates through torch.empty (the workspace, the moments) and
    around the parameters and gradients; two poisons give the same bits, so nothing in the workspace is read before it
    is written."""
    plain = run_hip(case, steps=2, zero_grads=True)
    got = []
    for poison in (ZERO, SENTINEL):
        with guarded(poison) as g:
            params = [place(p.to(DEV)).requires_grad_(True) for p in case.params]
            opt = optim.AdamW(case.groups(params))
            for k in range(2):
                for p, gr in zip(params, case.grads[k]):
                    if p.grad is None:
                        p.grad = place(gr.to(DEV))
                    else:
                        p.grad.copy_(gr)
                opt.step(clip=optim_ref.CLIP, zero_grads=True)
            torch.cuda.synchronize()
            g.verify()
            assert len(g.records) > 2 * len(params), "the step allocated nothing through the harness"
            assert "adamw.py" in g.modules
        m, v, _ = state_lists(opt, params)
        got.append([p.detach() for p in params] + m + v + [p.grad for p in params] + [opt.grad_norm.reshape(1)])
    want = plain["p"] + plain["m"] + plain["v"] + [p.grad for p in plain["p"]]
    for i, (a, b) in enumerate(zip(got[0], got[1])):
        assert same_bytes(a, b), f"tensor {i} differs between the two poisons"
    for i, (a, w) in enumerate(zip(got[0], want)):
        assert same_bytes(a.detach(), w.detach()), f"tensor {i} differs from the run outside the harness"
