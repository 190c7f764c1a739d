"""GPU: GraphedTrainStep with si_mamba_amd.optim.AdamW as its optimizer -- the clip, the update and the schedule inside
the captured step as three launches -- against the eager loop with the same optimizer (bit for bit under the
deterministic backward), against torch's tail on the setup of test_gpu_model.py::test_graphed_train_step_matches_eager
(that test's tolerances), and the two-graph data-parallel step against the single graph.

The learning rate: Adam's normalised update turns a last-bit difference of a near-zero gradient into a step of up to
+-lr (the reason that test runs plain SGD), so two correct tails can part by 2 lr per step.  LR = 2e-4 keeps six such
steps at 2.4e-3, inside that test's 5e-3, whatever the gradients do."""
import copy

import pytest
import torch

from graphed_dp_rank import CLIP, cls_batches, cls_loss, small_pointmamba, worst_difference
from helpers import same_bits
from si_mamba_amd import optim, set_deterministic
from si_mamba_amd.graphed import GraphedTrainStep

pytestmark = pytest.mark.gpu

LOSS_TOL, PARAM_TOL = 2e-3, 5e-3          # test_graphed_train_step_matches_eager's
LR, WD, WARMUP = 2e-4, 0.05, 3
VALUES = [LR, 0.5 * LR, 0.25 * LR, 0.125 * LR]          # steps_per_epoch = 2: the rate changes under the replays


@pytest.fixture
def deterministic_backward():
    """The package's deterministic backward and torch's switch: the library GEMMs need the latter (the package's own mode
    alone leaves their last bits free, tests/test_gpu_deterministic.py)."""
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    set_deterministic(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=prev_warn)
        set_deterministic(None)


@pytest.fixture
def one_rank_group(tmp_path, device):
    import torch.distributed as dist
    assert not dist.is_initialized()
    torch.cuda.set_device(device)
    dist.init_process_group("nccl", init_method=f"file://{tmp_path}/store", rank=0, world_size=1)
    try:
        yield dist.group.WORLD
    finally:
        dist.destroy_process_group()


def _on(device, data):
    return [tuple(t.to(device) for t in d) for d in data]


def hip_adamw(model, schedule=True):
    opt = optim.AdamW(optim.reference_param_groups(model, WD), lr=LR)
    if schedule:
        opt.set_schedule(VALUES, steps_per_epoch=2)
    return opt


def eager_hip(model, opt, batch):
    opt.zero_grad(set_to_none=True)
    loss = cls_loss(model)(*batch)
    loss.backward()
    opt.step(clip=CLIP)
    return loss.detach()


def eager_torch(model, opt, batch, lr):
    for g in opt.param_groups:
        g["lr"].fill_(lr)
    opt.zero_grad(set_to_none=True)
    loss = cls_loss(model)(*batch)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(model.parameters(), CLIP, foreach=True)
    opt.step()
    return loss.detach()


def assert_same_parameters(ma, mb):
    for (k, a), b in zip(ma.named_parameters(), mb.parameters()):
        assert same_bits(a, b), k


def test_single_process_matches_eager_bit_for_bit_and_torch(device, deterministic_backward):
    torch.manual_seed(0)
    ma = small_pointmamba(device)
    mb, mc = copy.deepcopy(ma), copy.deepcopy(ma)
    oa, ob = hip_adamw(ma), hip_adamw(mb)
    groups = optim.reference_param_groups(mc, WD)
    oc = torch.optim.AdamW(groups, lr=torch.tensor(LR, device=device), capturable=True, foreach=True)
    data = _on(device, cls_batches(4, 8, 256))
    step = GraphedTrainStep(cls_loss(ma), oa, data[0], clip=CLIP, warmup=WARMUP)
    assert step.hip_tail and step.grad_norm is oa.grad_norm
    la, lb, lc, norms = [], [], [], []
    for k in range(WARMUP):                                   # the graphed object took its warm-up steps on data[0]
        eager_hip(mb, ob, data[0])
        eager_torch(mc, oc, data[0], VALUES[k // 2])
    for k, d in enumerate(data[1:], start=WARMUP):
        la.append(step(*d).clone())
        norms.append((step.grad_norm.clone(), None))
        lb.append(eager_hip(mb, ob, d))
        norms[-1] = (norms[-1][0], ob.grad_norm.clone())
        lc.append(eager_torch(mc, oc, d, VALUES[min(k // 2, len(VALUES) - 1)]))
    print("graphed", [float(x) for x in la], "eager", [float(x) for x in lb], "norms",
          [(float(a), float(b)) for a, b in norms], "worst parameter difference", worst_difference(ma, mb))
    # graphed == eager, bit for bit: losses, the norm before clipping, parameters, the rate the table gave
    for a, b in zip(la, lb):
        assert same_bits(a, b), (la, lb)
    for a, b in norms:
        assert same_bits(a, b) and float(a) > 0
    assert_same_parameters(ma, mb)
    assert oa.update_count() == ob.update_count() == WARMUP + 3
    want_lr = torch.tensor([VALUES[(WARMUP + 2) // 2]] * 2, dtype=torch.float32)
    assert oa.device_lr().cpu().tolist() == want_lr.tolist() == ob.device_lr().cpu().tolist()
    # .grad holds the raw gradients: their norm is the one reported
    raw = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in ma.parameters()]))
    assert abs(float(raw) - float(step.grad_norm)) <= 1e-5 * float(raw)
    # both against torch's tail fed the same rates
    la, lc = [float(x) for x in la], [float(x) for x in lc]
    worst = worst_difference(ma, mc)
    print("losses", la, lc, "worst parameter difference", worst)
    assert max(abs(a - c) for a, c in zip(la, lc)) < LOSS_TOL, (la, lc)
    assert worst < PARAM_TOL, worst
    moved = max(float((p.detach() - q.detach()).abs().max())
                for p, q in zip(ma.parameters(), small_pointmamba_like(ma, device).parameters()))
    assert moved > 0


def small_pointmamba_like(model, device):
    """The model as test_single_process... initialised it (seed 0), to show that the steps moved the parameters."""
    torch.manual_seed(0)
    return small_pointmamba(device)


def test_data_parallel_two_graphs_match_the_single_graph(device, one_rank_group, deterministic_backward):
    torch.manual_seed(0)
    ma = small_pointmamba(device)
    mb = copy.deepcopy(ma)
    oa, ob = hip_adamw(ma), hip_adamw(mb)
    data = _on(device, cls_batches(4, 8, 256))
    # (the single graph first: it captures in the global mode, which wants no collective still in the watchdog's hands)
    single = GraphedTrainStep(cls_loss(mb), ob, data[0], clip=CLIP, warmup=WARMUP)
    step = GraphedTrainStep(cls_loss(ma), oa, data[0], clip=CLIP, warmup=WARMUP, process_group=one_rank_group, module=ma)
    assert step.hip_tail and len(step.flat.buffers) == 1
    assert step.graph_a is not None and step.graph_b is not None and single.graph is not None
    for d in data[1:]:
        la, lb = step(*d), single(*d)
        print("two graphs", float(la), float(step.grad_norm), "single", float(lb), float(single.grad_norm))
        assert same_bits(la, lb)
        assert step.grad_norm is oa.grad_norm and same_bits(step.grad_norm, single.grad_norm)
        assert float(step.grad_norm) > 0
    assert_same_parameters(ma, mb)
    assert oa.update_count() == ob.update_count() == WARMUP + 3
    # the gradients still alias the flat buffer and hold the raw mean, not the clipped one
    assert step._probe.grad.data_ptr() == step._probe_ptr
    raw = torch.linalg.vector_norm(step.flat.buffers[0])
    assert abs(float(raw) - float(step.grad_norm)) <= 1e-5 * float(raw)
