"""GPU: the data-parallel GraphedTrainStep (graph A: zero + forward + backward into one flat gradient buffer; the one
all-reduce, eager; graph B: mean, clip, optimizer step) against the eager data-parallel step on the same ranks.

Bounds: those of tests/test_gpu_model.py::test_graphed_train_step_matches_eager -- losses within 2e-3, parameters
within 5e-3, plain SGD for the reason given there.  Dropout, drop-path and the HLT tie-break are off, and the MAE's
patch masks are an input of the step, so both sides see the same numbers.  World size 1 runs under a one-rank RCCL
group; two ranks share the one card over gloo (RCCL does not take two ranks on one device), or take one card each
over RCCL where there are two.  The models and steps live in tests/graphed_dp_rank.py, which is also the rank program.
"""
import copy
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

from graphed_dp_rank import (CLIP, LR, cls_batches, cls_loss, eager_step, graphed_against_eager, no_dropout,
                             small_pointmamba, worst_difference)
from helpers import clouds, max_scaled

pytestmark = pytest.mark.gpu

LOSS_TOL, PARAM_TOL = 2e-3, 5e-3


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


def _assert_close(la, lb, ma, mb):
    worst = worst_difference(ma, mb)
    print("losses", la, lb, "worst parameter difference", worst)
    assert len(la) == len(lb) > 0
    assert max(abs(a - b) for a, b in zip(la, lb)) < LOSS_TOL, (la, lb)
    assert worst < PARAM_TOL, worst


def test_world_size_one_matches_the_single_graph(device, one_rank_group):
    """3 warm-up + 6 steps against the one-graph GraphedTrainStep on a deep copy, and the norm before clipping against
    clip_grad_norm_'s on a copy that holds the parameters of the moment."""
    from si_mamba_amd.graphed import GraphedTrainStep
    torch.manual_seed(0)
    ma = small_pointmamba(device)
    mb, mc = copy.deepcopy(ma), copy.deepcopy(ma)
    oa = torch.optim.SGD(ma.parameters(), lr=LR)
    ob = torch.optim.SGD(mb.parameters(), lr=LR)
    data = _on(device, cls_batches(7, 8, 256))
    # (the single graph first: it captures in the global mode, which wants no collective still in the watchdog's hands)
    single = GraphedTrainStep(cls_loss(mb), ob, data[0], clip=CLIP, warmup=3)
    step = GraphedTrainStep(cls_loss(ma), oa, data[0], clip=CLIP, warmup=3, process_group=one_rank_group, module=ma)
    assert len(step.flat.buffers) == 1 and step.flat.params == list(ma.parameters())
    assert step.flat.buffers[0].numel() == sum(p.numel() for p in ma.parameters())
    la, lb = [], []
    for d in data[1:]:
        mc.load_state_dict(ma.state_dict())
        la.append(step(*d).item())
        lb.append(single(*d).item())
    _assert_close(la, lb, ma, mb)
    # the last step's norm: the same parameters, statistics and batch, eagerly
    _, norm = eager_step(mc, torch.optim.SGD(mc.parameters(), lr=LR), cls_loss(mc), data[-1])
    got, want = float(step.grad_norm), float(norm)
    print("grad_norm", got, want)
    assert want > 0 and abs(got - want) <= 1e-4 * want


def test_parameter_without_gradient_stays_out(device, one_rank_group):
    """A registered parameter the loss never touches: outside the flat buffer, .grad None, so AdamW neither moves nor
    decays it (a zero gradient in the flat buffer would let weight_decay shrink it)."""
    from si_mamba_amd.graphed import GraphedTrainStep
    torch.manual_seed(0)
    m = small_pointmamba(device)
    m.register_parameter("spare", nn.Parameter(torch.randn(7, device=device)))
    before = m.spare.detach().clone()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.05, capturable=True)
    data = _on(device, cls_batches(4, 8, 256))
    step = GraphedTrainStep(cls_loss(m), opt, data[0], clip=CLIP, warmup=3, process_group=one_rank_group, module=m)
    moved = m.cls_head_finetune[0].weight.detach().clone()
    for d in data[1:]:
        assert torch.isfinite(step(*d))
    assert m.spare.grad is None and torch.equal(m.spare, before)
    assert all(p is not m.spare for p in step.flat.params)
    assert len(step.flat.params) == len(list(m.parameters())) - 1
    assert not torch.equal(m.cls_head_finetune[0].weight, moved)          # the replays do update the others


def _seg_case(device):
    from si_mamba_amd.seg import PartSegMamba, default_seg_config, get_loss
    cfg = default_seg_config(trans_dim=96, depth=3, fetch_idx=(0, 1, 2), drop_path=0., drop_path_rate=0.)
    m = no_dropout(PartSegMamba(50, cfg).to(device).train())
    m.hlt_rand = False
    B, N = 4, 256
    data = []
    for i in range(5):
        g = torch.Generator().manual_seed(40 + i)
        data.append((clouds(B, N, 30 + i).transpose(1, 2).contiguous(),
                     nn.functional.one_hot(torch.randint(0, 16, (B,), generator=g), 16).float(),
                     torch.randint(0, 50, (B, N), generator=g)))
    crit = get_loss()
    return m, data, lambda model: lambda p, lab, tgt: crit(model(p, lab).reshape(-1, 50), tgt.view(-1))


def _mae_case(device):
    from si_mamba_amd.mae import Point_MAE_Mamba, default_mae_config
    cfg = default_mae_config(trans_dim=96, encoder_dims=96, depth=2, decoder_depth=1, drop_path=0., drop_path_rate=0.,
                             drop_out=0.)
    m = no_dropout(Point_MAE_Mamba(cfg).to(device).train())
    B, N, G = 4, 256, cfg.num_group
    nm = int(cfg.transformer_config.mask_ratio * G)
    data = []
    for i in range(5):
        g = torch.Generator().manual_seed(50 + i)
        data.append((clouds(B, N, 60 + i), torch.rand(B, G, generator=g).argsort(dim=1).argsort(dim=1) < nm))

    def make_loss(model):
        def loss(p, mask):
            # the random patch mask, drawn by the caller: the model keeps the number of masked patches it knows on
            # the host (a mask handed to forward() is counted on the device, which a capture cannot do)
            model.MAE_encoder._mask_center_rand = lambda center, noaug=False: mask
            return model(p)
        return loss
    return m, data, make_loss


@pytest.mark.parametrize("case", ["seg", "mae"])
def test_segmentation_and_mae_match_eager(case, device, one_rank_group):
    """PartSegMamba and Point_MAE_Mamba, 3 warm-up + 4 steps at world size 1 against the eager step on a deep copy.
    (The MAE's decoder_pos_embed takes no gradient: the flat buffer leaves it out.)"""
    torch.manual_seed(0)
    ma, data, make_loss = (_seg_case if case == "seg" else _mae_case)(device)
    mb = copy.deepcopy(ma)
    step, la, lb = graphed_against_eager(ma, mb, make_loss, _on(device, data), one_rank_group)
    _assert_close(la, lb, ma, mb)
    dead = [k for k, p in ma.named_parameters() if p.grad is None]
    assert all(k.startswith("decoder_pos_embed.") for k in dead) and bool(dead) == (case == "mae"), dead
    assert [k for k, p in mb.named_parameters() if p.grad is None] == dead


def test_recapture_takes_the_new_momentum(device, one_rank_group):
    """BatchNorm momentum is a constant of the captured kernels: a change shows after recapture(), not before.  lr = 0
    keeps the parameters, so every step below starts from the same state once the buffers are put back."""
    from si_mamba_amd.graphed import GraphedTrainStep
    torch.manual_seed(0)
    m = small_pointmamba(device)
    bn = m.encoder.first_conv[1]
    assert isinstance(bn, nn.BatchNorm1d) and bn.momentum == 0.1
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    (pts, gt), = _on(device, cls_batches(1, 8, 256))
    with torch.no_grad():
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
    start = copy.deepcopy(m.state_dict())
    step = GraphedTrainStep(cls_loss(m), opt, (pts, gt), clip=CLIP, warmup=3, process_group=one_rank_group, module=m)

    def stats_after(one_step):
        m.load_state_dict(start)
        one_step()
        torch.cuda.synchronize()
        return bn.running_mean.clone(), bn.running_var.clone()

    eager_old = stats_after(lambda: cls_loss(m)(pts, gt))
    bn.momentum = 0.5
    eager_new = stats_after(lambda: cls_loss(m)(pts, gt))
    stale = stats_after(lambda: step(pts, gt))
    step.recapture()
    fresh = stats_after(lambda: step(pts, gt))
    # 1e-4: the bar tests/test_gpu_sync_bn.py holds running statistics to
    for i in range(2):
        print(max_scaled(stale[i], eager_old[i]), max_scaled(fresh[i], eager_new[i]),
              max_scaled(eager_old[i], eager_new[i]))
        assert max_scaled(eager_old[i], eager_new[i]) > 1e-2
        assert max_scaled(stale[i], eager_old[i]) < 1e-4
        assert max_scaled(fresh[i], eager_new[i]) < 1e-4


def test_released_gradients_are_refused(device, one_rank_group):
    from si_mamba_amd.graphed import GraphedTrainStep
    torch.manual_seed(0)
    m = small_pointmamba(device)
    opt = torch.optim.SGD(m.parameters(), lr=LR)
    data = _on(device, cls_batches(1, 8, 256))
    step = GraphedTrainStep(cls_loss(m), opt, data[0], warmup=1, process_group=one_rank_group)
    assert step.grad_norm is None and step.sync_buffers is None
    step(*data[0])
    opt.zero_grad(set_to_none=True)
    with pytest.raises(RuntimeError, match="no longer alias the flat buffer"):
        step(*data[0])


def _two_ranks(tmp_path, device, backend):
    torch.manual_seed(0)
    m = small_pointmamba(device)
    torch.save(dict(state={k: v.cpu() for k, v in m.state_dict().items()}, data=cls_batches(5, 8, 256)),
               tmp_path / "in.pt")
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "graphed_dp_rank.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", "180", sys.executable, helper, str(r), "2", str(tmp_path),
                               backend]) for r in range(2)]
    codes = []
    for p in procs:
        codes.append(p.wait())
        if codes[-1] != 0:                                   # stop at the first failure, no second try
            for q in procs:
                if q.poll() is None:
                    q.kill()
                    q.wait()
            break
    if codes[0] == 77:
        pytest.skip("this torch build's gloo does not take device tensors: " + (tmp_path / "refused0.txt").read_text())
    assert codes == [0, 0], f"rank exit statuses {codes}"
    outs = [torch.load(tmp_path / f"out{r}.pt") for r in range(2)]
    for r, o in enumerate(outs):
        print("rank", r, o["graphed"], o["eager"], o["worst"])
        assert len(o["graphed"]) == len(o["eager"]) == 4
        assert max(abs(a - b) for a, b in zip(o["graphed"], o["eager"])) < LOSS_TOL, (r, o["graphed"], o["eager"])
        assert o["worst"] < PARAM_TOL, (r, o["worst"])
    # each rank saw its own clouds ...
    assert outs[0]["graphed"] != outs[1]["graphed"]
    # ... and applied the same all-reduced bits with SGD, from the parameters rank 0 sent
    for a, b in zip(outs[0]["params"], outs[1]["params"]):
        assert torch.equal(a, b)
    assert outs[0]["buffers"].keys() == outs[1]["buffers"].keys() and len(outs[0]["buffers"]) > 0
    for k, v in outs[0]["buffers"].items():
        assert torch.equal(v, outs[1]["buffers"][k]), k


def test_two_ranks_on_one_card_over_gloo(device, tmp_path):
    _two_ranks(tmp_path, device, "gloo")


def test_two_real_ranks(device, tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip(f"needs 2 GPUs, this machine has {torch.cuda.device_count()}")
    _two_ranks(tmp_path, device, "nccl")
