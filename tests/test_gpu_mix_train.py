"""GPU: cutmix -> PointMamba -> mixed_cross_entropy inside GraphedTrainStep: the captured step computes what the eager
step computes from the same state, and every replay mixes the batch anew."""
import copy

import pytest
import torch

import mix_ref as mr
from helpers import clouds

pytestmark = pytest.mark.gpu

SEED, STEP = mr.SEED, mr.STEP
B, N, WARMUP, REPLAYS = 4, 256, 1, 3


def small_model(device):
    """2 blocks, d = 32, train mode, no dropout: what is left of the randomness is cutmix's."""
    from si_mamba_amd.point_mamba import PointMamba, default_config
    torch.manual_seed(0)
    cfg = default_config(trans_dim=32, encoder_dims=32, depth=2, num_group=16, group_size=8, drop_path=0., knn_graph=8,
                         cls_dim=5)
    m = PointMamba(cfg).to(device).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def test_cutmix_inside_a_graphed_train_step(device):
    from si_mamba_amd import mixing
    from si_mamba_amd.graphed import GraphedTrainStep
    from si_mamba_amd.transforms import AugmentState
    ma = small_model(device)
    mb = copy.deepcopy(ma)
    # plain SGD, as test_gpu_model.py's graphed-against-eager comparison and for its reason
    oa = torch.optim.SGD(ma.parameters(), lr=0.002)
    ob = torch.optim.SGD(mb.parameters(), lr=0.002)
    pts = clouds(B, N, 40).to(device)
    gt = torch.randint(0, 5, (B,), generator=torch.Generator().manual_seed(1)).to(device)
    sa = AugmentState(SEED, device).manual_seed(SEED, STEP)
    sb = AugmentState(SEED, device).manual_seed(SEED, STEP)
    taken = torch.full((B,), -1, device=device, dtype=torch.int64)
    share = torch.zeros(B, device=device)

    def loss_of(model, state, p, y, record):
        mixed, partner, ratio = mixing.cutmix(p, "k", state=state)
        if record:
            taken.copy_(partner)
            share.copy_(ratio)
        return mixing.mixed_cross_entropy(model(mixed), y, partner, ratio)

    step = GraphedTrainStep(lambda p, y: loss_of(ma, sa, p, y, True), oa, (pts, gt), clip=10.0, warmup=WARMUP)
    assert sa.step == STEP + WARMUP                                  # capture itself executes nothing
    graphed, eager, partners, shares = [], [], [], []
    for k in range(WARMUP + REPLAYS):                                # the eager twin, warm-up steps included
        ob.zero_grad(set_to_none=True)
        loss = loss_of(mb, sb, pts, gt, False)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(mb.parameters(), 10.0)
        ob.step()
        if k >= WARMUP:
            eager.append(loss.item())
    for _ in range(REPLAYS):
        graphed.append(step(pts, gt).item())
        partners.append(taken.tolist())
        shares.append(share.tolist())
    assert sa.step == sb.step == STEP + WARMUP + REPLAYS
    print(f"graphed {graphed}\neager   {eager}\npartners {partners}")
    # test_gpu_model.py's bound for a graphed step against its eager twin (fp32 atomics in the reductions); the first
    # replay follows WARMUP identical steps
    assert abs(graphed[0] - eager[0]) < 2e-3, (graphed, eager)
    assert max(abs(a - b) for a, b in zip(graphed, eager)) < 2e-3, (graphed, eager)
    # every replay read the step it found: the partner maps are the restatement's for consecutive steps, and differ
    want = [mr.partner_map(B, SEED, STEP + WARMUP + k).tolist() for k in range(REPLAYS)]
    assert partners == want
    assert all(want[k] != want[k + 1] for k in range(REPLAYS - 1)), want
    assert all(shares[k] != shares[k + 1] for k in range(REPLAYS - 1)) and all(0 <= v < 1 for s in shares for v in s)
    assert all(torch.isfinite(p).all() for p in ma.parameters())
