"""The models and steps of tests/test_gpu_graphed_dp.py, and one rank of its two-rank cases (a helper, not a test file):

    python graphed_dp_rank.py RANK WORLD DIR BACKEND

Reads DIR/in.pt (the PointMamba state of rank 0, 5 batches of 8 clouds with labels), takes this rank's half of every
batch and runs 3 warm-up + 4 steps of the data-parallel GraphedTrainStep (rank 1 starts from its own initialisation:
the constructor's broadcast has to replace it), then the same steps eagerly on a copy with one all-reduce per gradient.
Writes DIR/outRANK.pt: both loss series, the worst parameter difference, and the parameters and floating-point
buffers after a last ``sync_buffers()``.  BACKEND gloo puts every rank on GPU 0, nccl puts rank r on GPU r.
Exit status 77 with DIR/refusedRANK.txt: this build's gloo does not take device tensors."""
import copy
import datetime
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import clouds  # noqa: E402  (run as a script: its own directory, tests/, leads sys.path)

CLIP, LR = 10.0, 0.002


def no_dropout(model):
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return model


def small_pointmamba(device):
    """The model of tests/test_gpu_model.py::test_graphed_train_step_matches_eager."""
    from si_mamba_amd.point_mamba import PointMamba, default_config
    cfg = default_config(trans_dim=64, encoder_dims=64, depth=2, num_group=32, group_size=16, cls_dim=5,
                         drop_path=0., knn_graph=8)
    return no_dropout(PointMamba(cfg).to(device).train())


def cls_batches(n, B, N):
    return [(clouds(B, N, 20 + i), torch.randint(0, 5, (B,), generator=torch.Generator().manual_seed(i)))
            for i in range(n)]


def cls_loss(model):
    return lambda p, y: model.get_loss_acc(model(p), y)[0]


def eager_step(model, opt, loss_fn, inputs, group=None):
    """The eager (data-parallel) step: rank 0's floating-point buffers, backward, one all-reduce per gradient, mean,
    clip_grad_norm_, update.  -> (loss, norm before clipping)"""
    world = 1 if group is None else dist.get_world_size(group)
    if world > 1:
        for b in model.buffers():
            if b.is_floating_point():
                dist.broadcast(b, 0, group=group)
    opt.zero_grad(set_to_none=True)
    loss = loss_fn(*inputs)
    loss.backward()
    if world > 1:
        for p in model.parameters():
            if p.grad is not None:
                dist.all_reduce(p.grad, group=group)
                p.grad /= world
    norm = torch.nn.utils.clip_grad_norm_(model.parameters(), CLIP)
    opt.step()
    return loss.detach(), norm


def graphed_against_eager(ma, mb, make_loss, data, group, warmup=3):
    """``warmup`` + len(data) - 1 steps of the data-parallel GraphedTrainStep on ``ma`` and of eager_step on ``mb``
    (plain SGD, see test_graphed_train_step_matches_eager).  -> (step, graphed losses, eager losses)"""
    from si_mamba_amd.graphed import GraphedTrainStep
    oa = torch.optim.SGD(ma.parameters(), lr=LR)
    ob = torch.optim.SGD(mb.parameters(), lr=LR)
    step = GraphedTrainStep(make_loss(ma), oa, data[0], clip=CLIP, warmup=warmup, process_group=group, module=ma)
    la = [step(*d).item() for d in data[1:]]
    fb = make_loss(mb)
    for _ in range(warmup):                        # the graphed object took its warm-up steps on data[0]: mirror them
        eager_step(mb, ob, fb, data[0], group)
    lb = [eager_step(mb, ob, fb, d, group)[0].item() for d in data[1:]]
    return step, la, lb


def worst_difference(ma, mb):
    return max(float((pa.detach() - pb.detach()).abs().max()) for pa, pb in zip(ma.parameters(), mb.parameters()))


def main():
    rank, world, folder, backend = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, init_method=f"file://{folder}/store", rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    try:
        if backend == "gloo":
            try:
                dist.all_reduce(torch.ones(1, device=dev))
            except RuntimeError as e:
                with open(os.path.join(folder, f"refused{rank}.txt"), "w") as fh:
                    fh.write(str(e))
                return 77
        blob = torch.load(os.path.join(folder, "in.pt"))
        torch.manual_seed(100 + rank)
        ma = small_pointmamba(dev)
        mb = copy.deepcopy(ma)
        mb.load_state_dict(blob["state"])
        if rank == 0:
            ma.load_state_dict(blob["state"])
        per = blob["data"][0][0].shape[0] // world
        data = [tuple(t[rank * per:(rank + 1) * per].to(dev) for t in d) for d in blob["data"]]
        step, la, lb = graphed_against_eager(ma, mb, cls_loss, data, dist.group.WORLD)
        worst = worst_difference(ma, mb)
        step.sync_buffers()                                        # the statistics the next step would start from
        torch.cuda.synchronize()
        torch.save(dict(graphed=la, eager=lb, worst=worst, params=[p.detach().cpu() for p in ma.parameters()],
                        buffers={k: b.cpu() for k, b in ma.named_buffers() if b.is_floating_point()}),
                   os.path.join(folder, f"out{rank}.pt"))
        return 0
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main())
