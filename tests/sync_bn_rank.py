"""One rank of tests/test_gpu_sync_bn.py::test_two_real_ranks (a helper, not a test file):

    python sync_bn_rank.py RANK WORLD DIR

Reads DIR/in.pt (Encoder state, the whole batch, the output gradient), runs the Encoder converted with
nn.SyncBatchNorm.convert_sync_batchnorm on this rank's share of the batch on GPU RANK, and writes DIR/outRANK.pt."""
import os
import sys

import torch
import torch.distributed as dist
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    rank, world, folder = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    from si_mamba_amd import encoder_ops
    from si_mamba_amd.point_mamba import Encoder
    dev = torch.device("cuda", rank)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", init_method=f"file://{folder}/store", rank=rank, world_size=world)
    try:
        data = torch.load(os.path.join(folder, "in.pt"))
        enc = Encoder(384)
        enc.load_state_dict(data["state"])
        enc = nn.SyncBatchNorm.convert_sync_batchnorm(enc).to(dev).train()
        per = data["pts"].shape[0] // world
        pts = data["pts"][rank * per:(rank + 1) * per].to(dev).requires_grad_(True)
        dy = data["dy"][rank * per:(rank + 1) * per].to(dev)
        taken = []
        real = encoder_ops.SyncBnReluFn.apply
        encoder_ops.SyncBnReluFn.apply = lambda *a: (taken.append(1), real(*a))[1]
        y = enc(pts)
        y.backward(dy)
        torch.cuda.synchronize()
        assert len(taken) == 2, f"the cross-rank route ran {len(taken)} times, expected both BatchNorms"
        torch.save(dict(y=y.detach().cpu(), pts_grad=pts.grad.cpu(),
                        grads={k: p.grad.cpu() for k, p in enc.named_parameters()},
                        buffers={k: b.cpu() for k, b in enc.named_buffers()}),
                   os.path.join(folder, f"out{rank}.pt"))
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
