"""Data-parallel plumbing: one process per GPU, torch.distributed over RCCL (backend "nccl" on ROCm).

Mirrors reference utils/dist_utils.py:9-54 (init_dist / reduce_tensor / gather_tensor) and the DDP
wrap of tools/runner_finetune.py:124-125.  The hot-path kernels have no cross-sample term, so the
only collective per step is the bucketed gradient all-reduce DDP issues on its own RCCL stream --
unless the model was converted to nn.SyncBatchNorm (--sync_bn), whose layers add one all-gather of
(3, C) float64 forward and one all-reduce of (2, C) float32 backward each (encoder_ops.sync_bn_relu_fn).

FlatGradients / FlatBroadcast serve the step that replays from hipGraphs (graphed.GraphedTrainStep with a process
group), which cannot hold DDP's hooks: every gradient a view of one buffer and ONE eager all-reduce between two
graphs, the BatchNorm statistics of rank 0 in one broadcast.
"""
from __future__ import annotations

import os

import torch
import torch.distributed as dist


def init_dist(backend: str | None = None):
    """Initialise from torchrun's env (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*).  Returns (rank, world)."""
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1 and "MASTER_ADDR" not in os.environ:
        return 0, 1
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    if backend == "nccl":
        local = int(os.environ.get("LOCAL_RANK", str(rank % max(torch.cuda.device_count(), 1))))
        torch.cuda.set_device(local)
    if not dist.is_initialized():
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, world


def one_rank_env():
    """Outside torchrun (no RANK / MASTER_ADDR in the environment): the variables of a one-rank group on a free local
    port, so that init_dist() builds a real process group -- the data-parallel path with nobody else in it."""
    if "RANK" in os.environ or "MASTER_ADDR" in os.environ:
        return
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))


def get_dist_info():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def reduce_tensor(tensor, world_size=None):
    """all-reduce(SUM) / world -- reference utils/dist_utils.py:41-48."""
    _, ws = get_dist_info()
    world_size = ws if world_size is None else world_size
    if ws == 1:
        return tensor.clone()
    rt = tensor.clone()
    dist.all_reduce(rt, op=dist.ReduceOp.SUM)
    return rt / world_size


def gather_tensor(tensor, world_size=None):
    """all-gather + cat on dim 0 -- reference utils/dist_utils.py:50-54."""
    _, ws = get_dist_info()
    if ws == 1:
        return tensor.clone()
    outs = [torch.empty_like(tensor) for _ in range(ws)]
    dist.all_gather(outs, tensor)
    return torch.cat(outs, dim=0)


def wrap_ddp(model, device=None, bucket_cap_mb: int = 64):
    """DDP tuned for xGMI: the 49 MB of fp32 gradients go out as ONE bucket (ring all-reduce is
    per-link bound, fewer/larger messages win), gradients alias the bucket, static graph."""
    if not (dist.is_available() and dist.is_initialized()):
        return model                      # plain single-process run: nothing to synchronise
    from torch.nn.parallel import DistributedDataParallel as DDP
    ids = None if device is None or device.type != "cuda" else [device.index]
    # broadcast_buffers=True is DDP's default and what the reference gets (tools/runner_finetune.py:124-125):
    # BatchNorm running statistics follow rank 0 (a few KB per step)
    return DDP(model, device_ids=ids, bucket_cap_mb=bucket_cap_mb, gradient_as_bucket_view=True,
               static_graph=True, broadcast_buffers=True)


def _by_dtype_and_device(tensors):
    groups = {}
    for t in tensors:
        groups.setdefault((t.dtype, t.device), []).append(t)
    return groups


class FlatGradients:
    """The gradients of ``params`` as views of one contiguous buffer per (dtype, device) -- in practice one fp32
    buffer, 49 MB for the classifier.

    Every ``p.grad`` becomes a view of its slice (a gradient that already exists is copied into it), and autograd
    accumulates into a gradient that exists in place, so after ``zero_()`` and a backward pass the buffers hold the
    step's gradients: ONE all-reduce per buffer sums them over the ranks, and the clip is two ops on the same
    memory.  A parameter in ``exclude`` is left out and its ``.grad`` stays as it is (``None`` for a parameter the
    loss never reaches, so the optimizer keeps skipping it).  ``zero_grad(set_to_none=True)`` on the parameters
    undoes the aliasing: zero with ``zero_()``.  Works on CPU tensors as well."""

    def __init__(self, params, exclude=()):
        skip = {id(p) for p in exclude}
        self.params = []
        for p in params:
            if id(p) not in skip:
                skip.add(id(p))                                   # a parameter listed twice is held once
                self.params.append(p)
        self.buffers = []
        for (dtype, device), ps in _by_dtype_and_device(self.params).items():
            buf = torch.zeros(sum(p.numel() for p in ps), dtype=dtype, device=device)
            off = 0
            for p in ps:
                view = buf[off:off + p.numel()].view_as(p)
                if p.grad is not None:
                    view.copy_(p.grad)
                p.grad = view
                off += p.numel()
            self.buffers.append(buf)

    def zero_(self):
        for buf in self.buffers:
            buf.zero_()
        return self

    def all_reduce_(self, group=None):
        """Sum over the ranks of ``group``, one collective per buffer (the caller divides by the world size)."""
        for buf in self.buffers:
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
        return self


class FlatBroadcast:
    """``tensors`` sent from the group's first rank in one collective per (dtype, device): the sender packs them into
    a flat staging tensor it keeps, the others unpack -- one copy kernel on either side.  BatchNorm's running
    statistics go this way before a step, as DistributedDataParallel(broadcast_buffers=True) sends them."""

    def __init__(self, tensors, group=None):
        self.group = group
        self.src = dist.get_global_rank(group, 0) if group is not None else 0
        self.sender = dist.get_rank() == self.src
        self.sets = []
        for (dtype, device), ts in _by_dtype_and_device(tensors).items():
            flat = torch.empty(sum(t.numel() for t in ts), dtype=dtype, device=device)
            self.sets.append((flat, ts, [v.view_as(t) for v, t in zip(flat.split([t.numel() for t in ts]), ts)]))

    @torch.no_grad()
    def __call__(self):
        for flat, tensors, views in self.sets:
            if self.sender:
                torch._foreach_copy_(views, tensors)
            dist.broadcast(flat, self.src, group=self.group)
            if not self.sender:
                torch._foreach_copy_(tensors, views)
