"""CPU: si_mamba_amd.dist.FlatGradients (every gradient a view of one flat buffer, one all-reduce) and the refusals of
the data-parallel GraphedTrainStep that need no GPU.

The two-rank case runs over gloo as tests/test_dist_gloo.py does, on a small MixerModel whose mixers are the oracle's
(the HIP mixers cannot run on CPU ranks): the eager two-phase step -- backward into the flat buffer, one all-reduce,
/ world -- against the gradients DistributedDataParallel (wrap_ddp) leaves on the same ranks with the same shards.
"""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from oracle import scan_ref
from si_mamba_amd import dist as sdist
from si_mamba_amd.block import MixerModel
from si_mamba_amd.dist import FlatGradients


def _small_mixer_model():
    torch.manual_seed(0)
    m = MixerModel(32, 2, drop_path=0.)
    for layer in m.layers:
        layer.mixer = scan_ref.MambaRef(32, d_state=4)
    return m


def _loss(model, x, pos):
    return model(x, pos).square().mean()


def test_views_alias_the_buffer():
    m = _small_mixer_model()
    params = list(m.parameters())
    flat = FlatGradients(params)
    assert len(flat.buffers) == 1 and flat.params == params
    buf = flat.buffers[0]
    assert buf.dtype == torch.float32 and buf.numel() == sum(p.numel() for p in params)
    off = 0
    for p in params:
        assert p.grad.shape == p.shape and p.grad.is_contiguous()
        assert p.grad.data_ptr() == buf.data_ptr() + off * buf.element_size()
        off += p.numel()
    x, pos = torch.randn(2, 12, 32), torch.randn(2, 12, 32)
    _loss(m, x, pos).backward()                              # autograd accumulates in place: the views stay views
    assert float(buf.abs().sum()) > 0
    assert torch.equal(torch.cat([p.grad.flatten() for p in params]), buf)
    off = 0
    for p in params:
        assert p.grad.data_ptr() == buf.data_ptr() + off * buf.element_size()
        off += p.numel()
    want = torch.autograd.grad(_loss(m, x, pos), params)
    for p, g in zip(params, want):
        assert torch.equal(p.grad, g)                        # 0 + g


def test_zero_clears_every_gradient():
    m = _small_mixer_model()
    flat = FlatGradients(m.parameters())
    _loss(m, torch.randn(2, 12, 32), torch.randn(2, 12, 32)).backward()
    assert flat.zero_() is flat
    assert all(not p.grad.any() for p in m.parameters())
    assert not flat.buffers[0].any()


def test_excluded_parameter_keeps_no_gradient():
    m = _small_mixer_model()
    left_out = m.norm_f.bias
    flat = FlatGradients(m.parameters(), exclude=[left_out])
    assert left_out.grad is None
    assert all(p is not left_out for p in flat.params)
    assert flat.buffers[0].numel() == sum(p.numel() for p in m.parameters()) - left_out.numel()


def test_one_buffer_per_dtype_and_existing_gradients_are_kept():
    a = nn.Parameter(torch.randn(3, 5))
    b = nn.Parameter(torch.randn(7, dtype=torch.float64))
    c = nn.Parameter(torch.randn(2))
    a.grad = torch.full_like(a, 2.0)
    flat = FlatGradients([a, b, c, a])                       # a parameter listed twice is held once
    assert flat.params == [a, b, c]
    assert [(buf.dtype, buf.numel()) for buf in flat.buffers] == [(torch.float32, 17), (torch.float64, 7)]
    assert torch.equal(flat.buffers[0], torch.cat([torch.full((15,), 2.0), torch.zeros(2)]))
    assert c.grad.data_ptr() == flat.buffers[0].data_ptr() + 15 * 4 and b.grad.data_ptr() == flat.buffers[1].data_ptr()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, ret):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    sdist.init_dist("gloo")
    try:
        g = torch.Generator().manual_seed(7)
        x, pos = torch.randn(4, 12, 32, generator=g), torch.randn(4, 12, 32, generator=g)
        xs, ps = x[rank * 2:(rank + 1) * 2], pos[rank * 2:(rank + 1) * 2]
        ma, mb = _small_mixer_model(), _small_mixer_model()
        flat = FlatGradients(ma.parameters())
        flat.zero_()
        _loss(ma, xs, ps).backward()                         # phase A
        flat.all_reduce_(dist.group.WORLD)                   # the one collective
        flat.buffers[0].mul_(1.0 / world)                    # phase B starts here
        ddp = sdist.wrap_ddp(mb, torch.device("cpu"))        # (kept alive: its backward hook finds it by weak reference)
        _loss(ddp, xs, ps).backward()
        ret[rank] = ([p.grad.clone() for p in ma.parameters()], [p.grad.clone() for p in mb.parameters()])
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_match_ddp():
    world, port = 2, _free_port()
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    for rank in range(world):
        got, want = ret[rank]
        assert len(got) == len(want) > 0
        for a, b in zip(got, want):
            scale = float(b.abs().max())
            assert scale > 0
            assert float((a - b).abs().max()) <= 1e-6 * scale
    for a, b in zip(ret[0][0], ret[1][0]):                   # both ranks hold the same reduced bits
        assert torch.equal(a, b)


def test_process_group_without_torch_distributed_is_refused():
    from si_mamba_amd.graphed import GraphedTrainStep
    assert not dist.is_initialized()
    m = nn.Linear(4, 2)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    with pytest.raises(RuntimeError, match="torch.distributed is not initialised"):
        GraphedTrainStep(lambda x: m(x).sum(), opt, (torch.randn(3, 4),), process_group=object())


def test_sync_batchnorm_is_refused():
    from si_mamba_amd.graphed import GraphedTrainStep
    m = nn.Sequential(nn.Linear(4, 4), nn.SyncBatchNorm(4))
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    with pytest.raises(RuntimeError, match="SyncBatchNorm.*cannot be captured"):
        GraphedTrainStep(lambda x: m(x).sum(), opt, (torch.randn(3, 4),), process_group=object(), module=m)


def test_module_without_a_group_is_refused():
    from si_mamba_amd.graphed import GraphedTrainStep
    m = nn.Linear(4, 2)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    with pytest.raises(ValueError, match="process_group"):
        GraphedTrainStep(lambda x: m(x).sum(), opt, (torch.randn(3, 4),), module=m)


def test_new_arguments_are_keyword_only():
    import inspect
    from si_mamba_amd.graphed import GraphedTrainStep
    sig = inspect.signature(GraphedTrainStep.__init__).parameters
    for name, default in (("process_group", None), ("module", None), ("broadcast_buffers", True)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is default
