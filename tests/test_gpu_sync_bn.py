"""GPU: BatchNorm+ReLU with batch statistics over the rows of several ranks (nn.SyncBatchNorm on csrc/bn_relu.hip).

The stages (simamba_bn_stats_local / _merge / simamba_bn_relu_apply / _bwd_sums / _bwd_dx) are plain functions of
buffers, so W ranks are W row shards of one tensor in one process: local statistics per shard, stacked to (W, 3, C)
and merged, apply per shard, local sums per shard added up (the all-reduce), dx per shard.  They are driven through
the slice loops of encoder_ops that SyncBnReluFn itself runs.  Oracle: float64 F.batch_norm(training=True) + relu
with autograd on the concatenation of the shards (+ gterm.repeat_interleave(group)).

Bars (tests/test_gpu_encoder.py's): normalised max error < 1e-4 for fp32 y / running_mean / running_var, < 5e-4 for
dx / dgterm / sum dweight / sum dbias; bf16 2e-2 and 1e-1.

Shapes: the smallest that reach each path of the kernels (256 rows per workgroup).  A group of 512 rows has to divide
every shard, so the two-slice case with a group wider than a chunk uses shards of 512 and 1024 rows; shards of 256 and
1024 rows at C = 1280 run with a group of 256."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from helpers import peak_err

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1


def _bounds(shards):
    out, r = [], 0
    for n in shards:
        out.append((r, r + n))
        r += n
    return out


def run_staged(x, gt, group, dy, w, b, shards, rm=None, rv=None):
    """The five stages over row shards of x; returns a dict of everything they produce."""
    from si_mamba_amd import _lib
    from si_mamba_amd import encoder_ops as eo
    lib = _lib.load()
    dev, C, W = x.device, x.shape[1], len(shards)
    sl = _bounds(shards)
    xs = [x[a:z] for a, z in sl]
    dys = [dy[a:z] for a, z in sl]
    gs = [None if gt is None else gt[a // group:z // group] for a, z in sl]
    parts = [eo._bn_partial(lib, n, C, dev) for n in shards]
    gathered = torch.empty(W, 3, C, device=dev, dtype=torch.float64)
    for i in range(W):
        eo.bn_stats_local(xs[i], gs[i], group, gathered[i], parts[i])
    mean = torch.empty(C, device=dev)
    invstd = torch.empty(C, device=dev)
    count = torch.empty(1, device=dev, dtype=torch.float64)
    eo.bn_stats_merge(gathered, rm, rv, MOM, EPS, mean, invstd, count)
    y = torch.empty_like(x)
    for i, (a, z) in enumerate(sl):
        eo.bn_relu_apply(xs[i], gs[i], group, w, b, mean, invstd, y[a:z])
    total = torch.zeros(2, C, device=dev)
    for i in range(W):
        sums = torch.empty(2, C, device=dev)
        eo.bn_relu_bwd_sums(dys[i], xs[i], gs[i], group, w, b, mean, invstd, sums, parts[i])
        total += sums
    dx = torch.empty_like(x)
    dgs = [eo.bn_relu_bwd_dx(dys[i], xs[i], gs[i], group, w, b, mean, invstd, total, count, dx[a:z])
           for i, (a, z) in enumerate(sl)]
    return dict(y=y, dx=dx, dgt=None if gt is None else torch.cat(dgs), dbias=total[0], dweight=total[1], mean=mean,
                invstd=invstd, count=count, gathered=gathered)


def oracle(x, gt, group, dy, w, b):
    """float64 batch_norm(training=True) + relu with autograd on all rows; running statistics from zeros / ones."""
    xd = x.double().clone().requires_grad_(True)
    gd = None if gt is None else gt.double().clone().requires_grad_(True)
    wd, bd = w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
    C = x.shape[1]
    rm = torch.zeros(C, device=x.device, dtype=torch.float64)
    rv = torch.ones(C, device=x.device, dtype=torch.float64)
    xe = xd if gd is None else xd + gd.repeat_interleave(group, dim=0)
    y = torch.relu(F.batch_norm(xe, rm, rv, wd, bd, True, MOM, EPS))
    y.backward(dy.double())
    return dict(y=y.detach(), dx=xd.grad, dgt=None if gd is None else gd.grad, dweight=wd.grad, dbias=bd.grad, rm=rm,
                rv=rv, var=xe.detach().var(0, unbiased=False))


def make_case(shards, C, group, dtype, device, seed):
    g = torch.Generator().manual_seed(seed)
    rows = sum(shards)
    x = (torch.randn(rows, C, generator=g) * 2 + 0.7).to(device).to(dtype)
    gt = torch.randn(rows // group, C, generator=g).to(device) if group else None
    dy = torch.randn(rows, C, generator=g).to(device).to(dtype)
    w = (torch.rand(C, generator=g) + 0.5).to(device)
    b = (torch.randn(C, generator=g) * 0.3).to(device)
    return x, gt, dy, w, b


CASES = [((64, 256, 300), 8, 0, torch.float32),        # less than a chunk, exactly one, a ragged tail; 2 lanes per row
         ((512, 768), 512, 32, torch.float32),         # group term, dgterm per-group sums
         ((256, 1024), 1280, 256, torch.float32),      # two channel slices and ld
         ((512, 1024), 1280, 512, torch.float32),      # ... and a group wider than a chunk, finished on the host
         ((1024, 512, 512), 256, 32, torch.bfloat16)]  # bf16 I/O


@pytest.mark.parametrize("shards,C,group,dtype", CASES)
def test_staged_shards_match_float64(shards, C, group, dtype, device):
    x, gt, dy, w, b = make_case(shards, C, group, dtype, device, sum(shards) + C)
    rm, rv = torch.zeros(C, device=device), torch.ones(C, device=device)
    got = run_staged(x, gt, group, dy, w, b, shards, rm, rv)
    want = oracle(x, gt, group, dy, w, b)
    torch.cuda.synchronize()
    tol, gtol = (1e-4, 5e-4) if dtype == torch.float32 else (2e-2, 1e-1)
    errs = dict(y=peak_err(got["y"], want["y"]), running_mean=peak_err(rm, want["rm"]), running_var=peak_err(rv, want["rv"]),
                dx=peak_err(got["dx"], want["dx"]), dweight=peak_err(got["dweight"], want["dweight"]),
                dbias=peak_err(got["dbias"], want["dbias"]))
    if gt is not None:
        errs["dgterm"] = peak_err(got["dgt"], want["dgt"])
    print(shards, C, group, dtype, errs)
    assert float(got["count"]) == sum(shards)
    for k in ("y", "running_mean", "running_var"):
        assert errs[k] < tol, (k, errs)
    for k in ("dx", "dweight", "dbias", "dgterm"):
        assert errs.get(k, 0.0) < gtol, (k, errs)
    # running_var takes the unbiased variance of the TOTAL count: the update formed with a shard's count instead is
    # told apart by the same bar
    # (fp32 cases: at bf16's bar of 2e-2 the two updates, 1e-4 apart at these counts, are not distinguishable)
    if dtype == torch.float32:
        n0 = shards[0]
        wrong = (1 - MOM) * 1.0 + MOM * want["var"] * n0 / (n0 - 1)
        assert peak_err(wrong, want["rv"]) > tol
        assert peak_err(rv, wrong) > tol


def test_merge_is_bitwise_repeatable_and_in_rank_order(device):
    shards, C = (64, 256, 300), 8
    x, gt, dy, w, b = make_case(shards, C, 0, torch.float32, device, 3)
    got = run_staged(x, gt, 0, dy, w, b, shards)
    from si_mamba_amd import encoder_ops as eo
    outs = []
    for _ in range(2):
        mean, invstd = torch.empty(C, device=device), torch.empty(C, device=device)
        count = torch.empty(1, device=device, dtype=torch.float64)
        eo.bn_stats_merge(got["gathered"], None, None, MOM, EPS, mean, invstd, count)
        outs.append((mean, invstd))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0], got["mean"]) and torch.equal(outs[0][1], got["invstd"])
    # the blocks are this rank's own count, mean and M2, free of the shard's shift
    a, z = _bounds(shards)[2]
    xs = x[a:z].double()
    blk = got["gathered"][2]
    assert torch.equal(blk[0], torch.full((C,), 300.0, device=device, dtype=torch.float64))
    assert peak_err(blk[1], xs.mean(0)) < 1e-6
    # fp32 partial sums: at most ~130 sequential additions per channel (2^-24 each), about a first row that may lie
    # a few standard deviations off the mean (S2 up to ~10x M2)
    assert peak_err(blk[2], ((xs - xs.mean(0)) ** 2).sum(0)) < 1e-4


@pytest.mark.parametrize("rows,C,group", [(300, 8, 0), (1024, 512, 32)])
def test_one_rank_equals_the_monolithic_forward(rows, C, group, device):
    """W = 1: mean and invstd are those simamba_bn_relu_fwd writes (1e-6 relative), and so are the running statistics."""
    from si_mamba_amd import _lib
    lib = _lib.load()
    x, gt, dy, w, b = make_case((rows,), C, group, torch.float32, device, rows)
    rm, rv = torch.zeros(C, device=device), torch.ones(C, device=device)
    got = run_staged(x, gt, group, dy, w, b, (rows,), rm, rv)
    rm1, rv1 = torch.zeros(C, device=device), torch.ones(C, device=device)
    mean, invstd, y = torch.empty(C, device=device), torch.empty(C, device=device), torch.empty_like(x)
    part = torch.empty(lib.simamba_bn_relu_grid(rows), 2, C, device=device)
    rc = lib.simamba_bn_relu_fwd(x.data_ptr(), _lib.ptr(gt), group, w.data_ptr(), b.data_ptr(), rm1.data_ptr(),
                                 rv1.data_ptr(), MOM, EPS, 1, y.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                 part.data_ptr(), rows, C, 0, 0, _lib.stream_ptr(device))
    assert rc == 0
    torch.cuda.synchronize()
    torch.testing.assert_close(got["mean"], mean, rtol=1e-6, atol=0)
    torch.testing.assert_close(got["invstd"], invstd, rtol=1e-6, atol=0)
    torch.testing.assert_close(rm, rm1, rtol=1e-6, atol=0)
    torch.testing.assert_close(rv, rv1, rtol=1e-6, atol=0)
    assert peak_err(got["y"], y) < 1e-6


@pytest.mark.parametrize("rows,C,group,ld,dtype", [
    (300, 8, 0, 0, torch.float32),           # a ragged tail, two threads per row
    (1024, 512, 32, 0, torch.float32),       # the group term and the per-group sums of dx
    (512, 8, 0, 16, torch.float32),          # channels 8..15 of a 16-wide tensor, in place
    (512, 256, 32, 0, torch.bfloat16)])
def test_fused_and_staged_entry_points_are_the_same_passes(rows, C, group, ld, dtype, device):
    """Raw ABI, one rank: simamba_bn_relu_apply with the mean / invstd simamba_bn_relu_fwd wrote gives the fused y, and
    simamba_bn_relu_bwd_sums + _bwd_dx with them and count = rows give simamba_bn_relu_bwd's dx, dgterm, dweight and
    dbias -- bit for bit: the same kernels on the same inputs, no atomics."""
    from si_mamba_amd import _lib
    lib = _lib.load()
    width = ld or C
    c0 = width - C
    x, gt, dy, w, b = make_case((rows,), width, group, dtype, device, rows + C)
    code, st = _lib.dtype_code(dtype), _lib.stream_ptr(device)

    def at(t):                                               # the slice's first element
        return t.data_ptr() + c0 * t.element_size()

    def f32(*shape):
        return torch.zeros(*shape, device=device)
    part = f32(lib.simamba_bn_relu_grid(rows), 2, C)
    mean, invstd = f32(C), f32(C)
    count = torch.full((1,), float(rows), device=device, dtype=torch.float64)
    dgroup = group
    fused = dict(y=torch.zeros_like(x), dx=torch.zeros_like(x), dw=f32(C), db=f32(C),
                 dg=f32(rows // group, C) if group else None)
    staged = {k: None if v is None else torch.zeros_like(v) for k, v in fused.items()}
    args = (at(x), _lib.ptr(gt), group, at(w), at(b))
    assert lib.simamba_bn_relu_fwd(*args, None, None, MOM, EPS, 1, at(fused["y"]), mean.data_ptr(), invstd.data_ptr(),
                                   part.data_ptr(), rows, C, ld, code, st) == 0
    assert lib.simamba_bn_relu_apply(*args, mean.data_ptr(), invstd.data_ptr(), at(staged["y"]), rows, C, ld, code,
                                     st) == 0
    args = (at(dy),) + args + (mean.data_ptr(), invstd.data_ptr())
    o = fused
    assert lib.simamba_bn_relu_bwd(*args, at(o["dx"]), _lib.ptr(o["dg"]), dgroup, o["dw"].data_ptr(),
                                   o["db"].data_ptr(), part.data_ptr(), rows, C, ld, code, 1, st) == 0
    o = staged
    assert lib.simamba_bn_relu_bwd_sums(*args, o["dw"].data_ptr(), o["db"].data_ptr(), part.data_ptr(), rows, C, ld,
                                        code, st) == 0
    assert lib.simamba_bn_relu_bwd_dx(*args, o["dw"].data_ptr(), o["db"].data_ptr(), count.data_ptr(), at(o["dx"]),
                                      _lib.ptr(o["dg"]), dgroup, rows, C, ld, code, st) == 0
    torch.cuda.synchronize()
    assert float(fused["y"].float().abs().sum()) > 0 and float(fused["dx"].float().abs().sum()) > 0
    for k, v in fused.items():
        if v is not None:
            assert torch.equal(staged[k], v), k
    if c0:                                                   # the other channels of the wide tensor are left alone
        assert not fused["y"][:, :c0].any() and not fused["dx"][:, :c0].any()


def test_large_mean_is_stable_across_shards(device):
    """Two shards whose first rows, and hence shifts, differ; channel means 1000x the spread must not cancel in the
    merge (the bar of test_bn_relu_large_mean_is_stable)."""
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(8192, 64, generator=g) * 0.01 + 10.0).to(device)
    assert not torch.equal(x[0], x[4096])
    w, b = torch.ones(64, device=device), torch.zeros(64, device=device)
    got = run_staged(x, None, 0, torch.zeros_like(x), w, b, (4096, 4096))
    ref = torch.relu(F.batch_norm(x.double(), None, None, w.double(), b.double(), True))
    err = peak_err(got["y"], ref)
    print("large mean, two shards:", err)
    assert err < 2e-3


@pytest.fixture
def one_rank_group(tmp_path, device):
    import torch.distributed as dist
    assert not dist.is_initialized()
    torch.cuda.set_device(device)
    dist.init_process_group("nccl", init_method=f"file://{tmp_path}/store", rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("C,group,momentum", [(512, 32, 0.1), (1280, 0, None)])
def test_function_at_world_size_one(C, group, momentum, device, one_rank_group):
    """sync_bn_relu_fn on nn.SyncBatchNorm under a one-rank group (collectives and all) against bn_relu_fn on an
    identically initialised nn.BatchNorm1d: outputs, input and parameter gradients, buffers, num_batches_tracked."""
    from si_mamba_amd.encoder_ops import bn_relu_fn, sync_bn_relu_fn
    rows = 768
    x, gt, dy, w, b = make_case((rows,), C, group, torch.float32, device, C)
    bn_a, bn_b = nn.SyncBatchNorm(C, momentum=momentum).to(device), nn.BatchNorm1d(C, momentum=momentum).to(device)
    with torch.no_grad():
        bn_a.weight.copy_(w); bn_a.bias.copy_(b)
        bn_b.load_state_dict(bn_a.state_dict())
    res = []
    for fn, bn in ((sync_bn_relu_fn, bn_a), (bn_relu_fn, bn_b)):
        for _ in range(2):                                  # two steps: the running buffers move twice
            bn.zero_grad()
            xa = x.clone().requires_grad_(True)
            ga = None if gt is None else gt.clone().requires_grad_(True)
            y = fn(xa, bn, gterm=ga, group=group)
            y.backward(dy)
        res.append((y, xa.grad, None if ga is None else ga.grad))
    (ya, dxa, dga), (yb, dxb, dgb) = res
    assert peak_err(ya, yb) < 1e-4
    assert peak_err(dxa, dxb) < 5e-4
    if gt is not None:
        assert peak_err(dga, dgb) < 5e-4
    assert peak_err(bn_a.weight.grad, bn_b.weight.grad) < 5e-4
    assert peak_err(bn_a.bias.grad, bn_b.bias.grad) < 5e-4
    assert peak_err(bn_a.running_mean, bn_b.running_mean) < 1e-4
    assert peak_err(bn_a.running_var, bn_b.running_var) < 1e-4
    assert int(bn_a.num_batches_tracked) == int(bn_b.num_batches_tracked) == 2


def test_dispatch_of_sync_batchnorm(device, one_rank_group, monkeypatch):
    """bn_relu_fn with nn.SyncBatchNorm: eval mode is the fused eval path, bit for bit what nn.BatchNorm1d gets; training
    with one rank is BnReluFn (as nn.SyncBatchNorm itself does); training with more ranks is SyncBnReluFn."""
    from si_mamba_amd import encoder_ops as eo
    C, group = 512, 32
    x, gt, dy, w, b = make_case((512,), C, group, torch.float32, device, 11)
    bn_a, bn_b = nn.SyncBatchNorm(C).to(device), nn.BatchNorm1d(C).to(device)
    with torch.no_grad():
        bn_a.weight.copy_(w); bn_a.bias.copy_(b)
        bn_a.running_mean.normal_(); bn_a.running_var.uniform_(0.5, 2.0)
        bn_b.load_state_dict(bn_a.state_dict())
    called = []
    real = eo.sync_bn_relu_fn
    monkeypatch.setattr(eo, "sync_bn_relu_fn", lambda *a, **k: (called.append(1), real(*a, **k))[1])
    bn_a.eval(); bn_b.eval()
    with torch.no_grad():
        assert torch.equal(eo.bn_relu_fn(x, bn_a, gterm=gt, group=group), eo.bn_relu_fn(x, bn_b, gterm=gt, group=group))
    bn_a.train(); bn_b.train()
    assert torch.equal(eo.bn_relu_fn(x, bn_a, gterm=gt, group=group), eo.bn_relu_fn(x, bn_b, gterm=gt, group=group))
    assert not called
    monkeypatch.setattr(eo, "_sync_world", lambda bn: 2)     # what a two-rank group answers
    ya = eo.bn_relu_fn(x, bn_a, gterm=gt, group=group)
    assert called == [1]
    assert peak_err(ya, eo.bn_relu_fn(x, bn_b, gterm=gt, group=group)) < 1e-4


def test_capture_is_refused(device, one_rank_group, monkeypatch):
    """A collective cannot be captured into a graph: the call says so instead of issuing one (the answer of
    torch.cuda.is_current_stream_capturing is supplied here; nothing is captured)."""
    from si_mamba_amd.encoder_ops import sync_bn_relu_fn
    bn = nn.SyncBatchNorm(8).to(device)
    x = torch.randn(64, 8, device=device)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="captured into a graph"):
        sync_bn_relu_fn(x, bn)
    assert int(bn.num_batches_tracked) == 0


def _compare_encoders(ya, pa_grad, grads_a, bufs_a, enc_b, yb, pb_grad):
    """The bars of test_encoder_fused_matches_composed."""
    assert peak_err(ya, yb) < 1e-4
    assert peak_err(pa_grad, pb_grad) < 2e-3
    for k, b in enc_b.named_parameters():
        a = grads_a[k]
        if k in ("first_conv.0.bias", "first_conv.3.bias", "second_conv.0.bias"):
            # biases in front of a BatchNorm: the gradient is exactly 0, both sides hold rounding noise
            assert float(a.abs().max()) < 1e-4 and float(b.grad.abs().max()) < 1e-4, k
        else:
            assert peak_err(a, b.grad) < 2e-3, k
    for k, b in enc_b.named_buffers():
        assert peak_err(bufs_a[k], b) < 1e-4, k


def test_encoder_with_sync_batchnorm(device, one_rank_group, monkeypatch):
    """Encoder converted with convert_sync_batchnorm, its BatchNorms on the cross-rank route (one-rank group), against
    the composed torch path with plain BatchNorm."""
    from si_mamba_amd import encoder_ops as eo
    from si_mamba_amd import point_mamba
    from si_mamba_amd.point_mamba import Encoder
    torch.manual_seed(0)
    enc_b = Encoder(384).to(device)
    enc_a = Encoder(384).to(device)
    enc_a.load_state_dict(enc_b.state_dict())
    enc_a = nn.SyncBatchNorm.convert_sync_batchnorm(enc_a)
    assert type(enc_a.first_conv[1]) is nn.SyncBatchNorm and type(enc_a.second_conv[1]) is nn.SyncBatchNorm
    enc_b.fused = False
    enc_a.train(); enc_b.train()
    calls = []
    monkeypatch.setattr(point_mamba, "bn_relu_fn",
                        lambda *a, **k: (calls.append(1), eo.sync_bn_relu_fn(*a, **k))[1])
    pts = torch.randn(4, 16, 32, 3, device=device)
    dy = torch.randn(4, 16, 384, device=device)
    pa, pb = pts.clone().requires_grad_(True), pts.clone().requires_grad_(True)
    ya, yb = enc_a(pa), enc_b(pb)
    ya.backward(dy); yb.backward(dy)
    assert len(calls) == 2
    _compare_encoders(ya, pa.grad, {k: p.grad for k, p in enc_a.named_parameters()}, dict(enc_a.named_buffers()),
                      enc_b, yb, pb.grad)


def test_two_real_ranks(device, tmp_path):
    """Two processes, one GPU each: the converted Encoder on each half of a batch against one plain-BatchNorm Encoder on
    the whole batch -- outputs, input gradients, the ranks' parameter gradients added up, and the buffers."""
    if torch.cuda.device_count() < 2:
        pytest.skip(f"needs 2 GPUs, this machine has {torch.cuda.device_count()}")
    from si_mamba_amd.point_mamba import Encoder
    torch.manual_seed(0)
    enc = Encoder(384).to(device).train()
    pts = torch.randn(8, 16, 32, 3, device=device)
    dy = torch.randn(8, 16, 384, device=device)
    torch.save(dict(state=enc.state_dict(), pts=pts.cpu(), dy=dy.cpu()), tmp_path / "in.pt")
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sync_bn_rank.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, helper, str(r), "2", str(tmp_path)])
             for r in range(2)]
    codes = []
    for p in procs:
        codes.append(p.wait())
        if codes[-1] != 0:                                   # stop at the first failure, no second try
            for q in procs:
                if q.poll() is None:
                    q.kill()
                    q.wait()
            break
    assert codes == [0, 0], f"rank exit statuses {codes}"
    pb = pts.clone().requires_grad_(True)
    yb = enc(pb)
    yb.backward(dy)
    outs = [torch.load(tmp_path / f"out{r}.pt") for r in range(2)]
    ya = torch.cat([o["y"] for o in outs])
    pg = torch.cat([o["pts_grad"] for o in outs])
    grads = {k: outs[0]["grads"][k] + outs[1]["grads"][k] for k in outs[0]["grads"]}
    for k, v in outs[0]["buffers"].items():                  # every rank holds the same statistics
        assert torch.equal(v, outs[1]["buffers"][k]), k
    _compare_encoders(ya, pg, grads, outs[0]["buffers"], enc, yb, pb.grad)
