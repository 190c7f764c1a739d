"""Streaming ops of the patch encoder on the MI355X kernels (csrc/bn_relu.hip).

  bn_relu_fn      relu(BatchNorm1d(x + g))   reference models/point_mamba.py:46-49, :52-55
                  (nn.BatchNorm1d + nn.ReLU after a 1x1 Conv1d, token-major here); ``g`` is the per-patch
                  additive term that replaces the reference's concat of the global feature (:64-66)
  group_max_fn    max over the points of a patch   reference :63, :68  (torch.max(..., dim=2)[0])

  token_linear    y = x W^T + b on a token-major (rows, C) view (the reference's 1x1 Conv1d, :44-57) whose weight
                  gradient is a split-K batched product: dW = sum_s dY_s^T X_s over 64 row slabs, fp32 partials.
                  The one-GEMM form autograd would run has K = rows = 262 144 and a (C_out, C_in) result of a few
                  tiles: the library's kernels for it leave most of the chip idle (bf16: 540-790 us per layer
                  against 44-143 us split; fp32: 443-1 778 against 156-750 us; tools/bench_wgrad_splitk.py).

  sync_bn_relu_fn the same with batch statistics over the rows of every rank of a process group (nn.SyncBatchNorm,
                  what the reference's --sync_bn puts in BatchNorm1d's place: tools/runner_finetune.py:121-122,
                  runner_pretrain.py:111-112): the kernels' stages with one all-gather of (3, C) float64 between
                  the statistics and the normalisation, and one all-reduce of (2, C) float32 between the two passes
                  of the backward

  token_linear_group_max   group_max_fn(token_linear(x, W, b)) as ONE autograd node (the encoder's last layer): the same
                  forward, and a backward that never forms the dense (rows, C_out) gradient of which the max leaves
                  one entry in n non-zero -- csrc/encoder_sparse.hip sums only the products that are not zero (1/n of
                  the two GEMMs, no atomics, bitwise repeatable); bf16 I/O, where the dense GEMMs are the faster
                  ones, and shapes outside token_linear_group_max_ok take the two separate ops

bn_relu_fn and group_max_fn are plain autograd Functions over the C ABI; BatchNorm keeps nn.BatchNorm1d's buffers (running_mean,
running_var, num_batches_tracked) and train/eval semantics.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import _lib


_BN_MAX_C = 1024     # channels per kernel call; wider layers go slice by slice (in place, row stride = C)
_BN_CHUNK = 256      # rows per workgroup in csrc/bn_relu.hip: the granularity of its per-group dx sums


_SPLITK = 64         # row slabs of token_linear's weight gradient
_SPLITK_MIN_ROWS = 512   # per slab; below it the plain product is used


class TokenLinearFn(torch.autograd.Function):
    """F.linear on (rows, C_in) tokens with a split-K weight gradient (library GEMMs; no custom kernel)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        y = torch.nn.functional.linear(x, weight, bias)       # under autocast: the reference's rounding (bf16 GEMM)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        io = dy.dtype
        rows, n_out = dy.shape
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = (dy @ weight.to(io)).to(x.dtype)
        if ctx.needs_input_grad[1]:
            xc = x.to(io).contiguous()
            if rows % _SPLITK == 0 and rows // _SPLITK >= _SPLITK_MIN_ROWS:
                m = rows // _SPLITK
                a = dy.view(_SPLITK, m, n_out).transpose(1, 2)
                b = xc.view(_SPLITK, m, xc.shape[1])
                part = torch.bmm(a, b) if io == torch.float32 else torch.bmm(a, b, out_dtype=torch.float32)
                dw = part.sum(0).to(weight.dtype)
            else:
                dw = (dy.t() @ xc).to(weight.dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.sum(0, dtype=torch.float32).to(weight.dtype)
        return dx, dw, db


def token_linear(x, weight, bias=None):
    """(rows, C_in) @ (C_out, C_in)^T + bias.  GPU tensors take the split-K weight gradient; anything else is
    torch.nn.functional.linear."""
    if x.is_cuda and x.dim() == 2 and torch.is_grad_enabled() and (weight.requires_grad or x.requires_grad):
        return TokenLinearFn.apply(x, weight, bias)
    return torch.nn.functional.linear(x, weight, bias)


def _slices(C):
    return [(c0, min(c0 + _BN_MAX_C, C)) for c0 in range(0, C, _BN_MAX_C)]


def _off(t, elems):
    """data_ptr of a contiguous tensor advanced by `elems` elements (None stays None)."""
    return None if t is None else t.data_ptr() + elems * t.element_size()


def _slice_of(g, c0, c1, C):
    return None if g is None else (g if (c0 == 0 and c1 == C) else g[:, c0:c1].contiguous())


def _bn_partial(lib, rows, C, dev):
    return torch.empty(lib.simamba_bn_relu_grid(rows), 2, min(C, _BN_MAX_C), device=dev, dtype=torch.float32)


def _bn_operands(x, gterm, weight, bias):
    """What both Functions hand to the kernels: x contiguous, the additive term and the parameters contiguous in fp32,
    and the outputs y, mean, invstd."""
    xc = x.contiguous()
    g, w, b = (None if t is None else t.float().contiguous() for t in (gterm, weight, bias))
    mean = torch.empty(xc.shape[1], device=xc.device, dtype=torch.float32)
    return xc, g, w, b, torch.empty_like(xc), mean, torch.empty_like(mean)


def _dtypes(*tensors):
    return tuple(None if t is None else t.dtype for t in tensors)


def _bn_grads(dtypes, dx, dgt, dw, db):
    """backward's tuple for (x, gterm, group, weight, bias, + 5 more), each gradient in the dtype its input had."""
    xdtype, gdtype, wdtype, bdtype = dtypes
    return (dx.to(xdtype), None if dgt is None else dgt.to(gdtype), None,
            None if wdtype is None else dw.to(wdtype), None if bdtype is None else db.to(bdtype),
            None, None, None, None, None)


def _bn_dgroup(g, group):
    # the kernel sums dx over runs of dgroup <= 256 rows; wider groups are finished by the caller
    dgroup = 0 if g is None else (group if _BN_CHUNK % group == 0 else _BN_CHUNK)
    if g is not None and dgroup == _BN_CHUNK and group % _BN_CHUNK != 0:
        raise ValueError("bn_relu_fn: group must divide 256 or be a multiple of it")
    return dgroup


def _bn_dx_slices(xc, g, group, call):
    """call(c0, c1, g's slice, dg, dgroup) per channel slice, dg (rows / dgroup, c1 - c0) for the kernel's per-group
    sums of dx; returns the gradient of g (rows / group, C) float32, or None without g."""
    rows, C = xc.shape
    dgroup = _bn_dgroup(g, group)
    dgs = []
    for c0, c1 in _slices(C):
        dg = None if g is None else torch.empty(rows // dgroup, c1 - c0, device=xc.device, dtype=torch.float32)
        dgs.append(dg)
        call(c0, c1, _slice_of(g, c0, c1, C), dg, dgroup)
    if g is None:
        return None
    dgt = dgs[0] if len(dgs) == 1 else torch.cat(dgs, dim=1)
    if dgroup != group:
        dgt = dgt.view(rows // group, group // dgroup, C).sum(1)
    return dgt


class BnReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gterm, group, weight, bias, running_mean, running_var, momentum, eps, training):
        _lib.require_gpu(x, "bn_relu_fn")
        lib = _lib.load()
        xc, g, w, b, y, mean, invstd = _bn_operands(x, gterm, weight, bias)
        rows, C = xc.shape
        dev = xc.device
        code = _lib.dtype_code(xc.dtype)
        part = _bn_partial(lib, rows, C, dev)
        with torch.cuda.device(dev), _lib.timed("bn_relu_fwd", dev):
            for c0, c1 in _slices(C):
                _lib.call("simamba_bn_relu_fwd", _off(xc, c0), _slice_of(g, c0, c1, C), int(group), _off(w, c0),
                          _off(b, c0), _off(running_mean, c0), _off(running_var, c0), float(momentum), float(eps),
                          int(bool(training)), _off(y, c0), _off(mean, c0), _off(invstd, c0), part, rows, c1 - c0,
                          C, code, device=dev)
        ctx.save_for_backward(xc, g, w, b, mean, invstd)
        ctx.meta = (int(group), bool(training), code, _dtypes(x, gterm, weight, bias))
        ctx.part = part
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, g, w, b, mean, invstd = ctx.saved_tensors
        group, training, code, dtypes = ctx.meta
        rows, C = xc.shape
        dev = xc.device
        dyc = dy.to(xc.dtype).contiguous()
        dx = torch.empty_like(xc)
        dw = torch.empty(C, device=dev, dtype=torch.float32)
        db = torch.empty(C, device=dev, dtype=torch.float32)

        def one(c0, c1, gsl, dg, dgroup):
            _lib.call("simamba_bn_relu_bwd", _off(dyc, c0), _off(xc, c0), gsl, group, _off(w, c0), _off(b, c0),
                      _off(mean, c0), _off(invstd, c0), _off(dx, c0), dg, dgroup, _off(dw, c0), _off(db, c0),
                      ctx.part, rows, c1 - c0, C, code, int(training), device=dev)
        with torch.cuda.device(dev), _lib.timed("bn_relu_bwd", dev):
            dgt = _bn_dx_slices(xc, g, group, one)
        return _bn_grads(dtypes, dx, dgt, dw, db)


# ---- the kernels' stages over plain buffers (SyncBnReluFn; the tests drive them with row shards as ranks) --------------
def bn_stats_local(xc, g, group, stats, part):
    """This rank's (count, mean, M2) per channel of xc (rows, C) (+ g[row // group]) into ``stats`` (3, C) float64."""
    rows, C = xc.shape
    code, dev = _lib.dtype_code(xc.dtype), xc.device
    for c0, c1 in _slices(C):
        _lib.call("simamba_bn_stats_local", _off(xc, c0), _slice_of(g, c0, c1, C), int(group), _off(stats, c0), C,
                  part, rows, c1 - c0, C, code, device=dev)


def bn_stats_merge(gathered, running_mean, running_var, momentum, eps, mean, invstd, count):
    """(W, 3, C) float64 blocks of all ranks -> mean, invstd (C) float32, count (1) float64, running statistics."""
    world, _, C = gathered.shape
    _lib.call("simamba_bn_stats_merge", gathered, world, running_mean, running_var, float(momentum), float(eps),
              mean, invstd, count, C, device=gathered.device)


def bn_relu_apply(xc, g, group, w, b, mean, invstd, y):
    rows, C = xc.shape
    code, dev = _lib.dtype_code(xc.dtype), xc.device
    for c0, c1 in _slices(C):
        _lib.call("simamba_bn_relu_apply", _off(xc, c0), _slice_of(g, c0, c1, C), int(group), _off(w, c0),
                  _off(b, c0), _off(mean, c0), _off(invstd, c0), _off(y, c0), rows, c1 - c0, C, code, device=dev)


def bn_relu_bwd_sums(dyc, xc, g, group, w, b, mean, invstd, sums, part):
    """This rank's sum dy*mask (``sums[0]``) and sum dy*mask*xhat (``sums[1]``); ``sums`` (2, C) float32."""
    rows, C = xc.shape
    code, dev = _lib.dtype_code(xc.dtype), xc.device
    for c0, c1 in _slices(C):
        _lib.call("simamba_bn_relu_bwd_sums", _off(dyc, c0), _off(xc, c0), _slice_of(g, c0, c1, C), int(group),
                  _off(w, c0), _off(b, c0), _off(mean, c0), _off(invstd, c0), _off(sums[1], c0), _off(sums[0], c0),
                  part, rows, c1 - c0, C, code, device=dev)


def bn_relu_bwd_dx(dyc, xc, g, group, w, b, mean, invstd, sums, count, dx):
    """dx with the sums and the row count of ALL ranks; returns the gradient of g (rows / group, C) float32 or None."""
    rows, C = xc.shape
    code, dev = _lib.dtype_code(xc.dtype), xc.device

    def one(c0, c1, gsl, dg, dgroup):
        _lib.call("simamba_bn_relu_bwd_dx", _off(dyc, c0), _off(xc, c0), gsl, int(group), _off(w, c0), _off(b, c0),
                  _off(mean, c0), _off(invstd, c0), _off(sums[1], c0), _off(sums[0], c0), count, _off(dx, c0),
                  dg, dgroup, rows, c1 - c0, C, code, device=dev)
    return _bn_dx_slices(xc, g, group, one)


class SyncBnReluFn(torch.autograd.Function):
    """relu(batch_norm(x + g)) in training mode with the statistics of every rank's rows: one all-gather of (3, C)
    float64 forward, one all-reduce of (2, C) float32 backward, however many channel slices the layer has."""

    @staticmethod
    def forward(ctx, x, gterm, group, weight, bias, running_mean, running_var, momentum, eps, process_group):
        _lib.require_gpu(x, "sync_bn_relu_fn")
        lib = _lib.load()
        xc, g, w, b, y, mean, invstd = _bn_operands(x, gterm, weight, bias)
        rows, C = xc.shape
        dev = xc.device
        world = dist.get_world_size(process_group)
        count = torch.empty(1, device=dev, dtype=torch.float64)
        stats = torch.empty(3, C, device=dev, dtype=torch.float64)
        gathered = torch.empty(world, 3, C, device=dev, dtype=torch.float64)
        part = _bn_partial(lib, rows, C, dev)
        with torch.cuda.device(dev), _lib.timed("sync_bn_relu_fwd", dev):
            bn_stats_local(xc, g, group, stats, part)
            dist.all_gather_into_tensor(gathered, stats, group=process_group)
            bn_stats_merge(gathered, running_mean, running_var, momentum, eps, mean, invstd, count)
            bn_relu_apply(xc, g, group, w, b, mean, invstd, y)
        ctx.save_for_backward(xc, g, w, b, mean, invstd, count)
        ctx.meta = (int(group), _dtypes(x, gterm, weight, bias))
        ctx.part = part
        ctx.process_group = process_group
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, g, w, b, mean, invstd, count = ctx.saved_tensors
        group, dtypes = ctx.meta
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(_CAPTURE_MSG)
        C = xc.shape[1]
        dev = xc.device
        dyc = dy.to(xc.dtype).contiguous()
        dx = torch.empty_like(xc)
        sums = torch.empty(2, C, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev), _lib.timed("sync_bn_relu_bwd", dev):
            bn_relu_bwd_sums(dyc, xc, g, group, w, b, mean, invstd, sums, ctx.part)
            local = sums.clone()             # weight / bias gradients stay this rank's sums (DDP averages them)
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=ctx.process_group)
            dgt = bn_relu_bwd_dx(dyc, xc, g, group, w, b, mean, invstd, sums, count, dx)
        return _bn_grads(dtypes, dx, dgt, local[1], local[0])


_CAPTURE_MSG = ("sync_bn_relu_fn: the stream is being captured into a graph; the collectives of cross-rank batch "
                "statistics are not supported inside a capture")


def _bn_step(bn):
    """nn.BatchNorm1d / nn.SyncBatchNorm bookkeeping of one forward: (use batch statistics, momentum, running_mean,
    running_var to hand to the kernels); counts the batch in num_batches_tracked."""
    training = bn.training or bn.running_mean is None
    momentum = bn.momentum
    if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
        if momentum is None:                       # cumulative moving average (nn.BatchNorm1d semantics)
            momentum = 1.0 / float(bn.num_batches_tracked)
    rm = bn.running_mean if (bn.track_running_stats and (bn.training or not training)) else None
    rv = bn.running_var if rm is not None else None
    return training, 0.0 if momentum is None else momentum, rm, rv


def _dist_up():
    return dist.is_available() and dist.is_initialized()


def _bn_relu_local(x, bn, gterm, group):
    training, momentum, rm, rv = _bn_step(bn)
    return BnReluFn.apply(x, gterm, group, bn.weight, bn.bias, rm, rv, momentum, bn.eps, training)


def sync_bn_relu_fn(x, bn, gterm=None, group=0, process_group=None):
    """relu(bn(x + gterm[row // group])) with training statistics over the rows of every rank of ``process_group``
    (``bn.process_group`` when None, else the default group) -- nn.SyncBatchNorm's meaning, on the HIP kernels.

    Ranks may hold different numbers of rows; each needs at least one.  The weight and bias gradients are this rank's
    own sums, as nn.SyncBatchNorm returns them.  ``bn`` outside training mode uses its running statistics: no
    collective, the same call as bn_relu_fn."""
    if not isinstance(bn, (torch.nn.BatchNorm1d, torch.nn.SyncBatchNorm)):
        raise TypeError(f"sync_bn_relu_fn: expected nn.SyncBatchNorm or nn.BatchNorm1d, got {type(bn).__name__}")
    if not bn.training:
        return _bn_relu_local(x, bn, gterm, group)
    if x.shape[0] < 1:
        raise ValueError(f"sync_bn_relu_fn: this rank holds {x.shape[0]} rows; every rank needs at least 1")
    if not _dist_up():
        raise RuntimeError("sync_bn_relu_fn: torch.distributed has no initialised process group")
    if x.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(_CAPTURE_MSG)
    if process_group is None:
        process_group = getattr(bn, "process_group", None)
    _, momentum, rm, rv = _bn_step(bn)
    return SyncBnReluFn.apply(x, gterm, group, bn.weight, bn.bias, rm, rv, momentum, bn.eps, process_group)


def _sync_world(bn):
    return dist.get_world_size(bn.process_group) if _dist_up() else 1


def bn_relu_fn(x, bn: torch.nn.BatchNorm1d, gterm=None, group=0):
    """relu(bn(x + gterm[row // group])) for token-major x (rows, C) with ``bn``'s parameters, buffers and mode.

    ``nn.BatchNorm1d`` means PER-RANK batch statistics: BnReluFn.  The ``nn.SyncBatchNorm`` that ``--sync_bn`` puts in
    its place (reference tools/runner_finetune.py:121-122, runner_pretrain.py:111-112) reduces its training
    statistics across ranks: SyncBnReluFn when it trains in a process group of more than one rank, and BnReluFn in
    eval mode (running statistics), with a single rank or with no process group, where nn.SyncBatchNorm itself is a
    plain batch norm.  Any other module type goes through the module itself (stock torch kernels on the same device),
    so its semantics are kept instead of being silently replaced."""
    if type(bn) is torch.nn.SyncBatchNorm:
        if bn.training and _sync_world(bn) > 1:
            return sync_bn_relu_fn(x, bn, gterm=gterm, group=group)
    elif type(bn) is not torch.nn.BatchNorm1d:
        if gterm is not None:
            x = x + gterm.to(x.dtype).repeat_interleave(group, dim=0)
        return torch.relu(bn(x))
    return _bn_relu_local(x, bn, gterm, group)


class GroupMaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _lib.require_gpu(x, "group_max_fn")
        xc = x.contiguous()
        groups, n, C = xc.shape
        dev = xc.device
        code = _lib.dtype_code(xc.dtype)
        out = torch.empty(groups, C, device=dev, dtype=xc.dtype)
        idx = torch.empty(groups, C, device=dev, dtype=torch.uint8)
        _lib.call("simamba_group_max_fwd", xc, out, idx, groups, n, C, code, device=dev)
        ctx.save_for_backward(idx)
        ctx.meta = (groups, n, C, code, xc.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        groups, n, C, code, dtype = ctx.meta
        d = dout.to(dtype).contiguous()
        dx = torch.empty(groups, n, C, device=d.device, dtype=dtype)
        _lib.call("simamba_group_max_bwd", d, idx, dx, groups, n, C, code, device=d.device)
        return dx


def group_max_fn(x):
    """(groups, n, C) -> (groups, C): max over the n points of each patch."""
    return GroupMaxFn.apply(x)


# ---- linear + max over the patch as one node with a sparse backward (csrc/encoder_sparse.hip) ---------------------------
_SPARSE_MAX_N = 32         # points per patch
_SPARSE_MAX_COUT = 384     # rows of W the input-gradient kernel keeps in LDS


def _linear_io_dtype(x):
    """dtype F.linear will return for x: the autocast dtype inside an autocast region, else x's own."""
    return torch.get_autocast_dtype("cuda") if (x.is_cuda and torch.is_autocast_enabled("cuda")) else x.dtype


def token_linear_group_max_ok(x, weight, n):
    """Shape limits of simamba_max_linear_bwd_dx / _dw (include/simamba.h); anything else takes token_linear +
    group_max_fn.  The one place where the route is chosen: by default fp32 I/O only, where the sparse backward was
    measured faster (_lib.sparse_max_linear_enabled); _lib.sparse_max_linear forces either route."""
    if not (x.is_cuda and x.dim() == 2 and weight.dim() == 2 and _lib.sparse_max_linear_enabled(_linear_io_dtype(x))):
        return False
    rows, cin = x.shape
    cout = weight.shape[0]
    return (1 <= n <= _SPARSE_MAX_N and rows > 0 and rows % n == 0 and cin == weight.shape[1] and cin % 64 == 0
            and cout % 4 == 0 and 4 <= cout <= _SPARSE_MAX_COUT
            and _linear_io_dtype(x) in (torch.float32, torch.bfloat16)
            and x.is_contiguous() and x.data_ptr() % 16 == 0)


class TokenLinearGroupMaxFn(torch.autograd.Function):
    """max over each run of n rows of F.linear(x, weight, bias).  Saves x, weight and the arg max (uint8): neither the
    (rows, C_out) product nor a dense gradient of it."""

    @staticmethod
    def forward(ctx, x, weight, bias, n):
        y = torch.nn.functional.linear(x, weight, bias).contiguous()     # as TokenLinearFn: autocast's rounding
        rows, cout = y.shape
        groups = rows // n
        dev = y.device
        code = _lib.dtype_code(y.dtype)
        out = torch.empty(groups, cout, device=dev, dtype=y.dtype)
        idx = torch.empty(groups, cout, device=dev, dtype=torch.uint8)
        _lib.call("simamba_group_max_fwd", y, out, idx, groups, n, cout, code, device=dev)
        ctx.save_for_backward(x, weight, idx)
        ctx.meta = (groups, int(n), code, y.dtype, bias is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, idx = ctx.saved_tensors
        groups, n, code, io, has_bias = ctx.meta
        cout, cin = weight.shape
        dev = dout.device
        d = dout.to(io).contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            w = weight.detach().to(io).contiguous()
            dx = torch.empty(groups * n, cin, device=dev, dtype=io)
            _lib.call("simamba_max_linear_bwd_dx", d, idx, w, dx, groups, n, cin, cout, code, device=dev)
            dx = dx.to(x.dtype)
        if ctx.needs_input_grad[1]:
            xc = x.detach().to(io).contiguous()
            slabs = _lib.load().simamba_max_linear_bwd_slabs(groups, cin)
            part = torch.empty(slabs, cout, cin, device=dev, dtype=torch.float32)
            dw = torch.empty(cout, cin, device=dev, dtype=torch.float32)
            _lib.call("simamba_max_linear_bwd_dw", d, idx, xc, dw, part, groups, n, cin, cout, code, device=dev)
            dw = dw.to(weight.dtype)
        if has_bias and ctx.needs_input_grad[2]:
            db = d.sum(0, dtype=torch.float32).to(weight.dtype)          # over the patches, not the points
        return dx, dw, db, None


def token_linear_group_max(x, weight, bias, n):
    """(groups * n, C_in) tokens -> (groups, C_out): max over the n points of each patch of x W^T + b.  The forward is
    token_linear followed by group_max_fn, bit for bit; within token_linear_group_max_ok (fp32 I/O by default) the
    backward skips the zeros the max leaves (TokenLinearGroupMaxFn), otherwise the two ops run as they are."""
    if token_linear_group_max_ok(x, weight, n):
        _lib.count("max_linear_sparse")
        return TokenLinearGroupMaxFn.apply(x, weight, bias, n)
    _lib.count("max_linear_dense")
    y = token_linear(x, weight, bias)
    return group_max_fn(y.view(y.shape[0] // n, n, y.shape[1]))
