"""hipGraph capture of a fixed-shape forward (inference / evaluation) or of a whole training step.

A PointMamba forward is ~900 kernel launches; at evaluation batch sizes (the reference tests with B = 32,
tools/runner_finetune.py:427-467) the GPU finishes them faster than Python can enqueue them.  Every op of this
package only enqueues on the stream it is handed and allocates through PyTorch's caching allocator, so the
whole forward -- HIP kernels, hipBLASLt GEMMs and the side-stream eigen-ordering with its two event joins --
captures into one hipGraph and replays with a single launch.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from .dist import FlatBroadcast, FlatGradients
from .optim import AdamW as _HipAdamW


class GraphedForward:
    """Capture ``module(*example_inputs)`` once (no grad), then ``__call__`` copies new inputs into the static
    buffers, replays the graph and returns the static output tensor(s)."""

    def __init__(self, module, *example_inputs, warmup: int = 3):
        if not all(t.is_cuda for t in example_inputs):
            raise RuntimeError("GraphedForward needs CUDA/ROCm tensors")
        self.module = module
        self.static_in = [t.clone() for t in example_inputs]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):           # lazy initialisations (library handles, LDS attributes) happen here
                module(*self.static_in)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.static_out = module(*self.static_in)

    @torch.no_grad()
    def __call__(self, *inputs):
        for dst, src in zip(self.static_in, inputs):
            dst.copy_(src)
        self.graph.replay()
        return self.static_out


class GraphedTrainStep:
    """Capture one whole training step -- zero_grad, forward, loss, backward, optional gradient clipping, optimizer
    step -- in hipGraphs: one graph in a single process, two graphs around the one gradient all-reduce in a
    data-parallel run (one process per GPU).

        step = GraphedTrainStep(lambda pts, gt: loss_fn(model(pts), gt), optimizer, (pts, gt), params=..., clip=10.0)
        loss = step(new_pts, new_gt)        # copies the inputs into the static buffers, replays, returns the loss

    The small-batch configurations (MAE pre-training at 64 clouds, part segmentation at 16) are launch-bound in
    eager mode: ~2 000 launches per step against 15-20 ms of GPU work.  Requirements: an optimizer built with
    ``capturable=True``, no host synchronisation inside ``loss_fn`` (no ``.item()``, no shape that depends on data).
    Random ops (DropPath, Dropout, the HLT tie-break) draw from the graph-safe Philox stream.

    Sampling and augmentation belong inside ``loss_fn`` (transforms.sample_and_augment: one launch, its random numbers
    keyed by a device-side ``AugmentState`` that every replay reads and advances, so each step draws anew); the subset
    of the sampled points is a static input like any other, drawn on the device before the call:

        state = AugmentState(seed, device)                       # before the capture: it copies from the host
        def loss_fn(raw, fps_idx, sel, gt):
            return criterion(model(sample_and_augment(raw, train_transforms, idx=fps_idx, sel=sel, state=state)), gt)
        step = GraphedTrainStep(loss_fn, optimizer, (raw, fps_idx, sel, gt), clip=10.0)
        loss = step(raw, fps_idx, torch.randperm(point_all, device=device)[:npoints], gt)

    Data-parallel (``process_group=``, keyword-only; ``dist.group.WORLD`` for the default group):

        init_dist()
        step = GraphedTrainStep(loss_fn, optimizer, (pts, gt), clip=10.0, process_group=dist.group.WORLD, module=model)
        loss = step(pts_of_this_rank, gt_of_this_rank)          # the local loss; dist.reduce_tensor averages it

    A collective cannot be captured, so the step is two graphs with the all-reduce between them, and the gradients
    live in one flat buffer (dist.FlatGradients) so that it is ONE collective:

        [broadcast of ``module``'s floating-point buffers from rank 0, one collective, eager]
        graph A   flat.zero_(); loss = loss_fn(*static_in); loss.backward()
        flat.all_reduce_()                                      # eager, on the current stream
        graph B   flat *= 1 / world; [norm = |flat|; flat *= min(1, clip / (norm + 1e-6))]; optimizer.step()

    The clip is clip_grad_norm_'s arithmetic on the flat buffer; the norm before clipping stays in ``self.grad_norm``.
    Construction broadcasts the parameters (and ``module``'s buffers) from rank 0 as DistributedDataParallel's
    constructor does, and runs the warm-up steps eagerly in the same two-phase form, collective included: every rank
    constructs at the same time.  A parameter that the first warm-up step leaves without a gradient stays outside
    the flat buffer with ``.grad = None``, so the optimizer skips it as it does after ``zero_grad(set_to_none=True)``
    (no weight decay on a parameter the loss never reaches).  Between calls the gradients must keep aliasing the flat
    buffer: no ``zero_grad(set_to_none=True)`` by the caller.  Integer buffers (``num_batches_tracked``) advance
    alike on every rank and are not sent.  ``nn.SyncBatchNorm`` is refused: its collectives sit inside the forward.

    With ``process_group=None`` none of this exists: one graph, ``zero_grad(set_to_none=True)`` inside it, whether
    or not torch.distributed is initialised.

    With a ``si_mamba_amd.optim.AdamW`` as ``optimizer`` the clip and the update are its three launches:
    ``optimizer.step(clip=clip)`` in the single graph, ``optimizer.step(clip=clip, grad_scale=1 / world)`` as graph B
    (the same arithmetic: scale by 1 / world, norm, scale by the clipped coefficient), and ``self.grad_norm`` is the
    optimizer's.  One difference: ``.grad`` (the flat buffer) holds the raw gradients afterwards, not the clipped
    mean.  A schedule attached with ``set_schedule`` changes the learning rate under the replays with no recapture.
    With any other optimizer nothing changes.
    """

    def __init__(self, loss_fn, optimizer, example_inputs, params=None, clip=None, warmup: int = 3, *,
                 process_group=None, module=None, broadcast_buffers: bool = True):
        if module is not None:
            if process_group is None:
                raise ValueError("GraphedTrainStep: module= only serves the data-parallel step (process_group=)")
            if any(isinstance(m, torch.nn.SyncBatchNorm) for m in module.modules()):
                raise RuntimeError("GraphedTrainStep: the module contains nn.SyncBatchNorm, whose collectives run "
                                   "inside the forward and cannot be captured into a graph; keep plain BatchNorm "
                                   "(per-rank statistics) or the eager step")
        if process_group is not None and not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("GraphedTrainStep: process_group given but torch.distributed is not initialised "
                               "(call si_mamba_amd.dist.init_dist() first)")
        if not all(t.is_cuda for t in example_inputs):
            raise RuntimeError("GraphedTrainStep needs CUDA/ROCm tensors")
        self.loss_fn, self.opt, self.clip = loss_fn, optimizer, clip
        self.hip_tail = isinstance(optimizer, _HipAdamW)
        self.params = [p for g in optimizer.param_groups for p in g["params"]] if params is None else list(params)
        self.static_in = [t.clone() for t in example_inputs]
        self.group = process_group
        if process_group is not None:
            self.world = dist.get_world_size(process_group)
            self._sync_state(module)
            floats = [] if module is None else [b for b in module.buffers() if b.is_floating_point()]
            self.sync_buffers = FlatBroadcast(floats, process_group) if floats and broadcast_buffers else None
            self.grad_norm = torch.zeros((), device=self.static_in[0].device) if clip is not None else None
            self.flat = None
        elif self.hip_tail:
            self.grad_norm = None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):               # optimizer state, library handles and autotuned paths settle here
                self._eager()
        torch.cuda.current_stream().wait_stream(side)
        if process_group is not None and self.flat is None:
            raise RuntimeError("GraphedTrainStep: the data-parallel step needs at least one warm-up step, which "
                               "finds the parameters that take a gradient")
        self.recapture()

    def recapture(self):
        """Capture the step again, after a change on the Python side that a graph froze as a constant: BatchNorm
        momentum, drop-path rates, a float learning rate.  (A tensor ``lr`` with a capturable optimizer is read by
        the graph on every replay and needs no recapture, nor does si_mamba_amd.optim.AdamW with a schedule.)"""
        self.graph = self.graph_a = self.graph_b = None        # the old graphs hand their memory pool back first
        torch.cuda.synchronize()
        if self.group is None:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.static_loss = self._eager()
            return
        # thread_local: the process group's watchdog thread polls the events of the collectives issued so far (the
        # warm-up's, the last step's) for some 100 ms after they finished; under the default global capture mode its
        # query counts as an offence against this thread's capture and ends the process
        self.graph_a, self.graph_b = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_a, capture_error_mode="thread_local"):
            self.static_loss = self._backward()
        with torch.cuda.graph(self.graph_b, pool=self.graph_a.pool(), capture_error_mode="thread_local"):
            self._update()

    def _sync_state(self, module):
        src = dist.get_global_rank(self.group, 0)
        with torch.no_grad():
            for t in self.params + ([] if module is None else list(module.buffers())):
                dist.broadcast(t, src, group=self.group)

    def _eager(self):
        if self.group is not None:
            if self.sync_buffers is not None:
                self.sync_buffers()
            loss = self._backward()
            self.flat.all_reduce_(self.group)
            self._update()
            return loss
        self.opt.zero_grad(set_to_none=True)
        loss = self.loss_fn(*self.static_in)
        loss.backward()
        if self.hip_tail:
            self.opt.step(clip=self.clip)
            self.grad_norm = self.opt.grad_norm
            return loss.detach()
        if self.clip is not None:
            torch.nn.utils.clip_grad_norm_(self.params, self.clip, foreach=True)
        self.opt.step()
        return loss.detach()

    def _backward(self):
        """Graph A: this rank's loss and gradients, accumulated into the zeroed flat buffer."""
        if self.flat is None:
            # the first warm-up step runs with every gradient unset and shows which parameters the loss reaches
            self.opt.zero_grad(set_to_none=True)
            for p in self.params:
                p.grad = None
        else:
            self.flat.zero_()
        loss = self.loss_fn(*self.static_in)
        loss.backward()
        if self.flat is None:
            self.flat = FlatGradients(self.params, exclude=[p for p in self.params if p.grad is None])
            if not self.flat.params:
                raise RuntimeError("GraphedTrainStep: the loss reaches none of the parameters")
            self._probe = self.flat.params[0]
            self._probe_ptr = self._probe.grad.data_ptr()
        return loss.detach()

    @torch.no_grad()
    def _update(self):
        """Graph B: mean over the ranks, clip_grad_norm_'s arithmetic on the flat buffer, optimizer step."""
        if self.hip_tail:
            self.opt.step(clip=self.clip, grad_scale=1.0 / self.world)
            self.grad_norm = self.opt.grad_norm
            return
        bufs = self.flat.buffers
        for buf in bufs:
            buf.mul_(1.0 / self.world)
        if self.clip is not None:
            if len(bufs) == 1:
                torch.linalg.vector_norm(bufs[0], dtype=torch.float32, out=self.grad_norm)
            else:
                norms = torch.stack([torch.linalg.vector_norm(buf, dtype=torch.float32) for buf in bufs])
                torch.linalg.vector_norm(norms, out=self.grad_norm)
            coef = torch.clamp(self.clip / (self.grad_norm + 1e-6), max=1.0)
            for buf in bufs:
                buf.mul_(coef)
        self.opt.step()

    def __call__(self, *inputs):
        for dst, src in zip(self.static_in, inputs):
            if src is not dst:
                dst.copy_(src)
        if self.group is None:
            self.graph.replay()
            return self.static_loss
        grad = self._probe.grad
        if grad is None or grad.data_ptr() != self._probe_ptr:
            raise RuntimeError("GraphedTrainStep: the gradients no longer alias the flat buffer the graphs write "
                               "(zero_grad(set_to_none=True) in between?); the step zeroes them itself")
        if self.sync_buffers is not None:
            self.sync_buffers()
        self.graph_a.replay()
        self.flat.all_reduce_(self.group)
        self.graph_b.replay()
        return self.static_loss
