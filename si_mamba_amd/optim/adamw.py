"""The optimizer tail of a training step -- gradient clipping by the global norm, decoupled AdamW, the per-epoch
learning-rate schedule -- as three HIP launches over every parameter tensor at once (csrc/optim.hip,
simamba_optim_adamw_step; exported as ``si_mamba_amd.optim``), with nothing read on the host, so that the whole of it captures into a hipGraph.

    groups = reference_param_groups(model, weight_decay=0.05)          # tools/builder.py:58-72
    opt = AdamW(groups, lr=3e-4, weight_decay=0.05)
    opt.set_schedule(runner_epoch_values(cos_lr_values(3e-4, 300, 10), 300), steps_per_epoch=len(loader))

The reference builds torch.optim.AdamW over the same two groups and timm's CosineLRScheduler, which writes a Python
float into ``param_groups[...]['lr']`` once per epoch (tools/builder.py:74-95, tools/runner_finetune.py:252-256); a
captured graph freezes such a float.  Here the schedule is a table in device memory, indexed on the device by the count
of updates, and the learning rate a graph replays with changes from one replay to the next with no recapture.

The state (``step``, ``exp_avg``, ``exp_avg_sq`` per parameter, torch's meaning) and the group options are
torch.optim.AdamW's: a ``state_dict()`` of either loads into the other.  Each group of the dict also carries
``updates``, the count of ``step()`` calls, so that a resumed run continues its schedule.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _lib

__all__ = ["AdamW", "cos_lr_values", "runner_epoch_values", "reference_param_groups"]

_SEG_WORDS = 8          # int64 words of a simamba_optim_segment: p, g, exp_avg, exp_avg_sq, n, group, step, reserved
_SEG_HOST_WORDS = 6     # the words the host owns; the step count lives on the device
_STEP_F32 = 12          # the step count's index among the 16 fp32 words of a segment
_GROUP_WORDS = 8        # lr address, then beta1, beta2, eps, weight_decay, lr_scale as fp64, two reserved


# ---- the reference's schedule ----------------------------------------------------------------------------------------
def cos_lr_values(base_lr, epochs, initial_epochs, lr_min=1e-6, warmup_lr_init=1e-6):
    """The ``epochs + 1`` values ``_get_lr(t)``, t = 0 .. epochs, of timm's CosineLRScheduler as the reference builds it
    (tools/builder.py:87-95: t_initial=epochs, warmup_t=initial_epochs, cycle_limit=1, cycle_mul=1, cycle_decay=0.1, no
    warm-up prefix), in float64: linear from ``warmup_lr_init`` below ``initial_epochs``, the half cosine
    ``lr_min + 0.5 (base_lr - lr_min)(1 + cos(pi t / epochs))`` below ``epochs``, ``lr_min`` from there on."""
    epochs, initial_epochs = int(epochs), int(initial_epochs)
    if epochs < 1 or initial_epochs < 0:
        raise ValueError(f"cos_lr_values: epochs >= 1 and initial_epochs >= 0, got {epochs} and {initial_epochs}")
    base_lr, lr_min, warmup_lr_init = float(base_lr), float(lr_min), float(warmup_lr_init)
    out = []
    for t in range(epochs + 1):
        if t < initial_epochs:
            out.append(warmup_lr_init + t * ((base_lr - warmup_lr_init) / initial_epochs))
        elif t < epochs:
            out.append(lr_min + 0.5 * (base_lr - lr_min) * (1.0 + math.cos(math.pi * t / epochs)))
        else:
            out.append(lr_min)
    return out


def runner_epoch_values(values, max_epoch):
    """What epoch ``e`` of the reference's loop trains at, e = 0 .. max_epoch: ``values[max(e - 1, 0)]``.  timm's
    constructor sets ``_get_lr(0)`` and the runner calls ``scheduler.step(epoch)`` AFTER epoch ``epoch``
    (tools/runner_finetune.py:148, 252-256), so epochs 0 and 1 both run at ``values[0]`` and epoch e > 0 at
    ``values[e - 1]``."""
    values = [float(v) for v in values]
    if not values:
        raise ValueError("runner_epoch_values: an empty schedule")
    return [values[min(max(e - 1, 0), len(values) - 1)] for e in range(int(max_epoch) + 1)]


def reference_param_groups(model, weight_decay, skip_list=()):
    """The reference's two parameter groups (tools/builder.py:58-72), ``[no decay, decay]``: a frozen parameter is left
    out; a parameter takes no weight decay when it is 1-D, or its name ends in ``.bias``, or its name contains
    ``token``, or its name is in ``skip_list``; every other parameter takes ``weight_decay``."""
    skip = set(skip_list)
    decay, no_decay = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if p.dim() == 1 or name.endswith(".bias") or "token" in name or name in skip:
            no_decay.append(p)
        else:
            decay.append(p)
    return [{"params": no_decay, "weight_decay": 0.0}, {"params": decay, "weight_decay": float(weight_decay)}]


# ---- the optimizer ---------------------------------------------------------------------------------------------------
def _torch_defaults():
    """torch.optim.AdamW's own group options (their names differ between torch versions), so that a state dict of this
    optimizer carries exactly the keys torch's does."""
    return dict(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).defaults)


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class AdamW(torch.optim.Optimizer):
    """Decoupled AdamW with the clip and the schedule inside ``step``: three launches whatever the number of tensors.

    ``step(clip=None, grad_scale=1.0, zero_grads=False)``: g' = grad_scale * coef * g with coef = min(1, clip /
    (grad_norm + 1e-6)) (NaN propagating, as torch.clamp) and ``self.grad_norm`` the device scalar |grad_scale * g|
    before clipping; then torch.optim.AdamW's update.  ``.grad`` is only read -- it holds the RAW gradients afterwards,
    not the clipped ones clip_grad_norm_ leaves -- or, with ``zero_grads``, zeroed in the same pass.  A parameter
    without a gradient is neither decayed nor stepped.  ``group['lr']`` is a float or a 0-dim device tensor; an eager
    ``step()`` copies changed floats to the device, so a host scheduler works outside graphs; ``set_schedule`` attaches
    a device table instead, after which the floats are not read and ``device_lr()`` holds the rates in use.

    The kernels read a table of addresses kept in device memory.  ``step()`` compares the ``data_ptr()`` of every
    parameter and state tensor on the host first and rewrites the table in place when one changed; inside a graph
    capture a change raises, so that a stale address never reaches a kernel.  The first ``step()`` (it allocates the
    state) must therefore run eagerly, or ``prepare()`` in its place.  The gradient addresses travel with every call
    instead (the first launch carries them as arguments and writes them into the table), so gradients may be fresh
    tensors every step, as after ``zero_grad(set_to_none=True)``, inside a capture too: a replay restores the
    addresses its capture saw.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, amsgrad=False,
                 maximize=False):
        if amsgrad:
            raise ValueError("si_mamba_amd.optim.AdamW: amsgrad is not supported")
        if maximize:
            raise ValueError("si_mamba_amd.optim.AdamW: maximize is not supported")
        defaults = _torch_defaults()
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        capturable=True, foreach=None, fused=None, differentiable=False)
        self._reset_tables()
        self._schedule = None
        self._steps_per_epoch = 1
        self._lr_scale = None
        self._pending_updates = 0
        self.grad_norm = None
        super().__init__(params, defaults)

    def _reset_tables(self):
        self._key = None              # what the device segment table was built from
        self._group_key = None        # what the device group table was built from
        self._sizes = None            # the element counts the chunk table was built from
        self._seg = self._seg_f32 = self._chunks = self._groups = self._lr_dev = self._updates = self._ws = None
        self._first_chunk = self._grad_ptrs = None

    # ---- construction-time checks --------------------------------------------------------------------------------
    @staticmethod
    def _check_group(group):
        if group.get("amsgrad"):
            raise ValueError("si_mamba_amd.optim.AdamW: amsgrad is not supported")
        if group.get("maximize"):
            raise ValueError("si_mamba_amd.optim.AdamW: maximize is not supported")
        if group.get("differentiable"):
            raise ValueError("si_mamba_amd.optim.AdamW: differentiable is not supported")
        if group.get("decoupled_weight_decay", True) is False:
            raise ValueError("si_mamba_amd.optim.AdamW: coupled weight decay (Adam) is not supported")
        lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
        if isinstance(lr, torch.Tensor):
            if lr.numel() != 1 or lr.dtype != torch.float32:
                raise ValueError("si_mamba_amd.optim.AdamW: a tensor lr is one float32 element")
        elif not (float(lr) >= 0.0):
            raise ValueError(f"si_mamba_amd.optim.AdamW: invalid learning rate {lr}")
        if not (0.0 <= float(b1) < 1.0 and 0.0 <= float(b2) < 1.0):
            raise ValueError(f"si_mamba_amd.optim.AdamW: invalid betas {(b1, b2)}")
        if not (float(eps) >= 0.0) or not (float(wd) >= 0.0):
            raise ValueError(f"si_mamba_amd.optim.AdamW: invalid eps {eps} or weight_decay {wd}")

    @staticmethod
    def _check_tensor(t, what):
        if t.is_sparse or t.layout is not torch.strided:
            raise ValueError(f"si_mamba_amd.optim.AdamW: sparse {what}s are not supported")
        if t.dtype != torch.float32:
            raise ValueError(f"si_mamba_amd.optim.AdamW: {what}s are float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"si_mamba_amd.optim.AdamW: a non-contiguous {what} is not supported")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])
        devices = set()
        for g in self.param_groups:
            for p in g["params"]:
                self._check_tensor(p, "parameter")
                devices.add(p.device)
        if len(devices) > 1:
            raise ValueError("si_mamba_amd.optim.AdamW: parameters on several devices "
                             f"({', '.join(sorted(map(str, devices)))}); one optimizer serves one device")
        self._key = self._group_key = None

    # ---- the schedule ---------------------------------------------------------------------------------------------
    def _device(self):
        for g in self.param_groups:
            for p in g["params"]:
                _lib.require_gpu(p, "si_mamba_amd.optim.AdamW")
                return p.device
        raise ValueError("si_mamba_amd.optim.AdamW: no parameters")

    def set_schedule(self, values, steps_per_epoch, lr_scale=None):
        """Attach a per-epoch table: update number u (counted from 0, carried by the state dict) runs every group g at
        ``values[min(u // steps_per_epoch, len(values) - 1)] * lr_scale[g]``, computed on the device and written back to
        the group's device learning rate.  Any per-epoch schedule fits: evaluate it on the host once (``cos_lr_values``,
        a LambdaLR's lambda, StepLR's ``gamma ** (e // step_size)``).  ``values=None`` detaches.  A table of the same
        length as the one attached is copied into it in place, so that captured graphs follow; anything else (another
        length, another ``steps_per_epoch``) needs a recapture."""
        if _capturing():
            raise RuntimeError("si_mamba_amd.optim.AdamW.set_schedule inside a graph capture")
        if values is None:
            self._schedule, self._lr_scale, self._group_key = None, None, None
            return
        values = [float(v) for v in values]
        steps_per_epoch = int(steps_per_epoch)
        if not values or len(values) > (1 << 20) or not all(math.isfinite(v) and v >= 0.0 for v in values):
            raise ValueError("si_mamba_amd.optim.AdamW.set_schedule: 1 .. 2^20 finite, non-negative values")
        if not 1 <= steps_per_epoch < 2 ** 31:
            raise ValueError(f"si_mamba_amd.optim.AdamW.set_schedule: steps_per_epoch {steps_per_epoch}")
        scale = [1.0] * len(self.param_groups) if lr_scale is None else [float(s) for s in lr_scale]
        if len(scale) != len(self.param_groups) or not all(math.isfinite(s) for s in scale):
            raise ValueError("si_mamba_amd.optim.AdamW.set_schedule: lr_scale holds one finite factor per group")
        table = torch.tensor(values, dtype=torch.float64)
        device = self._device()
        if self._schedule is not None and self._schedule.numel() == table.numel():
            self._schedule.copy_(table)
        else:
            self._schedule = table.to(device)
        self._steps_per_epoch, self._lr_scale, self._group_key = steps_per_epoch, scale, None

    def device_lr(self):
        """(groups) fp32 on the device: the learning rate each group's last update ran at (a copy)."""
        if self._lr_dev is None:
            raise RuntimeError("si_mamba_amd.optim.AdamW.device_lr before the first step()")
        return torch.stack([g["lr"].reshape(()) if isinstance(g["lr"], torch.Tensor) else self._lr_dev[i]
                            for i, g in enumerate(self.param_groups)])

    # ---- table upkeep ---------------------------------------------------------------------------------------------
    def _stale(self, what):
        raise RuntimeError(f"si_mamba_amd.optim.AdamW.step inside a graph capture: {what} since the last eager step(); "
                           "the device tables would be stale.  Run one eager step() first, then capture")

    def _sync(self):
        """Bring the device tables up to the Python side; returns (device, segments, chunks) or None when there is
        nothing to update.  Host work only, unless something changed."""
        params = [p for g in self.param_groups for p in g["params"]]
        if not params:
            return None
        for p in params:
            _lib.require_gpu(p, "si_mamba_amd.optim.AdamW.step")
        device = params[0].device
        capturing = _capturing()
        nseg = len(params)
        if nseg > _lib.OPTIM_MAX_SEGMENTS or len(self.param_groups) > _lib.OPTIM_MAX_GROUPS:
            raise ValueError(f"si_mamba_amd.optim.AdamW: at most {_lib.OPTIM_MAX_SEGMENTS} parameter tensors in "
                             f"{_lib.OPTIM_MAX_GROUPS} groups")
        sizes = tuple(p.numel() for p in params)
        if sizes != self._sizes:
            if capturing:
                self._stale("the parameter set changed")
            self._build_chunks(sizes, device)
        key, gi = [], 0
        for gidx, group in enumerate(self.param_groups):
            self._check_group(group)
            for p in group["params"]:
                i, gi = gi, gi + 1
                self._check_tensor(p, "parameter")
                if p.device != device:
                    raise ValueError("si_mamba_amd.optim.AdamW: parameters on several devices")
                grad = p.grad
                state = self.state.get(p)
                if grad is not None:
                    self._check_tensor(grad, "gradient")
                    _lib.require_gpu(grad, "si_mamba_amd.optim.AdamW.step")
                    if grad.device != device or grad.numel() != p.numel():
                        raise ValueError("si_mamba_amd.optim.AdamW: a gradient of another device or size")
                    if not state:
                        if capturing:
                            self._stale("a parameter took its first gradient")
                        state = self.state[p]
                        state["step"] = self._seg_f32[i, _STEP_F32]          # zero: no update has touched the slot
                        state["exp_avg"] = torch.empty_like(p, memory_format=torch.contiguous_format).zero_()
                        state["exp_avg_sq"] = torch.empty_like(p, memory_format=torch.contiguous_format).zero_()
                m = v = 0
                if state:
                    self._adopt_state(state, i, p, capturing)
                    m, v = state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr()
                self._grad_ptrs[i] = 0 if grad is None else grad.data_ptr()
                key.append((p.data_ptr(), 0, m, v, p.numel(), gidx))        # word 1, g, is the kernels' to write
        if key != self._key:
            if capturing:
                self._stale("an address of a parameter or state tensor changed")
            host = torch.tensor(key, dtype=torch.int64).reshape(nseg, _SEG_HOST_WORDS)
            self._seg[:, :_SEG_HOST_WORDS].copy_(host)
            self._key = key
        self._sync_groups(device, capturing)
        if self._pending_updates is not None:
            if capturing:
                self._stale("a state dict was loaded")
            self._updates.fill_(int(self._pending_updates))
            self._pending_updates = None
        return device, nseg, self._chunks.shape[0]

    def _build_chunks(self, sizes, device):
        """Tables for another set of tensors.  The step counts move over through ``_adopt_state``: the state still holds
        views of the old table."""
        counts = np.array([-(-n // _lib.OPTIM_CHUNK) for n in sizes], dtype=np.int64)
        total = int(counts.sum())
        if total > _lib.OPTIM_MAX_CHUNKS:
            raise ValueError(f"si_mamba_amd.optim.AdamW: {sum(sizes)} elements; at most "
                             f"{_lib.OPTIM_MAX_CHUNKS * _lib.OPTIM_CHUNK}")
        seg = np.repeat(np.arange(len(sizes), dtype=np.int64), counts)
        first = np.repeat(np.cumsum(counts) - counts, counts)
        table = np.stack([seg, np.arange(total, dtype=np.int64) - first], axis=1).astype(np.int32)
        ngroups = len(self.param_groups)
        updates = self._pending_updates
        if updates is None and self._updates is not None:
            updates = int(self._updates.item())
        self._pending_updates = updates or 0
        self._seg = torch.zeros(len(sizes), _SEG_WORDS, dtype=torch.int64, device=device)
        self._seg_f32 = self._seg.view(torch.float32)
        self._chunks = torch.from_numpy(table).to(device)
        self._first_chunk = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)      # host arrays of the call
        self._grad_ptrs = np.zeros(len(sizes), dtype=np.int64)
        self._groups = torch.zeros(ngroups, _GROUP_WORDS, dtype=torch.int64, device=device)
        self._lr_dev = torch.zeros(ngroups, dtype=torch.float32, device=device)
        self._updates = torch.zeros(1, dtype=torch.int64, device=device)
        if self.grad_norm is None or self.grad_norm.device != device:
            self.grad_norm = torch.zeros((), dtype=torch.float32, device=device)
        nbytes = _lib.load().simamba_optim_workspace_bytes(len(sizes), max(total, 1))
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self._sizes, self._key, self._group_key = sizes, None, None

    def _adopt_state(self, state, i, p, capturing):
        """The state of segment i as the kernels need it: the step count inside the table, fp32 contiguous moments on
        the parameter's device.  A state that came from a state dict (or from an older table) is copied over once."""
        mine = self._seg_f32[i, _STEP_F32]
        step = state.get("step")
        if not (isinstance(step, torch.Tensor) and step.device == mine.device and step.dtype == torch.float32
                and step.data_ptr() == mine.data_ptr()):
            if capturing:
                self._stale("a state dict was loaded")
            if isinstance(step, torch.Tensor):
                mine.copy_(step.detach().reshape(()))
            else:
                mine.fill_(float(step or 0.0))
            state["step"] = mine
        for k in ("exp_avg", "exp_avg_sq"):
            t = state.get(k)
            if t is None:
                raise ValueError(f"si_mamba_amd.optim.AdamW: a parameter's state has no {k}")
            if t.device != p.device or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
                if capturing:
                    self._stale("a state dict was loaded")
                state[k] = t.detach().to(device=p.device, dtype=torch.float32).contiguous().view_as(p)

    def _sync_groups(self, device, capturing):
        key, floats = [], []
        for i, g in enumerate(self.param_groups):
            lr = g["lr"]
            if isinstance(lr, torch.Tensor):
                _lib.require_gpu(lr, "si_mamba_amd.optim.AdamW.step (lr)")
                if lr.device != device:
                    raise ValueError("si_mamba_amd.optim.AdamW: a tensor lr on another device")
                ptr, lr_host = lr.data_ptr(), None
            else:
                ptr = self._lr_dev.data_ptr() + 4 * i
                lr_host = None if self._schedule is not None else float(lr)
            scale = 1.0 if self._lr_scale is None else self._lr_scale[i]
            key.append((ptr, float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                        scale))
            floats.append(lr_host)
        sched = None if self._schedule is None else (self._schedule.data_ptr(), self._steps_per_epoch)
        if (key, floats, sched) == self._group_key:
            return
        if capturing:
            self._stale("a group option, a float learning rate or the schedule changed")
        old = self._group_key
        if old is None or old[0] != key:
            host = np.zeros((len(key), _GROUP_WORDS), dtype=np.int64)
            host[:, 0] = [k[0] for k in key]
            host[:, 1:6].view(np.float64)[:] = [k[1:] for k in key]
            self._groups.copy_(torch.from_numpy(host))
        if any(f is not None for f in floats) and (old is None or old[1] != floats):
            # one copy of the float rates; the slots of tensor-lr and scheduled groups are not read by the kernels
            self._lr_dev.copy_(torch.tensor([0.0 if f is None else f for f in floats], dtype=torch.float32))
        self._group_key = (key, floats, sched)

    # ---- the step -------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prepare(self):
        """Everything ``step()`` does in front of its launches, and no launch: allocate the state of every parameter
        that holds a gradient and bring the device tables up to date.  In front of a capture whose first ``step()``
        would otherwise be the optimizer's first (a warm-up step serves as well)."""
        self._sync()

    @torch.no_grad()
    def step(self, closure=None, *, clip=None, grad_scale=1.0, zero_grads=False):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        max_norm = -1.0 if clip is None else float(clip)
        if clip is not None and not (max_norm >= 0.0):
            raise ValueError(f"si_mamba_amd.optim.AdamW.step: clip {clip}")
        grad_scale = float(grad_scale)
        if not math.isfinite(grad_scale):
            raise ValueError(f"si_mamba_amd.optim.AdamW.step: grad_scale {grad_scale}")
        synced = self._sync()
        if synced is None:
            return loss
        device, nseg, nchunks = synced
        if nchunks == 0:
            return loss
        sched_n = 0 if self._schedule is None else self._schedule.numel()
        _lib.call("simamba_optim_adamw_step", self._seg, self._chunks, self._groups, self._updates, self._schedule,
                  self.grad_norm, self._grad_ptrs.ctypes.data, self._first_chunk.ctypes.data, self._ws,
                  self._ws.numel(), nseg, nchunks, len(self.param_groups), sched_n,
                  self._steps_per_epoch, max_norm, grad_scale, _lib.OPTIM_ZERO_GRADS if zero_grads else 0,
                  device=device)
        return loss

    # ---- state dicts ----------------------------------------------------------------------------------------------
    def update_count(self):
        """The count of ``step()`` calls so far (a host read)."""
        if self._pending_updates is not None:
            return int(self._pending_updates)
        return int(self._updates.item()) if self._updates is not None else 0

    def state_dict(self):
        """torch.optim.AdamW's layout; every group also carries ``updates``.  The step counts are copies (one tensor,
        viewed per parameter), not views of the device table."""
        out = super().state_dict()
        n = self.update_count()
        for g in out["param_groups"]:
            g["updates"] = n
        if self._seg_f32 is None:
            return out
        steps = self._seg_f32[:, _STEP_F32].clone()
        state = {}
        for pid, st in out["state"].items():
            st = dict(st)
            step = st.get("step")
            if isinstance(pid, int) and pid < steps.numel() and isinstance(step, torch.Tensor) and step.is_cuda \
                    and step.data_ptr() == self._seg_f32[pid, _STEP_F32].data_ptr():
                st["step"] = steps[pid]
            state[pid] = st
        out["state"] = state
        return out

    def load_state_dict(self, state_dict):
        updates = None
        for g in state_dict["param_groups"]:
            if "updates" in g:
                updates = int(g["updates"])
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            g.pop("updates", None)
            self._check_group(g)
            g["capturable"] = True
        if updates is None:                        # a checkpoint of torch.optim.AdamW: every parameter stepped each time
            steps = [float(st["step"]) for st in self.state.values() if "step" in st]
            updates = int(max(steps)) if steps else 0
        self._pending_updates = updates
        self._key = self._group_key = None
