"""Point-cloud sampling and augmentation on the device (csrc/augment.hip): the reference's
``datasets/data_transforms.py`` classes and the runners' ``fps_idx[:, choice]`` + ``gather_operation``
(tools/runner_finetune.py:191-194), as one launch per batch with no host read.

The seven classes carry the reference's names, constructor arguments and defaults; ``pc = T(pc)`` works in place on a
``(B, N, 3)`` float32 device tensor and returns it, as the reference's do.  ``Compose([...])`` lowers a run of them to
one launch; ``sample_and_augment`` adds the gather and the subset in front of the chain, in the same launch.

Random numbers are counter based (Philox4x32-10; the layout is in include/simamba.h): an ``AugmentState`` is a device
tensor ``[seed, step]`` that the kernel reads and a one-lane kernel advances, so a call inside a captured graph draws
fresh values at every replay.  The reference's numpy / ``random`` streams cannot be reproduced on a device and are not:
the distributions are the reference's, the draws are not.

Not built: ``RandomHorizontalFlip(is_temporal=True)`` (4-D coordinates), clouds above 8192 points, extra channels such
as normals (the kernel takes ``(B, N, 3)`` only).  There is no CPU route and nothing here is differentiable: inputs on
the CPU or with ``requires_grad`` are refused.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib

__all__ = ["PointcloudRotate", "PointcloudScaleAndTranslate", "PointcloudJitter", "PointcloudScale",
           "PointcloudTranslate", "PointcloudRandomInputDropout", "RandomHorizontalFlip", "Compose", "AugmentState",
           "default_state", "sample_and_augment", "augment_params"]

_MASK64 = (1 << 64) - 1


def _as_i64(v):
    """A 64-bit pattern as the int64 torch stores."""
    v = int(v) & _MASK64
    return v - (1 << 64) if v >= 1 << 63 else v


class AugmentState:
    """``[seed, step]`` on ``device``: the key and the call counter of the augmentation kernels.  Every fused launch
    reads both and adds 1 to ``step`` on the device, in stream order.  ``.seed`` and ``.step`` copy to the host (a
    synchronisation: for tests and logging, not for the training loop); constructing and ``manual_seed`` copy from the
    host, so do both outside a graph capture."""

    def __init__(self, seed=0, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"AugmentState: device is {device}; si_mamba_amd runs on a ROCm device only "
                               "(no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.tensor = torch.tensor([_as_i64(seed), 0], dtype=torch.int64, device=device)

    @property
    def device(self):
        return self.tensor.device

    @property
    def seed(self):
        return int(self.tensor[0].item()) & _MASK64

    @property
    def step(self):
        return int(self.tensor[1].item()) & _MASK64

    def manual_seed(self, seed, step=0):
        """Set the seed and put the step back to ``step``."""
        self.tensor.copy_(torch.tensor([_as_i64(seed), _as_i64(step)], dtype=torch.int64))
        return self


_default_states = {}


def default_state(device):
    """The state the transforms use when none is given: one per device, created on first use from
    ``torch.initial_seed()`` (so ``torch.manual_seed`` ahead of the first call fixes it)."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    st = _default_states.get(device)
    if st is None:
        st = _default_states[device] = AugmentState(torch.initial_seed(), device)
    return st


class _Fused:
    """A transform the kernel applies: ``op()`` is its opcode and up to four fp32 parameters."""

    def op(self):
        raise NotImplementedError

    def __call__(self, pc, state=None):
        return sample_and_augment(pc, [self], state=state, out=pc)

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in vars(self).items())})"


class PointcloudRotate(_Fused):
    """A rotation about the y axis by ``u * 2 pi``, one angle per cloud (data_transforms.py:6-18)."""

    def op(self):
        return _lib.AUG_ROTATE, ()


class PointcloudScaleAndTranslate(_Fused):
    """Per cloud and axis ``p * s + t``, ``s ~ U[scale_low, scale_high)``, ``t ~ U[-translate_range, translate_range)``
    (data_transforms.py:21-36)."""

    def __init__(self, scale_low=2. / 3., scale_high=3. / 2., translate_range=0.2):
        self.scale_low, self.scale_high, self.translate_range = scale_low, scale_high, translate_range

    def op(self):
        return _lib.AUG_SCALE_TRANSLATE, (self.scale_low, self.scale_high, self.translate_range)


class PointcloudJitter(_Fused):
    """Per coordinate ``+ clamp(std * n, -clip, clip)``, ``n`` standard normal (data_transforms.py:39-51)."""

    def __init__(self, std=0.01, clip=0.05):
        self.std, self.clip = std, clip

    def op(self):
        return _lib.AUG_JITTER, (self.std, self.clip)


class PointcloudScale(_Fused):
    """Per cloud and axis ``p * s``, ``s ~ U[scale_low, scale_high)`` (data_transforms.py:54-66)."""

    def __init__(self, scale_low=2. / 3., scale_high=3. / 2.):
        self.scale_low, self.scale_high = scale_low, scale_high

    def op(self):
        return _lib.AUG_SCALE, (self.scale_low, self.scale_high)


class PointcloudTranslate(_Fused):
    """Per cloud and axis ``p + t``, ``t ~ U[-translate_range, translate_range)`` (data_transforms.py:69-80)."""

    def __init__(self, translate_range=0.2):
        self.translate_range = translate_range

    def op(self):
        return _lib.AUG_TRANSLATE, (self.translate_range,)


class PointcloudRandomInputDropout(_Fused):
    """Per cloud ``ratio = u * max_dropout_ratio``; every point with ``u_i <= ratio`` becomes the cloud's first point
    (data_transforms.py:83-98)."""

    def __init__(self, max_dropout_ratio=0.5):
        assert max_dropout_ratio >= 0 and max_dropout_ratio < 1
        self.max_dropout_ratio = max_dropout_ratio

    def op(self):
        return _lib.AUG_DROPOUT, (self.max_dropout_ratio,)


class RandomHorizontalFlip(_Fused):
    """With probability 0.95 per cloud, each horizontal axis is mirrored with probability 0.5: ``c' = max(c) - c``
    (data_transforms.py:101-121).  ``is_temporal`` (a fourth coordinate) is not built."""

    def __init__(self, upright_axis='z', is_temporal=False):
        if is_temporal:
            raise NotImplementedError("RandomHorizontalFlip: is_temporal=True (4-D coordinates) is not built")
        self.is_temporal = is_temporal
        self.D = 3
        self.upright_axis = {'x': 0, 'y': 1, 'z': 2}[upright_axis.lower()]
        self.horz_axes = set(range(self.D)) - set([self.upright_axis])

    def op(self):
        return _lib.AUG_FLIP, (float(self.upright_axis),)


def _chain_arrays(transforms, what):
    """(ops, op_params, n) as the host arrays the C ABI reads, from a sequence of fused transforms."""
    chain = list(transforms)
    for t in chain:
        if not isinstance(t, _Fused):
            raise TypeError(f"{what}: {t!r} is not one of this module's transforms (Compose runs foreign callables "
                            "between fused launches)")
    if len(chain) > _lib.AUG_MAX_OPS:
        raise ValueError(f"{what}: {len(chain)} transforms, one launch takes at most {_lib.AUG_MAX_OPS} "
                         "(Compose splits longer chains)")
    ops = (ctypes.c_int * max(len(chain), 1))()
    params = (ctypes.c_float * (4 * max(len(chain), 1)))()
    for o, t in enumerate(chain):
        code, p = t.op()
        ops[o] = code
        for k, v in enumerate(p):
            params[4 * o + k] = float(v)
    return ops, params, len(chain)


def _flatten(transforms):
    if isinstance(transforms, Compose):
        return list(transforms.transforms)
    if isinstance(transforms, _Fused):
        return [transforms]
    return list(transforms or ())


def _check_points(points, what):
    if not torch.is_tensor(points) or points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError(f"{what}: points must be a (B, N, 3) tensor, got "
                         f"{tuple(points.shape) if torch.is_tensor(points) else type(points).__name__}")
    _lib.require_gpu(points, what)
    if points.requires_grad:
        raise RuntimeError(f"{what}: points require grad; augmentation is data preparation and has no backward "
                           "(detach them first)")
    if points.dtype != torch.float32:
        raise TypeError(f"{what}: points must be float32, got {points.dtype}")
    B, N, _ = points.shape
    if B < 1 or N < 1 or N > _lib.AUG_MAX_POINTS:
        raise ValueError(f"{what}: need B >= 1 and 1 <= N <= {_lib.AUG_MAX_POINTS}, got {tuple(points.shape)}")


def _index(t, shape, what, dev, keep32=False):
    if not torch.is_tensor(t) or t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError(f"{what} must be an integer tensor")
    if t.device != dev:
        raise ValueError(f"{what} is on {t.device}, the points are on {dev}")
    if shape is not None and tuple(t.shape) != shape:
        raise ValueError(f"{what} must have shape {shape}, got {tuple(t.shape)}")
    if not (keep32 and t.dtype == torch.int32):
        t = t.to(torch.int64)
    return t.contiguous()


def sample_and_augment(points, transforms=None, idx=None, sel=None, lengths=None, state=None, out=None):
    """``out[b, i] = chain(points[b, idx[b, sel[i]]])`` in one launch.

    ``points`` (B, N, 3) float32 on the device.  ``transforms``: a sequence (or ``Compose``) of at most 8 of this
    module's transforms, applied in order; None or empty: the gather alone.  ``idx`` (B, M) int32 or int64: rows of
    every cloud (the fused ``gather_operation``; e.g. farthest-point-sampling indices).  ``sel`` (K,) integers:
    positions into ``idx``'s columns shared by the batch (the runners' ``fps_idx[:, choice]``), or, without ``idx``,
    rows of ``points``.  ``lengths`` (B,) integers: cloud ``b`` has ``lengths[b]`` output rows (clamped to [1, K]); the
    rows behind are written as 0 and nothing is read for them.  ``state``: an ``AugmentState`` (default: the device's
    ``default_state``); its step advances by 1.  ``out`` (B, K, 3) float32: the result's storage; it may be ``points``
    itself only without ``idx`` and ``sel``.  N, M and K are at most 8192.

    Nothing is read on the host, so the call can be captured in a graph; a replay draws with the state's step at that
    moment.  Returns ``out``."""
    what = "sample_and_augment"
    _check_points(points, what)
    chain = _flatten(transforms)
    ops, params, n_ops = _chain_arrays(chain, what)
    dev = points.device
    B, N, _ = points.shape
    p = points.contiguous()
    M = N
    if idx is not None:
        if idx.dim() != 2 or idx.shape[0] != B:
            raise ValueError(f"{what}: idx must be ({B}, M), got {tuple(idx.shape)}")
        idx = _index(idx, None, f"{what}: idx", dev, keep32=True)
        M = idx.shape[1]
    K = M
    if sel is not None:
        if sel.dim() != 1:
            raise ValueError(f"{what}: sel must be (K,), got {tuple(sel.shape)}")
        sel = _index(sel, None, f"{what}: sel", dev)
        K = sel.shape[0]
    if not (1 <= M <= _lib.AUG_MAX_POINTS and 1 <= K <= _lib.AUG_MAX_POINTS):
        raise ValueError(f"{what}: need 1 <= M, K <= {_lib.AUG_MAX_POINTS}, got M = {M}, K = {K}")
    if lengths is not None:
        lengths = _index(lengths, (B,), f"{what}: lengths", dev)
    if state is None:
        state = default_state(dev)
    elif not isinstance(state, AugmentState):
        raise TypeError(f"{what}: state must be an AugmentState, got {type(state).__name__}")
    if state.device != dev:
        raise ValueError(f"{what}: the state is on {state.device}, the points are on {dev}")
    if out is None:
        out = torch.empty(B, K, 3, device=dev, dtype=torch.float32)
    elif out is not points:
        if tuple(out.shape) != (B, K, 3) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise ValueError(f"{what}: out must be a contiguous ({B}, {K}, 3) float32 tensor on {dev}")
        if out.requires_grad:
            raise RuntimeError(f"{what}: out requires grad")
    if (out is points or out.data_ptr() == points.data_ptr()) and (idx is not None or sel is not None):
        raise ValueError(f"{what}: out may be the input only without idx and sel")
    target = p if out is points else out                         # a non-contiguous in-place input: through its copy
    _lib.count("augment_points")
    _lib.call("simamba_augment_points", p, idx, int(idx is not None and idx.dtype == torch.int64), sel, lengths, target,
              ops, params, n_ops, state.tensor, B, N, M, K, device=dev, time_as="augment_points")
    if target is not out:
        out.copy_(target)
    return out


def launch_corrupt(points, lengths, out, out_lengths, src, state, kind, flags, params):
    """The launch of ``corruptions.corrupt`` on checked arguments (csrc/corrupt.hip reads and advances the same
    ``AugmentState`` as the call above, so the two launches live side by side): ``points`` (B, N, 3) and ``out``
    (B, K, 3) contiguous float32, ``lengths`` (B,) int64 or None, ``out_lengths`` (B,) int64, ``src`` (B, K) int32 or
    None, ``kind`` / ``flags`` the ABI's integers, ``params`` its host array of four floats."""
    B, N, _ = points.shape
    _lib.count("corrupt_points")
    _lib.call("simamba_corrupt_points", points, lengths, out, out_lengths, src, state.tensor, kind, flags, params, B, N,
              out.shape[1], device=points.device, time_as="corrupt_points")


def augment_params(transforms, B, K, state=None, lengths=None, noise=False, keep=False, device=None):
    """What the next ``sample_and_augment`` with this chain and state will draw, without touching points or the step:
    ``(cloud_params (B, n_ops, 8) float32, noise (B, K, 3) float32 | None, keep (B, K) bool | None)``; the layout of
    ``cloud_params`` per op is that of ``simamba_augment_params`` (include/simamba.h).  For tests and logging."""
    what = "augment_params"
    chain = _flatten(transforms)
    ops, params, n_ops = _chain_arrays(chain, what)
    if state is None:
        state = default_state(device if device is not None else "cuda")
    dev = state.device
    if lengths is not None:
        lengths = _index(lengths, (B,), f"{what}: lengths", dev)
    cloud = torch.zeros(B, max(n_ops, 1), _lib.AUG_CLOUD_PARAMS, device=dev, dtype=torch.float32)
    nz = torch.empty(B, K, 3, device=dev, dtype=torch.float32) if noise else None
    kp = torch.empty(B, K, device=dev, dtype=torch.uint8) if keep else None
    _lib.call("simamba_augment_params", lengths, ops, params, n_ops, state.tensor, cloud, nz, kp, B, K, device=dev)
    return cloud[:, :n_ops], nz, (None if kp is None else kp.bool())


class Compose:
    """``Compose([t1, t2, ...])(pc)``: the transforms in order, in place.  Every run of this module's transforms is
    one launch (runs longer than 8 are split); anything else callable is run eagerly between the launches, as
    ``pc = t(pc)``, and has to return a (B, N, 3) float32 device tensor."""

    def __init__(self, transforms):
        self.transforms = list(transforms)
        for t in self.transforms:
            if not callable(t):
                raise TypeError(f"Compose: {t!r} is not callable")

    def runs(self):
        """The schedule: lists of fused transforms (one launch each) and foreign callables, in order."""
        out, run = [], []
        for t in self.transforms:
            if isinstance(t, _Fused) and len(run) < _lib.AUG_MAX_OPS:
                run.append(t)
                continue
            if run:
                out.append(run)
            run = [t] if isinstance(t, _Fused) else []
            if not isinstance(t, _Fused):
                out.append(t)
        if run:
            out.append(run)
        return out

    def __call__(self, pc, state=None):
        cur = pc
        for item in self.runs():
            cur = sample_and_augment(cur, item, state=state, out=cur) if isinstance(item, list) else item(cur)
        if cur is not pc:
            pc.copy_(cur)
        return pc

    def __repr__(self):
        return f"Compose({self.transforms!r})"
