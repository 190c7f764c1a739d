"""Poisoned, guard-banded replacements of torch.empty / empty_like / empty_strided for the memory-contract tests
(test_guarded_alloc.py, test_gpu_memory_contract.py).  A helper module: pytest collects nothing from it.

``with guarded(poison) as g:`` -- every tensor the listed device types get from torch.empty, torch.empty_like or
torch.empty_strided inside the block lives in the middle of a raw uint8 buffer of ``GUARD + body + GUARD`` bytes that is
filled, guards and body, with the poison written in the tensor's own element type.  ``g.verify()`` asserts that both
guards (and the padding that rounds the body up to ``ALIGN``) still hold the poison bit for bit.  What a call leaves
unwritten therefore holds the poison, and a dependence on it -- or on what lies around an input that went through
``place`` -- shows as a difference between two runs under two poisons.  All poisons are finite: an iterative kernel that
reads one still terminates, and an index read from one (0 or 1) stays inside any non-empty array.

Nothing here provokes a fault: every byte the harness can see change belongs to a buffer this process allocated.
"""
from __future__ import annotations

import os
import sys

import torch

GUARD = 4096          # bytes in front of and behind every body
ALIGN = 512           # the body is rounded up to this, so data_ptr() is as aligned as the caching allocator's blocks

_HERE = os.path.abspath(__file__)
_PKG = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "si_mamba_amd") + os.sep


class Poison:
    """What unwritten memory holds: ``f`` in floating-point buffers, ``i`` in integer, uint8 and bool ones."""

    def __init__(self, name, f, i):
        self.name, self.f, self.i = name, float(f), int(i)

    def value(self, dtype):
        if dtype.is_floating_point or dtype.is_complex:
            if dtype == torch.float16 and abs(self.f) > 60000.0:
                return 49152.0
            return self.f
        if dtype == torch.bool:
            return bool(self.i)
        return self.i

    def __repr__(self):
        return f"Poison({self.name})"


ZERO = Poison("zero", 0.0, 0)
SENTINEL = Poison("sentinel", -12288.0, 1)       # test_gpu_add_norm_slots.py's sentinel; exact in bf16
LARGE = Poison("large", 2.0 ** 100, 1)           # rows marked bitwise=False only

_active = []          # the guarded contexts entered and not yet left, innermost last


class _Record:
    __slots__ = ("raw", "offset", "nbytes", "body", "shape", "dtype", "site", "modules")

    def describe(self):
        return f"torch.empty at {self.site}: shape {tuple(self.shape)}, {self.dtype}"


def _fill(raw, dtype, value):
    raw.view(dtype).fill_(value)


class guarded:
    def __init__(self, poison, devices=("cuda",)):
        self.poison = poison
        self.devices = tuple(devices)
        self.records = []
        self.modules = set()          # si_mamba_amd/*.py files with a frame on the stack of a guarded allocation
        self._saved = None
        self._expected = {}

    # ---- context ---------------------------------------------------------------------------------------------------
    def __enter__(self):
        self._saved = (torch.empty, torch.empty_like, torch.empty_strided)
        real_empty, real_like, real_strided = self._saved
        ctx = self

        def empty(*args, **kw):
            if kw.get("out") is not None or kw.get("layout", torch.strided) is not torch.strided:
                return real_empty(*args, **kw)
            dev = ctx._device(kw.get("device"))
            if dev.type not in ctx.devices:
                return real_empty(*args, **kw)
            meta = real_empty(*args, **dict(kw, device="meta", pin_memory=False, requires_grad=False))
            return ctx._make(meta, dev, kw.get("requires_grad", False))

        def empty_like(inp, **kw):
            if kw.get("layout", torch.strided) is not torch.strided or inp.layout is not torch.strided:
                return real_like(inp, **kw)
            dev = ctx._device(kw["device"]) if kw.get("device") is not None else inp.device
            if dev.type not in ctx.devices:
                return real_like(inp, **kw)
            meta = real_like(inp, **dict(kw, device="meta", pin_memory=False, requires_grad=False))
            return ctx._make(meta, dev, kw.get("requires_grad", False))

        def empty_strided(size, stride, **kw):
            if kw.get("layout", torch.strided) is not torch.strided:
                return real_strided(size, stride, **kw)
            dev = ctx._device(kw.get("device"))
            if dev.type not in ctx.devices:
                return real_strided(size, stride, **kw)
            meta = real_strided(size, stride, **dict(kw, device="meta", pin_memory=False, requires_grad=False))
            return ctx._make(meta, dev, kw.get("requires_grad", False))

        torch.empty, torch.empty_like, torch.empty_strided = empty, empty_like, empty_strided
        _active.append(self)
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like, torch.empty_strided = self._saved
        if self in _active:
            _active.remove(self)
        return False

    # ---- allocation ------------------------------------------------------------------------------------------------
    @staticmethod
    def _device(device):
        if device is None:
            get = getattr(torch, "get_default_device", None)
            return get() if get is not None else torch.device("cpu")
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        return dev

    def _make(self, meta, dev, requires_grad):
        """The guarded tensor with ``meta``'s size, strides and dtype on ``dev``."""
        real_empty = self._saved[0]
        dtype, size, stride = meta.dtype, tuple(meta.shape), tuple(meta.stride())
        item = meta.element_size()
        extent = 0 if meta.numel() == 0 else 1 + sum((n - 1) * s for n, s in zip(size, stride))
        nbytes = extent * item
        body = -(-nbytes // ALIGN) * ALIGN
        raw = real_empty(GUARD + body + GUARD, dtype=torch.uint8, device=dev)
        _fill(raw, dtype, self.poison.value(dtype))
        t = real_empty(0, dtype=dtype, device=dev).set_(raw.untyped_storage(), GUARD // item, size, stride)
        rec = _Record()
        rec.raw, rec.offset, rec.nbytes, rec.body = raw, GUARD, nbytes, body
        rec.shape, rec.dtype = size, dtype
        rec.site, rec.modules = self._site()
        self.modules |= rec.modules
        self.records.append(rec)
        if requires_grad:
            t.requires_grad_(True)
        return t

    @staticmethod
    def _site():
        """("file:line in function" of the frame that called torch.empty, the package's files on the stack)."""
        f = sys._getframe(1)
        site, mods = None, set()
        while f is not None:
            name = f.f_code.co_filename
            if os.path.abspath(name) != _HERE:
                if site is None:
                    site = f"{name}:{f.f_lineno} in {f.f_code.co_name}"
                full = os.path.abspath(name)
                if full.startswith(_PKG):
                    mods.add(os.path.basename(full))
            f = f.f_back
        return site, mods

    # ---- checks ----------------------------------------------------------------------------------------------------
    def _pattern(self, dtype, dev, n):
        key = (dtype, dev, n)
        if key not in self._expected:
            want = self._saved[0](n, dtype=torch.uint8, device=dev) if self._saved else torch.empty(
                n, dtype=torch.uint8, device=dev)
            _fill(want, dtype, self.poison.value(dtype))
            self._expected[key] = want
        return self._expected[key]

    def verify(self):
        """Both guards of every buffer allocated so far still hold the poison, bit for bit."""
        if any(r.raw.is_cuda for r in self.records):
            torch.cuda.synchronize()
        for r in self.records:
            for which, lo, hi in (("front guard", 0, r.offset),
                                  ("back guard", r.offset + r.nbytes, r.offset + r.body + GUARD)):
                got = r.raw[lo:hi]
                want = self._pattern(r.dtype, r.raw.device, hi - lo)
                if not torch.equal(got, want):
                    first = int((got != want).nonzero()[0])
                    rel = first - (r.offset - lo) if which == "front guard" else first
                    where = (f"{-rel} bytes before the start" if which == "front guard"
                             else f"{rel} bytes past the end")
                    raise AssertionError(f"{which} overwritten, first changed byte {where} "
                                         f"(poison {self.poison.name}) -- {r.describe()}")

    def place(self, t):
        """A guarded copy of ``t`` (contiguous; detached)."""
        if self._saved is None or self not in _active:
            raise RuntimeError("place() outside the guarded context")
        out = torch.empty(t.shape, dtype=t.dtype, device=t.device)
        if t.device.type not in self.devices:
            raise RuntimeError(f"place(): {t.device} is not a guarded device type {self.devices}")
        out.copy_(t.detach())
        return out


def place(t):
    """Copy ``t`` into a guarded buffer of the innermost active context."""
    if not _active:
        raise RuntimeError("place() outside a guarded context")
    return _active[-1].place(t)


def same_bits(a, b):
    """torch.equal on the integer reinterpretation: NaN payloads and the sign of zero count."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.detach().contiguous().reshape(-1).view(torch.uint8),
                       b.detach().contiguous().reshape(-1).view(torch.uint8))
