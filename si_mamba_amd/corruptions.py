"""Point-cloud corruptions on the device (csrc/corrupt.hip) and the robustness score built on them.

``corrupt(points, kind, severity)`` damages every cloud of a ``(B, N, 3)`` float32 device batch in one launch and, unlike
the augmentations of ``transforms``, changes its size: it returns ``(out (B, K, 3), out_lengths (B,))``, which is what
``PointMamba.forward(points, lengths=)`` takes.  Nothing is read on the host, so ``DeviceLoader.fetch()`` ->
``corrupt()`` -> ``model(x, lengths=out_lengths)`` can sit in a captured graph.

The seven kinds follow the families of ModelNet-C (Ren, Pan, Liu: "Benchmarking and Analyzing Point Cloud Classification
under Corruptions", ICML 2022): points removed globally or in k-NN clusters, uniform outliers or Gaussian clusters added,
a bounded rotation about all three axes, an anisotropic scale followed by re-normalisation, and jitter.  ``SEVERITY``
holds five parameter sets per kind.  Its constants were written from the paper's description without its code at hand:
they are plain defaults, not a reproduction of the benchmark, and the draws (counter-based Philox, the layout is in
include/simamba.h) differ from the benchmark's numpy streams in any case.  Scores computed here are therefore
comparable with each other, not with published ModelNet-C tables.

``evaluate_robustness`` scores a classifier on the clean clouds and on every (kind, severity), and with a baseline's
error rates forms the corruption errors CE, mCE and their clean-relative forms RCE, RmCE of that paper.  No baseline
table is shipped.

There is no CPU route and nothing here is differentiable: inputs on the CPU or with ``requires_grad`` are refused.
"""
from __future__ import annotations

import ctypes
import inspect
import math

import torch

from . import _lib
from .transforms import AugmentState, _check_points, _index, default_state, launch_corrupt

__all__ = ["KINDS", "SEVERITY", "corrupt", "evaluate_robustness"]

KINDS = ("drop_global", "drop_local", "add_global", "add_local", "rotate", "scale", "jitter")

# kind -> (opcode, parameter names in the order of the ABI's params array, renorm default)
_SPEC = {
    "drop_global": (_lib.CORRUPT_DROP_GLOBAL, ("ratio",), False),
    "drop_local": (_lib.CORRUPT_DROP_LOCAL, ("total", "max_clusters"), False),
    "add_global": (_lib.CORRUPT_ADD_GLOBAL, ("count", "radius"), False),
    "add_local": (_lib.CORRUPT_ADD_LOCAL, ("total", "max_clusters", "sigma_low", "sigma_high"), False),
    "rotate": (_lib.CORRUPT_ROTATE3, ("theta",), False),
    "scale": (_lib.CORRUPT_SCALE_AXES, ("scale",), True),
    "jitter": (_lib.CORRUPT_JITTER, ("sigma",), False),
}
# the parameter that says how many points a kind can add
_ADDS = {"add_global": "count", "add_local": "total"}

SEVERITY = {
    "drop_global": tuple(dict(ratio=r) for r in (0.25, 0.375, 0.5, 0.625, 0.75)),
    "drop_local": tuple(dict(total=100 * l, max_clusters=8) for l in range(1, 6)),
    "add_global": tuple(dict(count=10 * l, radius=1.0) for l in range(1, 6)),
    "add_local": tuple(dict(total=100 * l, max_clusters=8, sigma_low=0.075, sigma_high=0.125) for l in range(1, 6)),
    "rotate": tuple(dict(theta=math.pi * l / 30) for l in range(1, 6)),
    "scale": tuple(dict(scale=s) for s in (1.6, 1.7, 1.8, 1.9, 2.0)),
    "jitter": tuple(dict(sigma=0.01 * l) for l in range(1, 6)),
}


def kind_params(kind, severity=None, **params):
    """The parameter dict of ``kind``: ``SEVERITY[kind][severity - 1]`` (severity 1..5) overridden by ``params``; every
    parameter of the kind must end up set."""
    if kind not in _SPEC:
        raise ValueError(f"corrupt: unknown kind {kind!r}; the kinds are {', '.join(KINDS)}")
    names = _SPEC[kind][1]
    unknown = sorted(set(params) - set(names))
    if unknown:
        raise TypeError(f"corrupt: {kind} takes {', '.join(names)}, not {', '.join(unknown)}")
    got = {}
    if severity is not None:
        if severity not in (1, 2, 3, 4, 5):
            raise ValueError(f"corrupt: severity must be 1..5 or None, got {severity!r}")
        got.update(SEVERITY[kind][severity - 1])
    got.update(params)
    if kind == "add_global":
        got.setdefault("radius", 1.0)
    missing = [k for k in names if k not in got]
    if missing:
        raise TypeError(f"corrupt: {kind} needs {', '.join(missing)} (or a severity)")
    return got


def corrupt(points, kind, severity=None, *, lengths=None, state=None, out=None, renorm=None, return_src=False,
            **params):
    """One corruption of every cloud, in one launch: ``(out, out_lengths)`` or, with ``return_src``,
    ``(out, out_lengths, src)``.

    ``points`` (B, N, 3) float32 on the device.  ``kind``: one of ``KINDS``; its parameters come from
    ``SEVERITY[kind][severity - 1]`` and / or keywords (``ratio`` | ``total``, ``max_clusters`` | ``count``, ``radius`` |
    ``total``, ``max_clusters``, ``sigma_low``, ``sigma_high`` | ``theta`` | ``scale`` | ``sigma``).  ``lengths`` (B,)
    integers: cloud ``b`` has ``lengths[b]`` real rows (clamped to [1, N]); the rows behind are never read.  ``state``: an
    ``AugmentState`` (default: the device's ``default_state``; the kernel draws under a key of its own, so sharing the
    state with the augmentations shares no stream); its step advances by 1.  ``out`` (B, K, 3) float32 with
    N <= K <= 8192: the result's storage, not overlapping ``points``; by default K = N + the number of points the kind
    can add (at most 8192), so nothing is clamped.  With a smaller K, added points stop at row K.  ``renorm``: follow
    with the unit-sphere normalisation of the result (default: the kind's own, True for ``scale`` only).

    ``out_lengths`` (B,) int64: the rows of every result; the rows behind are 0.  ``src`` (B, K) int32: the input row
    every output row came from, -1 for a global outlier, ``-1 - j`` for a point of local cluster ``j``, INT_MIN behind
    the length.  Nothing is read on the host, so the call can be captured in a graph."""
    what = "corrupt"
    _check_points(points, what)
    got = kind_params(kind, severity, **params)
    code, names, renorm_default = _SPEC[kind]
    dev = points.device
    B, N, _ = points.shape
    p = points.contiguous()
    if lengths is not None:
        lengths = _index(lengths, (B,), f"{what}: lengths", dev)
    if state is None:
        state = default_state(dev)
    elif not isinstance(state, AugmentState):
        raise TypeError(f"{what}: state must be an AugmentState, got {type(state).__name__}")
    if state.device != dev:
        raise ValueError(f"{what}: the state is on {state.device}, the points are on {dev}")
    if out is None:
        adds = max(int(got[_ADDS[kind]]), 0) if kind in _ADDS else 0
        out = torch.empty(B, min(N + adds, _lib.CORRUPT_MAX_POINTS), 3, device=dev, dtype=torch.float32)
    else:
        if (not torch.is_tensor(out) or out.dim() != 3 or out.shape[0] != B or out.shape[2] != 3
                or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous()):
            raise ValueError(f"{what}: out must be a contiguous ({B}, K, 3) float32 tensor on {dev}")
        if out.requires_grad:
            raise RuntimeError(f"{what}: out requires grad")
        if not N <= out.shape[1] <= _lib.CORRUPT_MAX_POINTS:
            raise ValueError(f"{what}: out has K = {out.shape[1]} rows per cloud, need {N} <= K <= "
                             f"{_lib.CORRUPT_MAX_POINTS}")
    K = out.shape[1]
    out_lengths = torch.empty(B, device=dev, dtype=torch.int64)
    src = torch.empty(B, K, device=dev, dtype=torch.int32) if return_src else None
    host = (ctypes.c_float * 4)(*[float(got[k]) for k in names])
    flags = _lib.CORRUPT_RENORM if (renorm_default if renorm is None else renorm) else 0
    launch_corrupt(p, lengths, out, out_lengths, src, state, code, flags, host)
    return (out, out_lengths, src) if return_src else (out, out_lengths)


def _takes_lengths(model):
    fn = model.forward if isinstance(model, torch.nn.Module) else model
    try:
        sig = inspect.signature(fn)
    except (TypeError, ValueError):
        return True                                              # not introspectable: the call itself will tell
    return "lengths" in sig.parameters or any(q.kind is q.VAR_KEYWORD for q in sig.parameters.values())


def robustness_scores(clean_correct, correct, total, kinds, severities, baseline=None):
    """The arithmetic of ``evaluate_robustness`` on counts: ``clean_correct`` an int, ``correct[k][s]`` ints for
    ``kinds[k]`` at ``severities[s]``, ``total`` clouds."""
    res = {"total": int(total), "clean_acc": clean_correct / total, "clean_err": 1.0 - clean_correct / total,
           "acc": {}, "err": {}}
    for k, kind in enumerate(kinds):
        res["acc"][kind] = [int(c) / total for c in correct[k]]
        res["err"][kind] = [1.0 - int(c) / total for c in correct[k]]
    res["mean_acc"] = sum(sum(v) for v in res["acc"].values()) / max(1, len(kinds) * len(severities))
    if baseline is not None:
        base_clean = float(baseline["clean"])
        ce, rce = {}, {}
        for kind in kinds:
            base = [float(v) for v in baseline[kind]]
            if len(base) != len(severities):
                raise ValueError(f"evaluate_robustness: baseline[{kind!r}] has {len(base)} error rates, "
                                 f"{len(severities)} severities are scored")
            ce[kind] = sum(res["err"][kind]) / sum(base)
            rce[kind] = (sum(e - res["clean_err"] for e in res["err"][kind]) / sum(v - base_clean for v in base))
        res["CE"], res["RCE"] = ce, rce
        res["mCE"] = sum(ce.values()) / len(ce)
        res["RmCE"] = sum(rce.values()) / len(rce)
    return res


@torch.no_grad()
def evaluate_robustness(model, points, labels, *, lengths=None, kinds=KINDS, severities=(1, 2, 3, 4, 5), batch_size=64,
                        state=None, baseline=None):
    """Score a classifier on clean and corrupted clouds.

    ``model(x, lengths=l)`` -> logits (b, classes) is called on batches of at most ``batch_size`` clouds: once on the
    clean clouds (with ``lengths`` as given, or without the keyword when ``lengths`` is None) and once per (kind,
    severity) on ``corrupt``'s output with its ``out_lengths``.  A model whose ``forward`` does not take ``lengths`` is
    refused up front (TypeError).  ``points`` (S, N, 3) float32 and ``labels`` (S,) integers on the device; put the
    model in ``eval()`` mode first.  ``state``: the ``AugmentState`` the corruptions draw from.

    The correct counts accumulate in one device tensor that is read once, at the end.  Returns a dict: ``total``,
    ``clean_acc``, ``clean_err``, ``acc[kind]`` / ``err[kind]`` (lists over ``severities``), ``mean_acc``; and with
    ``baseline`` = ``{"clean": its clean error rate, kind: [its error rate per severity], ...}``:
    ``CE[kind] = sum_l err / sum_l err_base``, ``mCE`` their mean, ``RCE[kind] = sum_l (err - clean_err) /
    sum_l (err_base - clean_base)`` and ``RmCE`` their mean."""
    what = "evaluate_robustness"
    if not _takes_lengths(model):
        raise TypeError(f"{what}: the model's forward takes no `lengths` keyword; corrupted clouds differ in size")
    _check_points(points, what)
    kinds, severities = tuple(kinds), tuple(severities)
    for kind in kinds:
        for sev in severities:
            kind_params(kind, sev)
    if baseline is not None:
        missing = [k for k in ("clean",) + kinds if k not in baseline]
        if missing:
            raise ValueError(f"{what}: the baseline lacks {', '.join(missing)}")
    dev = points.device
    S = points.shape[0]
    labels = _index(labels, (S,), f"{what}: labels", dev)
    if lengths is not None:
        lengths = _index(lengths, (S,), f"{what}: lengths", dev)
    if batch_size < 1:
        raise ValueError(f"{what}: batch_size must be at least 1")
    correct = torch.zeros(1 + len(kinds) * len(severities), device=dev, dtype=torch.int64)
    for lo in range(0, S, batch_size):
        x = points[lo:lo + batch_size].contiguous()
        y = labels[lo:lo + batch_size]
        ln = None if lengths is None else lengths[lo:lo + batch_size]
        logits = model(x) if ln is None else model(x, lengths=ln)
        correct[0] += (logits.argmax(-1) == y).sum()
        slot = 1
        for kind in kinds:
            for sev in severities:
                cx, cl = corrupt(x, kind, sev, lengths=ln, state=state)
                correct[slot] += (model(cx, lengths=cl).argmax(-1) == y).sum()
                slot += 1
    host = correct.tolist()                                      # the one host read
    per_kind = [host[1 + k * len(severities):1 + (k + 1) * len(severities)] for k in range(len(kinds))]
    return robustness_scores(host[0], per_kind, S, kinds, severities, baseline)
