"""Timing and A/B helpers for the tools in this directory: the one place here that records device events, takes the host
clock around a synchronised region, or starts timing processes.  tools/README.md says which tool uses which function.

    window, calls          ms per call: two events around back-to-back calls (launch gaps hidden behind the queue)
    per_call_median        ms per call: an event pair and a synchronise per call (the launch gap is inside)
    alternate              raw windows of several operations, one window of each per round
    host_clock             ms per step on the host clock between two device synchronises (what a training loop waits for)
    rounds                 zero-argument timers called in turn, n times over
    median, stats, summary the two shapes the committed profiles use
    fresh_processes        one child process per figure, the variants alternating, stopping at the first that fails

torch is imported inside the functions that need it: fresh_processes runs in drivers that must not open the device.
"""
import json
import os
import statistics
import subprocess
import sys
import time

median = statistics.median


def stats(v, nd):
    return [round(median(v), nd), round(min(v), nd), round(max(v), nd)]


def summary(v, nd):
    return {"median": round(median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd), "n": len(v)}


def require_gpu(tool):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool} needs a ROCm device: a time from anything else says nothing")


def use_lib_from_env():
    """SIMAMBA_LIB=<path> makes this process load that build of the library (tools/build_alt.sh, or another tree's)."""
    from si_mamba_amd import _lib
    if os.environ.get("SIMAMBA_LIB"):
        _lib.LIB_PATH = os.path.abspath(os.environ["SIMAMBA_LIB"])
    return _lib


def window(fn, reps, stream=None):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _warm(fn, n):
    import torch
    for _ in range(n):
        fn()
    torch.cuda.synchronize()


def calls(fn, *, warmup, reps, stream=None):
    _warm(fn, warmup)
    return window(fn, reps, stream)


def per_call_median(fn, *, warmup, reps):
    _warm(fn, warmup)
    return median([window(fn, 1) for _ in range(reps)])


def alternate(ops, *, target_ms=200.0, windows=5, reps=None, warmup=2, reverse_odd=False, window=window):
    """ops: name -> callable.  Every op is warmed up (`warmup` calls) and, where `reps` is None, its window is sized to
    about `target_ms` from a probe window of `warmup` calls.  Then `windows` rounds, one window of every op per round,
    in the opposite order every other round with `reverse_odd`.  Returns name -> the raw ms per call of each window."""
    n = {}
    for name, fn in ops.items():
        _warm(fn, warmup)
        n[name] = reps if reps is not None else max(1, min(2000, int(target_ms / max(window(fn, warmup), 1e-3))))
    ts = {name: [] for name in ops}
    for r in range(windows):
        for name in (list(ops)[::-1] if reverse_odd and r % 2 else ops):
            ts[name].append(window(ops[name], n[name]))
    return ts


def host_clock(fn, *, steps, warmup):
    import torch
    _warm(fn, warmup)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def rounds(fns, n):
    got = {k: [] for k in fns}
    for _ in range(n):
        for k, fn in fns.items():
            got[k].append(fn())
    return got


def last_json_line(text):
    return json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])


def fresh_processes(variants, rounds, *, timeout_s, parse=last_json_line):
    """variants: [(name, cwd, argv)].  `rounds` times over, every variant runs once as a child of its own, one at a
    time, under `timeout -k 10 timeout_s`.  Returns name -> [parse(stdout), ...].

    The first child that does not exit 0 -- a time limit (124, 137), an abort (134), a segmentation fault (139) or an
    error of its own -- ends the run: nothing more is started on a device that a process has just faulted or hung."""
    out = {name: [] for name, _, _ in variants}
    for r in range(rounds):
        for name, cwd, argv in variants:
            print(f"run {r + 1} of {rounds}: {name}", file=sys.stderr, flush=True)
            p = subprocess.run(["timeout", "-k", "10", str(timeout_s)] + list(argv), cwd=cwd, capture_output=True,
                               text=True)
            if p.returncode != 0:
                why = f" (timed out after {timeout_s} s)" if p.returncode in (124, 137) else ""
                print(f"{name}: exit status {p.returncode}{why}; no further process started\n{p.stderr[-4000:]}",
                      file=sys.stderr, flush=True)
                raise SystemExit(1)
            out[name].append(parse(p.stdout))
    return out
