"""Space-filling-curve orders (csrc/curve_order.hip, spectral.curve_order) on one GPU: the one-launch kernel against the
same orders composed from torch ops, and against the eigen-ordering it stands next to.

Shapes (B, G): (64, 128), (64, 512), (16, 8192); k = 4 curves (hilbert, hilbert-trans, z, z-trans), bits = 10, the
cloud's own box.  Per shape, us per call:
  kernel          spectral.curve_order, eager calls back to back, one replay of its hipGraph, and per launch of a
                  hipGraph of 16 launches (the kernel without the host's and the graph launch's share)
  torch_composed  the float64 cell, the Skilling / Morton bit loops and a sort of code << 13 | index as torch ops (below:
                  they live here, not in the package), eager and as a hipGraph; its orders are checked to equal the
                  kernel's before anything is timed
  spectral_order  the fused graph + eigen-solver + argsort (the model's SAST ordering), at the first two shapes, for scale
Device events around back-to-back calls, 5 windows per variant, the variants alternating (measure.alternate).

``--bench-parent`` / ``--bench-this``: files holding the JSON line of ``python bench.py`` on the parent commit and on this
tree (the flagship step runs SAST and none of this code); both lines are recorded next to the figures.
``SIMAMBA_LIB=<path>`` times another build of the library (measure.use_lib_from_env).

    python tools/bench_curve_order.py [--bench-parent FILE --bench-this FILE] [--out profiles/curve_order.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import measure  # noqa: E402

SHAPES = [(64, 128), (64, 512), (16, 8192)]
CURVES = ("hilbert", "hilbert-trans", "z", "z-trans")
BITS = 10
IN_GRAPH = 16
GRAPH = dict(knn_graph=20, alpha=10.0, k_top_eigenvectors=4, smallest=True, symmetric=True, self_loop=False, binary=True)


# ---- the same orders from torch ops ----------------------------------------------------------------------------------
def _interleave(x, y, z, bits):
    code = torch.zeros_like(x)
    for i in range(bits):
        code |= ((x >> i) & 1) << (3 * i + 2)
        code |= ((y >> i) & 1) << (3 * i + 1)
        code |= ((z >> i) & 1) << (3 * i)
    return code


def _hilbert(x, y, z, bits):
    X = [x.clone(), y.clone(), z.clone()]
    Q = 1 << (bits - 1)
    while Q > 1:
        P = Q - 1
        for i in range(3):
            hit = (X[i] & Q) != 0
            t = torch.where(hit, torch.zeros_like(X[0]), (X[0] ^ X[i]) & P)
            X[0] = torch.where(hit, X[0] ^ P, X[0] ^ t)
            if i:
                X[i] = X[i] ^ t
        Q >>= 1
    X[1] = X[1] ^ X[0]
    X[2] = X[2] ^ X[1]
    t = torch.zeros_like(X[0])
    Q = 1 << (bits - 1)
    while Q > 1:
        t = torch.where((X[2] & Q) != 0, t ^ (Q - 1), t)
        Q >>= 1
    return _interleave(X[0] ^ t, X[1] ^ t, X[2] ^ t, bits)


def torch_composed(center, curves=CURVES, bits=BITS):
    """(B, G, 3) finite centres -> (B, k, G) int64, the kernel's orders under box="cloud"."""
    lo = center.amin(1, keepdim=True)
    ext = (center.amax(1, keepdim=True) - lo).amax(2, keepdim=True)
    v = (center.double() - lo.double()) / ext.double() * float(1 << bits)
    q = v.floor().clamp_(0, (1 << bits) - 1).long()
    q = torch.where(ext == 0, torch.zeros_like(q), q)
    x, y, z = q.unbind(-1)
    index = torch.arange(center.shape[1], device=center.device)
    out = []
    for name in curves:
        a, b = (y, x) if name.endswith("-trans") else (x, y)
        code = (_hilbert if name.startswith("hilbert") else _interleave)(a, b, z, bits)
        out.append(torch.sort(code << 13 | index, dim=1)[1])
    return torch.stack(out, 1)


# ---- timing ----------------------------------------------------------------------------------------------------------
def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def shape_figures(B, G, dev):
    from si_mamba_amd import spectral
    from si_mamba_amd.synthetic import make_clouds
    center = make_clouds(B, G, 1, dev).contiguous()
    kernel = lambda: spectral.curve_order(center, CURVES, BITS)                       # noqa: E731
    composed = lambda: torch_composed(center)                                        # noqa: E731
    same = bool(torch.equal(kernel(), composed()))
    ops = {"kernel": kernel, "torch_composed": composed}
    if G <= 512:
        ops["spectral_order"] = lambda: spectral.spectral_order(center, **GRAPH)
    graphs = {k + "_graph": _capture(fn).replay for k, fn in ops.items()}
    # IN_GRAPH launches in one graph, per launch: the kernel without the host's and the graph launch's share
    graphs["kernel_in_graph_of_%d" % IN_GRAPH] = _capture(lambda: [kernel() for _ in range(IN_GRAPH)]).replay
    acc = measure.alternate({**ops, **graphs}, target_ms=100.0, windows=5, reverse_odd=True)
    acc = {k: [x / IN_GRAPH for x in v] if k.startswith("kernel_in_graph_of") else v for k, v in acc.items()}
    us = {k: measure.summary([1e3 * x for x in v], 2) for k, v in acc.items()}
    return dict(B=B, G=G, k=len(CURVES), bits=BITS, composed_orders_equal_kernel=same, us_per_call=us,
                kernel_over_composed=round(us["kernel"]["median"] / us["torch_composed"]["median"], 4),
                kernel_graph_over_composed_graph=round(us["kernel_graph"]["median"] /
                                                       us["torch_composed_graph"]["median"], 4))


def _line(path):
    if not path:
        return None
    with open(path) as fh:
        return measure.last_json_line(fh.read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-parent", default=None, help="file with the JSON line of bench.py on the parent commit")
    ap.add_argument("--bench-this", default=None, help="the same on this tree")
    args = ap.parse_args()
    measure.require_gpu("bench_curve_order.py")
    measure.use_lib_from_env()
    dev = torch.device("cuda:0")
    line = json.dumps(dict(
        what="space-filling-curve orders, k = 4 curves, 10 bits per axis, one MI355X: spectral.curve_order (one launch) "
             "against the same orders composed from torch ops (float64 cell, bit loops, one sort per curve) and, at the "
             "model's sizes, against spectral_order; us per call, eager calls back to back and hipGraph replays, events "
             "around 5 windows of ~0.1 s per variant, the variants alternating.  bench_py: the flagship step (SAST, none "
             "of this code) on the parent commit and on this tree",
        device=torch.cuda.get_device_name(0), shapes=[shape_figures(B, G, dev) for B, G in SHAPES],
        bench_py=dict(parent=_line(args.bench_parent), this=_line(args.bench_this))))
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
