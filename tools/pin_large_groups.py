"""Fixtures for the large-G spectral kernels (128 < G <= 512).

    python tools/pin_large_groups.py        # from the repo root; the ref_* half needs the reference checkout

Writes, with the oracle's own generators (oracle/gen_golden.py spectral_case, oracle/pin_from_reference.py
spectral_fixture):
  tests/golden/spectral_g256.npz             unit-ball centres, B = 2, G = 256
  tests/golden/spectral_g512_surface.npz     surface_centers(2, 512, seed, npoints=8192): FPS centres of dense clouds
  tests/golden/ref_spectral_g256.npz, ref_spectral_g512_surface.npz   the reference's own function bodies on them

The (B,G,G) adjacencies would push the G = 512 files past the 1 MiB limit for a committed file, so every ``*.adj``
array is dropped: the tests recompute the adjacency with oracle.spectral_ref (tests/test_gpu_spectral_large.py).
The G = 512 files also drop the HLT records of the reference fixture, which nothing at that size reads.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gen_golden, pin_from_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
LIMIT = 1 << 20
CASES = [("spectral_g256", 256, 31, None), ("spectral_g512_surface", 512, 37, 8192)]


def _strip(path, drop_prefix=()):
    """Rewrite ``path`` without its adjacency arrays (and any key starting with ``drop_prefix``)."""
    with np.load(path, allow_pickle=False) as z:
        keep = {k: z[k] for k in z.files if not k.endswith(".adj") and not k.startswith(tuple(drop_prefix))}
    np.savez_compressed(path, **keep)
    size = os.path.getsize(path)
    assert size < LIMIT, (path, size)
    return size


def main():
    torch.set_num_threads(4)
    have_ref = pin_from_reference.reference_present()
    ref = pin_from_reference.load_reference() if have_ref else None
    for name, G, seed, npoints in CASES:
        centers = None
        if npoints is not None:
            centers = gen_golden.surface_centers(2, G, seed, npoints=npoints)
        gen_golden.spectral_case(name, 2, G, seed, centers=centers)
        print(f"{name}.npz: {_strip(os.path.join(OUT, name + '.npz'))} bytes")
        if ref is None:
            print("reference not present: ref_* fixtures not rewritten", file=sys.stderr)
            continue
        methods, sast, hlt_fn, _ = ref
        pin_from_reference.spectral_fixture(name, methods, sast, hlt_fn)
        drop = ("hlt.",) if G > 256 else ()
        print(f"ref_{name}.npz: {_strip(os.path.join(OUT, 'ref_' + name + '.npz'), drop)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
