"""Timings of the large-G spectral path (128 < G <= 512) and of farthest-point sampling on 8192-point clouds.

    python tools/bench_large_groups.py [--out profiles/large_groups.json] [--kernels-only]

Device events after warm-up, median of the timed repeats:
  * spectral_order (centres -> graph -> top-4 eigenpairs -> orders) at B = 64, G = 128 / 256 / 512;
  * the HLT route, create_graph_from_centers + the top-k eigen call, at the same sizes;
  * the rocSOLVER baseline, batched torch.linalg.eigh of the (64, 512, 512) random-walk Laplacians;
  * FPS (64, 8192 -> 512);
  * one PointMamba train step (the reference's fine-tune architecture: 12 blocks, d = 384) on 8192-point clouds with
    512 patches of 32, fp32 and bf16 autocast, in clouds/s.
``--kernels-only`` runs the spectral and FPS calls a few times without timing, for a rocprofv3 --kernel-trace --stats
run.  Also printed: the bytes the Householder pass of the large-G kernel moves per sample, from the shape.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from si_mamba_amd import grouping, spectral  # noqa: E402
from si_mamba_amd.synthetic import unit_ball_centers  # noqa: E402
from tools import measure  # noqa: E402


def median_ms(fn, warmup=3, reps=10):
    return measure.per_call_median(fn, warmup=warmup, reps=reps)


def householder_bytes(G):
    """Global bytes of the fused Householder pass for one G x G sample (fp32, full square): reflector k reads and
    writes its (G-k-1)^2 trailing block once (update k-1 fused with matvec k), plus one row for the next reflector;
    the Laplacian build writes G^2 and reads the adjacency twice."""
    tri = sum(8 * m * m + 8 * m for m in range(2, G))
    build = 4 * G * G + 2 * 4 * G * G
    return tri + build


def clouds(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(B, N, 3, generator=g)
    p = p - p.mean(1, keepdim=True)
    return p / p.norm(dim=-1).max(dim=1)[0][:, None, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    measure.require_gpu("bench_large_groups.py")
    dev = torch.device("cuda:0")
    B = 64
    cent = {G: unit_ball_centers(B, G, 0).to(dev) for G in (128, 256, 512)}
    pts = clouds(B, 8192, 1).to(dev)

    def order(G):
        return spectral.spectral_order(cent[G], 20, 10.0, 4, smallest=True, symmetric=True, self_loop=False,
                                       binary=True)

    def hlt(G):
        adj = spectral.create_graph_from_centers(cent[G], 20, 10.0, True, False, True)
        return spectral._eig(adj, 4, True, False, want_all=False)

    if args.kernels_only:
        for _ in range(3):
            for G in (128, 256, 512):
                order(G)
                hlt(G)
            grouping.sample_farthest_points(pts, 512)
        torch.cuda.synchronize()
        return 0

    rec = {"device": torch.cuda.get_device_name(0), "batch": B, "spectral_order_ms": {}, "hlt_graph_eig_ms": {},
           "householder_bytes_per_sample": {G: householder_bytes(G) for G in (128, 256, 512)}}
    for G in (128, 256, 512):
        rec["spectral_order_ms"][G] = median_ms(lambda: order(G))
        rec["hlt_graph_eig_ms"][G] = median_ms(lambda: hlt(G))
        print(f"G={G}: spectral_order {rec['spectral_order_ms'][G]:.3f} ms, graph + eig {rec['hlt_graph_eig_ms'][G]:.3f} ms"
              f" (B={B}); Householder pass {rec['householder_bytes_per_sample'][G] / 1e6:.1f} MB per sample", flush=True)
    adj = spectral.create_graph_from_centers(cent[512], 20, 10.0, True, False, True)
    A = (adj + adj.transpose(1, 2)) / 2
    Lrw = torch.eye(512, device=dev)[None] - (1.0 / (A.sum(2) + 1e-6))[:, :, None] * A
    rec["rocsolver_eigh_batched_ms_512"] = median_ms(lambda: torch.linalg.eigh(Lrw), warmup=2, reps=5)
    print(f"rocSOLVER eigh batched (64, 512, 512): {rec['rocsolver_eigh_batched_ms_512']:.2f} ms", flush=True)
    rec["fps_ms_64x8192_to_512"] = median_ms(lambda: grouping.sample_farthest_points(pts, 512))
    print(f"FPS (64, 8192 -> 512): {rec['fps_ms_64x8192_to_512']:.3f} ms", flush=True)

    from si_mamba_amd.point_mamba import PointMamba, default_config
    Bm = 8
    torch.manual_seed(0)
    m = PointMamba(default_config(num_group=512, group_size=32)).to(dev).train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4)
    x = clouds(Bm, 8192, 2).to(dev)
    gt = torch.randint(0, 15, (Bm,), device=dev)
    rec["train_step"] = {"batch": Bm, "npoints": 8192, "num_group": 512, "group_size": 32}
    for name, dt in (("fp32", None), ("bf16", torch.bfloat16)):
        def step():
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=dt, enabled=dt is not None):
                loss, _ = m.get_loss_acc(m(x), gt)
            loss.backward()
            opt.step()
        ms = median_ms(step, warmup=2, reps=5)
        rec["train_step"][name + "_ms"] = ms
        rec["train_step"][name + "_clouds_per_s"] = Bm / ms * 1e3
        print(f"PointMamba train step {name} (B={Bm}, 8192 pts, 512 patches): {ms:.1f} ms -> {Bm / ms * 1e3:.1f} "
              f"clouds/s", flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
