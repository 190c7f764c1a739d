import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import measure
measure.require_gpu("bench_spectral.py")
from si_mamba_amd import spectral
from si_mamba_amd.synthetic import unit_ball_centers
dev = torch.device("cuda:0")
for B, G in [(64, 128), (128, 128), (256, 128), (64, 64), (512, 64), (64, 256), (64, 512)]:
    c = unit_ball_centers(B, G, 0).to(dev)
    ms = measure.per_call_median(lambda: spectral.spectral_order(c, 20, 10.0, 4, smallest=True, symmetric=True,
                                                                 self_loop=False, binary=True), warmup=3, reps=10)
    print(f"spectral_order B={B} G={G}: median {ms:.3f} ms -> {B/ms*1e3:.0f} matrices/s")

# rocSOLVER baseline: torch.linalg.eigh on the device = hipSOLVER/rocSOLVER syevd, batched and in the
# reference's per-sample loop (models/point_mamba.py:725-742), on the same Laplacians
from si_mamba_amd.spectral import create_graph_from_centers
for B, G in [(64, 128), (64, 64)]:
    c = unit_ball_centers(B, G, 0).to(dev)
    adj = create_graph_from_centers(c, 20, 10.0, True, False, True)
    A = (adj + adj.transpose(1, 2)) / 2
    Lrw = torch.eye(G, device=dev)[None] - (1.0 / (A.sum(2) + 1e-6))[:, :, None] * A
    for name, fn in [("batched", lambda: torch.linalg.eigh(Lrw)),
                     ("per-sample loop", lambda: [torch.linalg.eigh(Lrw[i]) for i in range(B)])]:
        ms = measure.per_call_median(fn, warmup=2, reps=5)
        print(f"rocSOLVER eigh {name} B={B} G={G}: median {ms:.2f} ms -> {B/ms*1e3:.0f} matrices/s")
