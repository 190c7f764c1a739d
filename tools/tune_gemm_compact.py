"""Library-GEMM solutions for the mixer's strided-batched fp32 GEMMs at the compact batch counts of the DropPath route
(block.py: a mixer runs on 48, 52, 56 or 60 of the 64 samples), merged into si_mamba_amd/tuned/gemm_gfx950.csv, which
keys those GEMMs on the batch count (``..._B_64_...``).

    python tools/tune_gemm_compact.py tune 56 tuned/tune_B56.csv          # one batch count = one process, one time limit
    python tools/tune_gemm_compact.py merge tuned/tune_B*.csv             # add their strided-batched rows to the table

fp32 ONLY: TunableOp's sweep over the bf16 strided-batched candidates has faulted the GPU (DESIGN 4.6,
profiles/r02c_bf16_tune_fault*.log), so nothing here runs under autocast or in bf16, and the merge takes
``GemmStridedBatchedTunableOp_float_*`` rows only.  A result file whose validator lines (library versions) differ from
the table's is refused: TunableOp would ignore the table altogether.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, "si_mamba_amd", "tuned", "gemm_gfx950.csv")
PREFIX = "GemmStridedBatchedTunableOp_float_"


def tune(batch, out):
    from tools import measure
    measure.require_gpu("tune_gemm_compact.py")
    import torch
    import torch.cuda.tunable as tunable
    from si_mamba_amd.block import MixerModel
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    # the model's stack, two blocks of it: every mixer has the same GEMM shapes.  eval(): no DropPath, so both blocks
    # run at exactly `batch`; gradients still flow.
    m = MixerModel(d_model=384, n_layer=2).to(dev).eval()
    assert all(p.dtype == torch.float32 for p in m.parameters())
    x = torch.randn(batch, 1024, 384, device=dev, requires_grad=True)
    pos = torch.randn(batch, 1024, 384, device=dev)

    def step():
        m.zero_grad(set_to_none=True)
        m(x, pos).square().mean().backward()
        torch.cuda.synchronize()
    step()                                                  # untuned warm-up
    tunable.enable(True)
    tunable.set_max_tuning_duration(30)
    tunable.set_max_tuning_iterations(20)
    tunable.set_filename(out)
    tunable.tuning_enable(True)
    step()
    tunable.tuning_enable(False)
    if hasattr(tunable, "write_file"):                      # otherwise TunableOp writes `out` when the process ends
        tunable.write_file(out)
    rows = [r for r in tunable.get_results() if r[0].startswith(PREFIX)]
    print(f"B = {batch}: {len(rows)} strided-batched fp32 entries -> {out}", flush=True)


def merge(paths):
    table = open(TABLE).read().splitlines()
    validators = sorted(line for line in table if line.startswith("Validator,"))
    have = {tuple(line.split(",")[:2]) for line in table if not line.startswith("Validator,")}
    added = 0
    for path in paths:
        lines = open(path).read().splitlines()
        theirs = sorted(line for line in lines if line.startswith("Validator,"))
        if theirs != validators:
            raise SystemExit(f"{path}: validator lines differ from the table's -- these results are for other library "
                             f"versions:\n  " + "\n  ".join(theirs))
        for line in lines:
            key = tuple(line.split(",")[:2])
            if line.startswith(PREFIX) and "_B_64_" not in key[1] and key not in have:
                table.append(line)
                have.add(key)
                added += 1
    with open(TABLE, "w") as f:
        f.write("\n".join(table) + "\n")
    print(f"{added} rows added to {TABLE}")


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "tune":
        tune(int(sys.argv[2]), sys.argv[3])
    elif len(sys.argv) >= 3 and sys.argv[1] == "merge":
        merge(sys.argv[2:])
    else:
        raise SystemExit(__doc__)
