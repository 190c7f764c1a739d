"""A/B of the bf16 step with in_proj through the hand-written kernel (default where its grid fills the chip) and through the
library GEMM, fresh bench.py processes alternating in one session:  python tools/ab_in_proj.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import measure

ROUTES = {"None": None, "False": False}                # None: the default route; False: library GEMM
if "--child" in sys.argv:
    hand = ROUTES[sys.argv[sys.argv.index("--child") + 1]]
    sys.argv = ["bench.py", "--steps", "4", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-headline"]
    from si_mamba_amd import _lib
    _lib._hand_in_proj[0] = hand
    import bench
    bench.main()
else:
    runs = measure.fresh_processes([(h, ROOT, [sys.executable, os.path.abspath(__file__), "--child", h]) for h in ROUTES],
                                   2, timeout_s=600, parse=lambda txt: measure.last_json_line(txt)["bf16_step"])
    for i in range(2):
        for h in ROUTES:
            d = runs[h][i]
            print(d["value"], "clouds/s", d["ms_per_step"], "ms", d["routes"], d["kernels"].get("in_proj_fwd"))
