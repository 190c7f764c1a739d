"""tools/measure.py: the statistics, the scheduling of alternating windows and rounds (with a scripted fake window), the
process driver (children that never import torch), that every GPU-timing tool refuses to run without a device, and,
on the device, that each timer returns a finite positive time.  No test compares one time with another."""
import json
import math
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import measure  # noqa: E402


# ---- statistics -----------------------------------------------------------------------------------------------------
def test_median_stats_summary():
    odd, even = [3.14159, 1.0, 2.71828], [4.0, 1.0, 2.0, 3.5]
    assert measure.median(odd) == 2.71828
    assert measure.median(even) == 2.75                       # statistics.median: the mean of the middle two
    assert measure.stats(odd, 2) == [2.72, 1.0, 3.14]
    assert measure.stats(even, 1) == [2.8, 1.0, 4.0]          # round(2.75, 1): 2.75 is exact in binary, ties to even
    assert measure.summary(odd, 3) == {"median": 2.718, "min": 1.0, "max": 3.142, "n": 3}
    assert measure.summary(even, 0) == {"median": 3.0, "min": 1.0, "max": 4.0, "n": 4}


# ---- alternate and rounds: the order of the windows, with a fake window --------------------------------------------
class FakeWindow:
    """window(fn, reps) -> the next scripted time of fn; logs (name, reps).  The ops are `lambda: name`."""

    def __init__(self, times):
        self.times, self.log = {k: list(v) for k, v in times.items()}, []

    def __call__(self, fn, reps):
        self.log.append((fn(), reps))
        return self.times[fn()].pop(0)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(measure, "_warm", lambda fn, n: [fn() for _ in range(n)])


OPS = {"a": lambda: "a", "b": lambda: "b"}


def test_alternate_sizes_windows_and_alternates(no_device):
    # probes: a 0.5 ms -> 200 / 0.5 = 400 reps; b 40 ms -> 5 reps; then three rounds of scripted windows
    fake = FakeWindow({"a": [0.5, 1.0, 2.0, 3.0], "b": [40.0, 10.0, 20.0, 30.0]})
    got = measure.alternate(OPS, target_ms=200.0, windows=3, window=fake)
    assert got == {"a": [1.0, 2.0, 3.0], "b": [10.0, 20.0, 30.0]}
    assert fake.log == [("a", 2), ("b", 2)] + [("a", 400), ("b", 5)] * 3


def test_alternate_clamps_reps(no_device):
    # a: a probe of 0 ms counts as 1e-3 ms -> 200 000, clamped to 2000; b: 1000 ms -> int(0.2) = 0, clamped to 1
    fake = FakeWindow({"a": [0.0, 1.0], "b": [1000.0, 1.0]})
    measure.alternate(OPS, target_ms=200.0, windows=1, window=fake)
    assert fake.log[2:] == [("a", 2000), ("b", 1)]


def test_alternate_fixed_reps_and_reverse_odd(no_device):
    fake = FakeWindow({"a": [1.0, 2.0, 3.0], "b": [10.0, 20.0, 30.0]})
    got = measure.alternate(OPS, windows=3, reps=7, reverse_odd=True, window=fake)
    assert fake.log == [(n, 7) for n in "abbaab"]             # no probe: reps taken as given
    assert got == {"a": [1.0, 2.0, 3.0], "b": [10.0, 20.0, 30.0]}


def test_rounds_call_order():
    log = []
    got = measure.rounds({"x": lambda: log.append("x") or len(log), "y": lambda: log.append("y") or len(log)}, 3)
    assert log == list("xyxyxy")
    assert got == {"x": [1, 3, 5], "y": [2, 4, 6]}


# ---- fresh_processes: children that append their name to a file and print one JSON line ----------------------------
def child(name, path, then="pass"):
    code = (f"import json\nopen({path!r}, 'a').write({name!r} + '\\n')\n{then}\n"
            f"print('noise')\nprint(json.dumps(dict(who={name!r}, n=len(open({path!r}).read().split()))))\n")
    return name, None, [sys.executable, "-S", "-c", code]


def started(path):
    return open(path).read().split()


def test_fresh_processes_alternate_and_parse(tmp_path):
    path = str(tmp_path / "log")
    got = measure.fresh_processes([child("p", path), child("t", path)], 2, timeout_s=60)
    assert started(path) == ["p", "t", "p", "t"]
    assert got == {"p": [dict(who="p", n=1), dict(who="p", n=3)], "t": [dict(who="t", n=2), dict(who="t", n=4)]}
    only_n = measure.fresh_processes([child("p", path)], 1, timeout_s=60,
                                     parse=lambda s: measure.last_json_line(s)["n"])
    assert only_n == {"p": [5]}


def test_fresh_processes_stop_at_first_failure(tmp_path, capfd):
    path = str(tmp_path / "log")
    bad = child("bad", path, then="import sys\nsys.stderr.write('it broke\\n')\nsys.exit(3)")
    with pytest.raises(SystemExit) as exit_info:
        measure.fresh_processes([child("p", path), bad, child("t", path)], 2, timeout_s=60)
    assert exit_info.value.code not in (0, None)
    assert started(path) == ["p", "bad"]                      # round 1 ended at `bad`; `t` and round 2 never started
    err = capfd.readouterr().err
    assert "bad: exit status 3" in err and "it broke" in err


def test_fresh_processes_time_limit(tmp_path, capfd):
    path = str(tmp_path / "log")
    slow = child("slow", path, then="import time\ntime.sleep(60)")
    with pytest.raises(SystemExit):
        measure.fresh_processes([slow, child("t", path)], 1, timeout_s=1)
    assert started(path) == ["slow"]
    err = capfd.readouterr().err
    assert "slow: exit status 124" in err and "timed out" in err


# ---- every GPU-timing tool ends with one line where there is no device ---------------------------------------------
# an explicit list: the tools that need no GPU (emd_model, gen_svm_golden, cpu_baselines, tune_gemm_offline,
# pin_large_groups) would do real work.  {root}: this tree, as the "parent" of the process drivers; their children
# are the ones that refuse, and the driver passes the sentence on.
GPU_TOOLS = [
    "bench_augment.py", "bench_chamfer.py", "bench_chamfer.py --ragged --runs 1", "bench_conv_bwd.py",
    "bench_conv_bwd.py --unaligned", "bench_cross_merge.py", "bench_deterministic.py", "bench_dt_fusion.py",
    "bench_emd.py", "bench_encoder.py", "bench_graphed_dp.py --parent {root} --out {tmp}/graphed_dp.json --rounds 1",
    "bench_in_proj.py", "bench_large_groups.py", "bench_loader.py --skip-train", "bench_mae.py", "bench_out_norm.py",
    "bench_ragged_clouds.py", "bench_rms_norm.py", "bench_scan.py", "bench_scan_context.py", "bench_seg.py",
    "bench_seg_eval.py", "bench_sinkhorn.py", "bench_spectral.py", "bench_svm.py", "bench_sync_bn.py",
    "bench_wgrad_splitk.py", "bench_wgrad_sum.py", "bench_xdt.py", "bf16x3_probe.py", "cpu_enqueue_time.py",
    "dev_bwd_seq.py", "overlap_probe.py", "overlap_probe2.py", "profile_layer.py", "tune_gemm.py",
    "tune_gemm_compact.py tune 56 {tmp}/tune.csv",
]


@pytest.fixture(scope="module")
def tool_runs(tmp_path_factory):
    """Every tool of GPU_TOOLS run once, eight at a time (they only import and refuse): command -> CompletedProcess."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a ROCm device is present: the tools would run")
    tmp = str(tmp_path_factory.mktemp("tools"))

    def run(cmd):
        name, *args = cmd.format(root=ROOT, tmp=tmp).split()
        return subprocess.run([sys.executable, os.path.join(ROOT, "tools", name)] + args, capture_output=True,
                              text=True, cwd=tmp, timeout=600)
    with ThreadPoolExecutor(8) as pool:
        return dict(zip(GPU_TOOLS, pool.map(run, GPU_TOOLS)))


@pytest.mark.parametrize("cmd", GPU_TOOLS)
def test_gpu_tool_refuses_without_a_device(tool_runs, cmd):
    p = tool_runs[cmd]
    assert p.returncode != 0
    assert "needs a ROCm device: a time from anything else says nothing" in p.stderr
    assert "Traceback" not in p.stderr


# ---- on the device: every timer returns a time ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def adds(device):
    import torch
    x, y = torch.ones(1 << 20, device=device), torch.ones(1 << 18, device=device)
    return {"add_2^20": lambda: torch.add(x, x), "add_2^18": lambda: torch.add(y, y)}


def is_time(t):
    return isinstance(t, float) and math.isfinite(t) and t > 0


@pytest.mark.gpu
def test_gpu_window_calls_per_call_median(adds):
    import torch
    for fn in adds.values():
        assert is_time(measure.window(fn, 10))
        assert is_time(measure.window(fn, 10, torch.cuda.current_stream()))
        assert is_time(measure.calls(fn, warmup=2, reps=10))
        assert is_time(measure.per_call_median(fn, warmup=2, reps=5))


@pytest.mark.gpu
def test_gpu_alternate(adds):
    reps = []

    def logged(fn, n):
        reps.append(n)
        return measure.window(fn, n)
    got = measure.alternate(adds, target_ms=5, windows=3, window=logged)
    assert list(got) == list(adds)
    assert all(len(v) == 3 and all(is_time(t) for t in v) for v in got.values())
    assert all(1 <= n <= 2000 for n in reps)


@pytest.mark.gpu
def test_gpu_host_clock(adds):
    for fn in adds.values():
        assert is_time(measure.host_clock(fn, steps=5, warmup=1))


@pytest.mark.gpu
def test_gpu_require_gpu_passes(device):
    measure.require_gpu("test_tools_measure.py")
