import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run on the GPU box with -m gpu)")


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def on_fixture_cpu():
    """True on the kind of CPU the float fixtures were written on (golden/cpu_platform.json): there the CPU
    restatements reproduce them bit for bit."""
    import json
    from oracle.gen_golden import cpu_platform
    with open(os.path.join(GOLDEN, "cpu_platform.json")) as fh:
        return json.load(fh)["cpu"] == cpu_platform()


def assert_fixture_floats(actual, desired, rtol, atol):
    """Floats the CPU restatement computes, against a fixture: bit for bit on the fixture's kind of CPU; elsewhere MKL
    and torch's vector kernels round a few last bits differently, so within (rtol, atol)."""
    if on_fixture_cpu():
        np.testing.assert_array_equal(actual, desired)
    else:
        np.testing.assert_allclose(actual, desired, rtol=rtol, atol=atol)


@pytest.fixture(scope="session")
def device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda:0")
