"""CPU-suite companion of tests/test_gpu_loop_fused.py: the same cases on the host SIMT interpreter (the library's own pair_loop.hip and loop.hip compiled
for the host), in two lane orders -- the fused stages of the persistent pair loop against its three passes of before, bit for bit."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


@pytest.mark.parametrize("order", ["ascending", "reverse"])
def test_fused_pair_loop_on_the_host_simt_interpreter(order):
    from hipsim import build

    build.build()
    env = dict(os.environ, GHICP_SIM="1", HIPSIM_ORDER=order, HIPSIM_THREADS="2", HIPSIM_SEGV_TRACE="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_loop_fused.py"), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "13 passed" in r.stdout, (r.stdout + r.stderr)[-3000:]
