"""CPU-suite companion of tests/test_gpu_km4_uniform.py: that the families reach the solver paths they are for (on the rule-level model),
and the same tests on the host SIMT interpreter in its three lane orders.  The interpreter takes k4_uni from the lowest lane, as the
hardware does; the orders change when that lane's loads run relative to the other lanes' stores (a scalar copy taken before the store it
depends on shows as a matching that depends on the order)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import km4_uniform_cases as U  # noqa: E402


def test_the_families_reach_their_paths(oracle):
    seen = set()
    for fam, n, w in U.cases():
        m, st = oracle.km4_model(w, cap=3, hint=6, exact_rest=True, seed=True, lazy=True)
        assert m is not None and np.array_equal(m, oracle.km(w)[0]), (fam, n)
        seen.add(fam)
        if fam == "step_back":
            # the first step back is where S is computed (lazy) and the stack is cut instead of popped: pull rounds and unwound frames
            assert st["pull_rounds"] > 0 and st["lazy_unwound"] > 0 and st["failed"] > 0, (n, st)
        if fam == "identity":
            assert st["dfs_pops"] == 0 and st["failed"] == 0, (n, st)  # every root matches at once
        if fam == "background":
            assert st["failed"] == 0 and (w == w[0, 0]).all(), n  # no explicit entry, no relabelling: the march alone
        if fam == "counts":
            top = w.max(axis=1)
            assert set((w == top[:, None]).sum(axis=1).tolist()) == {3, 4, 6, 7}, n
            assert st["failed"] > 0 and st["pull_rounds"] > 0, (n, st)
    assert seen == {"kat", "step_back", "identity", "random", "ties", "counts", "background"}


@pytest.mark.parametrize("order", ["ascending", "reverse", "random:7"])
def test_uniform_state_on_the_host_simt_interpreter(order):
    from hipsim import build

    build.build()
    env = dict(os.environ, GHICP_SIM="1", HIPSIM_ORDER=order, HIPSIM_THREADS="2", HIPSIM_SEGV_TRACE="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_km4_uniform.py"), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "3 passed" in r.stdout, (r.stdout + r.stderr)[-3000:]
