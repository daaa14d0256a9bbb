"""CPU-only checks around the compact LDS layout of the Kuhn-Munkres solver: its size, the planning of a batch (through the host SIMT
interpreter's build of the library: the plan is host code), that the test matrices reach the solver paths the layout touches, and the GPU tests of
tests/test_gpu_km4_compact.py on the interpreter in its three lane orders."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import km4_compact_cases as K  # noqa: E402


@pytest.fixture(scope="module")
def simlib():
    from hipsim import build

    lib = C.CDLL(build.build())
    lib.ghicp_km4_lds_bytes.restype = C.c_int64
    return lib


def _plan(lib, ns, compact=1):
    n = np.asarray(ns, np.int32)
    per_cu = np.zeros(len(n), np.int32)
    lds = np.zeros(8, np.int64)
    nc = C.c_int32(0)
    rc = lib.ghicp_km4_plan_probe(n.ctypes.data_as(C.c_void_p), C.c_int32(len(n)), C.c_int32(compact), per_cu.ctypes.data_as(C.c_void_p),
                                  lds.ctypes.data_as(C.c_void_p), C.byref(nc))
    assert rc == 0
    return nc.value, per_cu.tolist(), lds[: nc.value].tolist()


def test_compact_layout_fits_a_quarter_of_the_cu(simlib):
    assert simlib.ghicp_km4_lds_bytes(1131, 1) <= 40960 < simlib.ghicp_km4_lds_bytes(1132, 1)
    assert simlib.ghicp_km4_lds_bytes(924, 0) <= 40960 < simlib.ghicp_km4_lds_bytes(925, 0)
    assert simlib.ghicp_km4_lds_bytes(1131, 0) == 50049  # the standard layout is what it was


def test_plan_one_class_up_to_the_compact_limit(simlib):
    nc, per_cu, lds = _plan(simlib, [351, 924, 925, 1131])
    assert nc == 1 and per_cu == [4, 4, 4, 4] and lds[0] <= 40960
    assert lds[0] >= simlib.ghicp_km4_lds_bytes(924, 0)  # n = 924 keeps the standard layout: the slot must hold it
    # switched off (GHICP_KM_COMPACT=0): the two classes of before
    nc, per_cu, lds = _plan(simlib, [351, 924, 925, 1131], compact=0)
    assert nc == 2 and per_cu == [4, 4, 3, 3] and lds[0] == 50049


def test_plan_keeps_the_three_per_cu_class_beyond_the_limit(simlib):
    nc, per_cu, lds = _plan(simlib, [1131, 1200])
    assert nc == 2 and per_cu == [4, 3] and lds[0] == simlib.ghicp_km4_lds_bytes(1200, 0) and lds[1] <= 40960
    nc, per_cu, _ = _plan(simlib, [1132, 3000, 100])
    assert nc == 3 and per_cu == [3, 1, 4]


def _row_kinds(oracle, w):
    """Hint rows and pool rows from the model's own statistics: `overflow_rows` counts, over all list rebuilds, the rows with more tight
    entries than the list cap.  At cap 3 (the kernel's) those are the flagged rows; at cap 6 the rows with more than six, i.e. the pool
    rows; the difference is the rows with 4..6, which keep hints.  The cap changes no visited set (a failed phase visits the reference's
    reachable set, rule R3), so both runs rebuild the same rows at the same labels: checked through `failed` and `rebuild_rows`."""
    m3, s3 = oracle.km4_model(w, cap=3, hint=6, exact_rest=True, seed=True, lazy=True)
    m6, s6 = oracle.km4_model(w, cap=6, hint=0, exact_rest=True, seed=True, lazy=True)
    assert m3 is not None and m6 is not None and np.array_equal(m3, m6)
    assert (s3["failed"], s3["rebuild_rows"]) == (s6["failed"], s6["rebuild_rows"])
    return s3, s3["overflow_rows"] - s6["overflow_rows"], s6["overflow_rows"]


def test_the_families_reach_flagged_hint_and_pool_rows(oracle):
    """What the matrices are for, checked on the rule-level model (oracle/km4_model.inc) for every n >= 31 (n <= 3 solves without a failed
    phase in both families).  Tie family: hint rows AND pool rows at rebuilds (n = 31: 184 and 249, n = 257: 13 227 and 15 226), failed phases
    with seeded floods (27 .. 231), S rounds and steps back of the search (34 .. 2929 pops).  Random family: failed phases (23 .. 409), list
    rebuilds (81 .. 12 728 rows: the re-validation and the global CSR offsets), seeded floods and S rounds at every such n, hint rows from
    n = 32 on (4 .. 390) -- and NEVER a pool row or a step back: those paths are the tie family's alone."""
    for fam, n, w in K.cases():
        if n < 31:
            continue
        st, hint_rows, pool_rows = _row_kinds(oracle, w)
        assert st["failed"] > 0 and st["seeded"] > 0 and st["rebuild_rows"] > 0 and st["pull_rounds"] > 0, (fam, n, st)
        if fam == "ties":
            top = w.max(axis=1)
            assert {3, 4, 6, 7, 9} <= set((w == top[:, None]).sum(axis=1).tolist()), n
            assert hint_rows > 0 and pool_rows > 0 and st["dfs_pops"] > 0, (n, hint_rows, pool_rows, st)
        else:
            assert pool_rows == 0 and st["dfs_pops"] == 0, (n, pool_rows, st)
            assert hint_rows > 0 or n == 31, (n, hint_rows)


@pytest.mark.parametrize("order", ["ascending", "reverse", "random:7"])
def test_compact_layout_on_the_host_simt_interpreter(order):
    from hipsim import build

    build.build()
    env = dict(os.environ, GHICP_SIM="1", HIPSIM_ORDER=order, HIPSIM_THREADS="2", HIPSIM_SEGV_TRACE="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_km4_compact.py"), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "4 passed" in r.stdout, (r.stdout + r.stderr)[-3000:]
