"""Matrices for the tests of the compact LDS layout of the Kuhn-Munkres solver (km4_dev.h): shared by tests/test_gpu_km4_compact.py
(MI355X) and, through it, tests/test_km4_compact_cpu.py (the same tests on the host SIMT interpreter)."""
import numpy as np

SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 257]  # bitset-word and wave edges, one n above the workgroup's 256 threads


def random_family(rng, n):
    """Sparse explicit entries over a background: the family of test_gpu_loop.py::test_km_kat_and_random."""
    frac = min(0.5, 6.0 / max(n, 1))
    cd = 5 + 60 * rng.random((n, n))
    cd[np.arange(n), (np.arange(n) * 7) % n] = 3 * rng.random(n)
    cd = np.where(rng.random((n, n)) < frac, 8 * rng.random((n, n)), cd)
    return np.where(cd < 8.0, -cd, -8.0)


def tie_family(rng, n):
    """Tie-heavy: row i shares its maximum weight among exactly k explicit entries, k cycling through 3, 4, 6, 7, 9 -- a listed row, rows that
    keep hints (4..6 tight entries) and rows that go to the pool (more than 6), by construction at the first rebuild -- and all those entries
    fall into the first third of the columns, so most roots find their tight columns taken: failed phases, relabellings by lattice steps
    (every weight is a multiple of 0.25: ties survive them), revalidation of the rows that were not visited, seeded floods."""
    w = np.full((n, n), -8.0)
    hot = max(1, n // 3)
    for i in range(n):
        k = min((3, 4, 6, 7, 9)[i % 5], n)
        top = -0.25 * float(rng.integers(1, 4))
        cols = rng.choice(n, size=k, replace=False) if k > hot else rng.choice(hot, size=k, replace=False)
        w[i, cols] = top
        extra = rng.choice(n, size=min(n, 4), replace=False)  # some lower explicit entries: they become tight after relabellings
        for c in extra:
            if w[i, c] == -8.0:
                w[i, c] = top - 0.25 * float(rng.integers(1, 8))
    return w


def cases():
    rng = np.random.default_rng(20261017)
    out = []
    for n in SIZES:
        out.append(("random", n, random_family(rng, n)))
        out.append(("ties", n, tie_family(rng, n)))
    return out
