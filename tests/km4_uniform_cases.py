"""Matrices for the tests of the Kuhn-Munkres solver's wave-uniform state (km4_dev.h: the search's row, stack pointer, scan pointer, label
and entry count and the flood's queue head and tail live in scalar registers): shared by tests/test_gpu_km4_uniform.py (MI355X) and,
through it, tests/test_km4_uniform_cpu.py (the same tests on the host SIMT interpreter).  Every family aims at one place where a value
that is NOT the same in every lane, taken from the first lane alone, would change the traversal."""
import numpy as np

import km4_compact_cases as K

BG = -8.0
SIZES = [63, 64, 65, 128, 129]  # window and ballot edges: one 64-column window less one, exactly one, one more; two, two and one


def kat():
    """km.cpp:237-259, the reference's own known-answer vector"""
    return np.array([[-5, -2, -100], [-4, -2, -6], [-100, -1, -7]], float)


def all_background(n):
    """Every row background-tight, no explicit entry: root r marches through the columns 0 .. r, whose owners share its label -- chains
    longer than one window, 64 picks in a window, the pick that ends a window's chain in lane 63."""
    return np.full((n, n), -2.5)


def identity(n):
    """Every root matches at once: one listed entry, its column free."""
    w = np.full((n, n), BG)
    w[np.arange(n), np.arange(n)] = -1.0
    return w


def step_back(n):
    """Blocks of three rows (3b, 3b+1, 3b+2) over the columns of the same numbers: row 3b is tight in column 3b alone, row 3b+1 in columns
    3b and 3b+2, row 3b+2 in column 3b+2 alone.  Root 3b+1 takes column 3b first, whose owner has nothing else: the search steps back on
    its FIRST step (S is computed with one frame on the stack) and goes on with column 3b+2; root 3b+2 then finds its only column taken, by
    a row whose other column leads nowhere: a failed phase, a relabelling, a seeded flood."""
    w = np.full((n, n), BG)
    for b in range(0, n - 2, 3):
        w[b, b] = -1.0
        w[b + 1, b] = -1.0
        w[b + 1, b + 2] = -1.0
        w[b + 2, b + 2] = -1.0
    for i in range(n - n % 3, n):
        w[i, i] = -1.0
    return w


def tight_counts(rng, n):
    """Rows with exactly 3, 4, 6 and 7 tight entries at the first rebuild (listed, hinted, hinted, pooled), in turn, all within the first
    third of the columns, weights on the 0.25 lattice so that the ties survive relabellings."""
    w = np.full((n, n), BG)
    hot = max(8, n // 3)
    for i in range(n):
        k = (3, 4, 6, 7)[i % 4]
        top = -0.25 * float(rng.integers(1, 4))
        w[i, rng.choice(hot, size=k, replace=False)] = top
        for c in rng.choice(n, size=4, replace=False):
            if w[i, c] == BG:
                w[i, c] = top - 0.25 * float(rng.integers(1, 8))
    return w


def cases():
    rng = np.random.default_rng(20261019)
    out = [("kat", 3, kat()), ("step_back", 5, step_back(5)), ("step_back", 65, step_back(65)), ("identity", 65, identity(65))]
    for n in SIZES:
        out.append(("random", n, K.random_family(rng, n)))
        out.append(("ties", n, K.tie_family(rng, n)))
        out.append(("counts", n, tight_counts(rng, n)))
        out.append(("background", n, all_background(n)))
    return out
