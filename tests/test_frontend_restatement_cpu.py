"""The grid-free restatement (tests/frontend_restatement.py) pinned to the CPU oracle where the oracle is trusted: a natural scan of
moderate extent, where the oracle's own cell grid is far from every rounding margin."""
import numpy as np
import pytest

import frontend_restatement as FR


@pytest.fixture(scope="module")
def cloud(synth):
    return np.ascontiguousarray(synth.tls_pair(20_000).target)


def test_radius_counts_equal_the_oracles(oracle, cloud):
    _, _, no = oracle.pca(cloud, 0.5)
    np.testing.assert_array_equal(FR.radius_counts(cloud, 0.5), no)
    sub = np.array([0, 5, 19_999])
    np.testing.assert_array_equal(FR.radius_counts(cloud, 0.5, sub), no[sub])


def test_pca_reference_meets_the_eigenvalue_bound(oracle, cloud):
    """|lambda_oracle - lambda_ref| <= 2^-22 lambda1_ref: N2 rounds each scatter entry by at most 2^-23 max|S_ij| <= 2^-23 lambda1, a symmetric
    perturbation moves an eigenvalue by at most its Frobenius norm (<= 1.5 * 2^-23 lambda1), the final float rounding adds 2^-24 lambda1."""
    lo, co, no = oracle.pca(cloud, 0.5)
    lr, cr, nr = FR.pca_reference(cloud, 0.5)
    np.testing.assert_array_equal(nr, no)
    assert (no >= 3).sum() > 10_000
    err = np.abs(lo.astype(np.float64) - lr)
    assert (err <= 2.0 ** -22 * lr[:, :1]).all(), float((err / np.maximum(lr[:, :1], 1e-300)).max())
    assert not lr[no < 3].any() and not cr[no < 3].any()
    np.testing.assert_array_equal(FR.curvature_of(lo), co)  # the formula, from the oracle's own eigenvalues


def test_grid_regimes_counts_cells_and_blocks():
    """the transcription against a table small enough to count by hand: cell = 0.50005, points in cells x = 0, 1, 3 of a line"""
    x = np.zeros((7, 3), np.float32)
    x[:, 0] = [0.0, 0.1, 0.2, 0.6, 0.7, 1.6, 1.7]
    g = FR.grid_regimes(x, 0.5)
    assert g.dim.tolist() == [4, 1, 1] and not g.widened and g.coarsened == 0
    assert g.keys.tolist() == [0, 1, 3] and g.np.tolist() == [3, 2, 2] and g.total.tolist() == [5, 5, 2]
    assert g.g_first.tolist() == [16, 32, 32] and g.resident.all()
    assert [FR.lane_split(v) for v in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)] == [64, 32, 16, 16, 8, 8, 4, 4, 2, 2, 1, 1]
