"""The brute-force FPFH restatement (tests/fpfh_restatement.py) is proved against the oracle before the GPU test trusts it; no GPU involved.

On every cloud of tests/fpfh_edge_cases.py, brute-force k-NN -> SPFH (with the oracle's normals) -> weighting equals `oracle.fpfh`'s histograms
bit for bit.  The two share no search code (all-pairs distances and a stable sort here, ring expansion over a grid there), so a neighbour that
the ring expansion lost, a tie broken the other way or a skip rule applied differently shows as a differing row.  The closed-form anchor
needs neither: on a plane lattice every row is exactly 100 in bins 5, 16 and 27.  The cases are also shown to reach the code paths they are
named for, and the rows on which the GPU test compares normals with numpy's eigh are counted here, with the oracle's normals."""
import numpy as np
import pytest

import fpfh_edge_cases as E
import fpfh_restatement as R

U = np.uint32


@pytest.fixture(scope="module")
def clouds(synth, oracle):
    cache = {}

    def get(name):
        if name not in cache:
            p = E.build(name, synth, oracle.voxel_filter)
            nrm, hist = oracle.fpfh(p)
            nn, nd, nk = R.knn_brute(p)
            cache[name] = dict(p=p, nrm=nrm, hist=hist, nn=nn, nd=nd, nk=nk)
        return cache[name]

    return get


@pytest.mark.parametrize("name", E.NAMES)
def test_restatement_equals_oracle(clouds, oracle, name):
    c = clouds(name)
    p, m = c["p"], c["p"].shape[0]
    assert m <= 3000
    ref = R.fpfh(c["nn"], c["nd"], c["nk"], R.spfh(p, c["nrm"], c["nn"], c["nk"], oracle.atan2f))
    assert ref.shape == c["hist"].shape == (m, 33) and ref.dtype == np.float32
    np.testing.assert_array_equal(np.isnan(ref), np.isnan(c["hist"]))
    np.testing.assert_array_equal(ref.view(U), c["hist"].view(U))
    # rows of 4 floats are the same cloud to the oracle too
    n4, h4 = oracle.fpfh(E.rows4(p))
    np.testing.assert_array_equal(h4.view(U), c["hist"].view(U))
    np.testing.assert_array_equal(n4.view(U), c["nrm"].view(U))
    # what PCL guarantees of a row: finite, every 11-bin block sums to 100 or is empty
    assert np.isfinite(c["hist"]).all() and np.isfinite(c["nrm"]).all()
    blocks = c["hist"].reshape(m, 3, 11)
    assert ((np.abs(blocks.sum(2) - 100.0) < 1e-3) | (blocks == 0).all(2)).all()


@pytest.mark.parametrize("name", E.PLANES)
def test_plane_lattice_closed_form(clouds, name):
    """normal = the axis (towards the origin), f1 = f2 = f3 = +-0 for every pair: all of a block's mass in its middle bin, and
    F * (100 / s) with F == s is exactly 100 here"""
    c = clouds(name)
    axis = E.PLANES.index(name)
    want = np.zeros(3, np.float32)
    want[axis] = -1.0
    np.testing.assert_array_equal(c["nrm"], np.tile(want, (1600, 1)))  # -0.0 == 0.0
    np.testing.assert_array_equal(c["hist"], np.tile(E.plane_row(), (1600, 1)))


def test_cases_reach_their_code_paths(clouds, oracle):
    def stats(name):
        c, st = clouds(name), {}
        R.spfh(c["p"], c["nrm"], c["nn"], c["nk"], oracle.atan2f, st)
        return c, st

    for mm in E.SMALL_M:
        assert clouds("small_%d" % mm)["nk"] == min(20, mm)
    c, st = stats("small_1")
    assert st["pairs"] == 0 and st["self"] == 1 and not c["hist"].any()  # incr = 100 / 0 is never added
    c, st = stats("dup_twice")
    assert st["f4"] == 1200  # every point meets its twin: f4 == 0, and d == 0 in the weighting
    assert ((c["nd"] == 0).sum(1) == 2).all()
    c, st = stats("dup_25")
    rep = (c["nd"] == 0).all(1)
    assert rep.sum() == 25 and not c["hist"][rep].any() and c["hist"][~rep].any(1).mean() > 0.9  # all-zero rows: s == 0 in all three blocks
    assert (c["nn"][rep] != np.flatnonzero(rep)[:, None]).all(1).sum() == 5  # five of them are not in their own list
    c, st = stats("identical")
    assert st["pairs"] == 0 and st["self"] == 20 and not c["hist"].any()
    c, st = stats("lattice")
    assert st["vn"] > 1000  # a neighbour along the normal: v = dp x n vanishes
    d2 = np.sort(((c["p"][:, None, :] - c["p"][None, :, :]) ** 2).sum(2), axis=1)
    assert (d2[:, 19] == d2[:, 20]).mean() > 0.9  # exact ties at the k-th distance
    assert st["clamp"] > 100  # features of exactly 1 (f2 between axis normals) and pi (opposite normals): bin index 11 before the clamp
    for a in E.AXES:  # rank 1: the normal is perpendicular to every connecting line, f2 = f3 = 0 as on a plane
        c, st = stats("line_" + a)
        assert st["pairs"] == 9500 and st["switch"] == 0
    cell, dim = E.grid_dims(clouds("clusters")["p"])
    assert max(dim) > 256  # the widened cell of grid.h, and > 1000 empty shells between the clusters
    cell, dim = E.grid_dims(clouds("tiny")["p"])
    assert cell == np.float32(0.05) and dim == [1, 1, 1]
    cell, dim = E.grid_dims(clouds("faces")["p"])
    assert cell == np.float32(0.05) and dim[0] >= E.FACE_DIMS[0]
    assert sum(stats(n)[1]["switch"] > 0 for n in E.NAMES if clouds(n)["p"].shape[0] > 21) > 15  # the role switch is everywhere


@pytest.mark.parametrize("name", [n for n in E.NAMES if n not in E.NORMAL_EXEMPT])
def test_normal_filter_keeps_enough_rows(clouds, name):
    c = clouds(name)
    n64, lam = R.normals_f64(c["p"], c["nn"], c["nk"])
    keep = R.normal_filter(c["p"], n64, lam)
    assert keep.mean() >= E.KEEP_FLOOR.get(name, 0.9), keep.mean()
    cos = (n64 * c["nrm"]).sum(1)[keep]
    assert (cos >= 1.0 - 1e-6).all(), cos.min()  # same line within 1e-6 and the same orientation


@pytest.mark.parametrize("ks,kt", E.FD_SHAPES)
def test_fd_restatement_equals_oracle(oracle, ks, kt):
    hS, hT = E.fd_case(ks, kt)
    ref = R.fd_fpfh_ref(hS, hT)
    got = oracle.fd_fpfh(hS, hT).astype(np.float32)  # the oracle returns its float in a double
    np.testing.assert_array_equal(np.isnan(ref), np.isnan(got))
    ok = ~np.isnan(ref)
    np.testing.assert_array_equal(ref.view(U)[ok], got.view(U)[ok])
    if ks >= 63 and kt >= 63:
        assert np.isnan(ref).any() and ok.any()  # the rows without variance, and the others
        assert ref[2, 0] == 1.0 and ref[2, 1] == 1.0  # identical one-hot rows (S rows 2, 3 = T rows 0, 1)


def test_restatement_of_selected_rows(clouds, oracle):
    """fpfh_brute_rows (what the batched GPU test uses on clouds of 12 000 points) gives the rows of fpfh_brute"""
    c = clouds("natural")
    rows = np.array([2999, 0, 17, 17, 1500], np.int64)
    ref, nn, nd = R.fpfh_brute_rows(c["p"], c["nrm"], rows, atan2f=oracle.atan2f)
    np.testing.assert_array_equal(ref.view(U), c["hist"][rows].view(U))
    np.testing.assert_array_equal(nn, c["nn"][rows])
    np.testing.assert_array_equal(nd.view(U), c["nd"][rows].view(U))
