"""CPU checks of the restatement of CFilter's cleaning filters (tests/cpp/filters_cpu.cpp; reference include/filter.hpp:90-140 under
DESIGN.md N9 / Q10 / Q11) against independent code -- scipy's KD-tree in f64 for the statistical outlier filter, numpy for the two
cheap ones -- and the drop-in header's three methods compiled like a reference caller in both type modes."""
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial import cKDTree

import filters_restatement as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kdtree_mean_distance(xyz, mean_k):
    x = np.asarray(xyz, np.float64)[:, :3]
    d, _ = cKDTree(x).query(x, mean_k + 1)
    return d[:, 1:].reshape(len(x), mean_k).mean(axis=1)


def test_mean_distances_match_a_kdtree():
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(1500, 3)).astype(np.float32) * np.float32(4.0)
    for k in (1, 8, 50):
        got = F.knn_mean_distance(pts, k).astype(np.float64)
        np.testing.assert_allclose(got, kdtree_mean_distance(pts, k), rtol=1e-6, atol=0)
    # a stride of 8 floats reads the same points
    wide = np.zeros((1500, 8), np.float32)
    wide[:, :3] = pts
    wide[:, 3:] = 77.0
    np.testing.assert_array_equal(F.knn_mean_distance(wide, 8), F.knn_mean_distance(pts, 8))


def test_kept_set_on_the_cube_with_outliers():
    pts, is_out = F.cube_with_outliers()
    keep, st, dist = F.sor_filter(pts, 8, 1.0)
    ref = kdtree_mean_distance(pts, 8)
    mean, std = ref.mean(), ref.std(ddof=1)
    thr = mean + 1.0 * std
    np.testing.assert_allclose(st[:3], [mean, std, thr], rtol=1e-6)
    assert st[3] == len(pts)
    # margin: no distance within 1 % of the threshold, so float against f64 distances cannot flip a point
    assert np.abs(ref / thr - 1.0).min() >= 0.01 and np.abs(dist.astype(np.float64) / st[2] - 1.0).min() >= 0.01
    np.testing.assert_array_equal(keep, np.flatnonzero(~(ref > thr)).astype(np.int32))
    assert not np.isin(np.flatnonzero(is_out), keep).any()  # every one of the 40 leaves
    assert len(keep) >= 1500 and np.all(np.diff(keep) > 0)


def test_threshold_orders_agree():
    pts, _ = F.cube_with_outliers()
    rng = np.random.default_rng(11)
    for d in (F.knn_mean_distance(pts, 8), rng.random(1024 * 37 + 5).astype(np.float32), rng.random(1024).astype(np.float32)):
        a, b = F.sor_stats(d, 1.0, tiled=False), F.sor_stats(d, 1.0, tiled=True)
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
        x = d.astype(np.float64)
        np.testing.assert_allclose(b[:3], [x.mean(), x.std(ddof=1), x.mean() + x.std(ddof=1)], rtol=1e-9)


def test_sor_edges():
    pts, _ = F.cube_with_outliers()
    for n in (0, 1, 8):  # fewer than mean_k + 1 points: all kept, NaN statistics, no valid point
        keep, st, dist = F.sor_filter(pts[:n], 8, 1.0)
        np.testing.assert_array_equal(keep, np.arange(n, dtype=np.int32))
        assert np.isnan(st[:3]).all() and st[3] == 0 and not dist.any()
        assert not F.knn_mean_distance(pts[:n], 8).any()
    keep, st, _ = F.sor_filter(np.tile(pts[:1], (30, 1)), 8, 1.0)  # identical points: threshold 0, nothing is above it
    assert st.tolist() == [0.0, 0.0, 0.0, 30.0] and len(keep) == 30


def test_dis_filter_keeps_what_the_expression_as_written_keeps():
    pts = F.dis_filter_case()
    keep = F.dis_filter(pts, 3.0, -1.0, 2.0)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    written = ((x * x + y + y).astype(np.float64) < 9.0) & (z < 2.0) & (z > -1.0)  # float32 arithmetic, then the comparison in f64
    np.testing.assert_array_equal(keep, np.flatnonzero(written).astype(np.int32))
    euclid = ((x * x + y * y).astype(np.float64) < 9.0) & (z < 2.0) & (z > -1.0)
    assert written[0] and not euclid[0] and written[2] and not euclid[2] and (written != euclid).sum() > 10
    assert not written[1] and not written[3] and not written[4] and not written[5]


def test_box_filter_is_strict():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-2, 2, (500, 3)).astype(np.float32)
    pts[0] = (1.0, 0.5, 0.5)    # on the face x = max_x of box 0: stays
    pts[1] = (0.5, 0.5, 0.5)    # inside box 0
    pts[2] = (-1.5, -1.5, -1.5)  # inside box 1
    boxes = np.array([[0, 0, 0, 1, 1, 1], [-2, -2, -2, -1, -1, -1]], np.float64)
    keep = F.box_filter(pts, boxes)
    p = pts.astype(np.float64)
    inside = np.zeros(len(pts), bool)
    for b in boxes:
        inside |= np.all((p > b[:3]) & (p < b[3:]), axis=1)
    np.testing.assert_array_equal(keep, np.flatnonzero(~inside).astype(np.int32))
    assert 0 in keep and 1 not in keep and 2 not in keep and 0 < len(keep) < len(pts)
    np.testing.assert_array_equal(F.box_filter(pts, np.zeros((0, 6))), np.arange(len(pts), dtype=np.int32))
    assert len(F.box_filter(pts, [[-9, -9, -9, 9, 9, 9]])) == 0


def test_api_declares_the_filters(api):
    for name in ("ghicp_knn_mean_distance", "ghicp_sor_filter", "ghicp_dis_filter", "ghicp_box_filter"):
        assert name in api.EXPORTS
    for name in ("knn_mean_distance", "sor_filter", "dis_filter", "box_filter"):
        assert callable(getattr(api.Context, name))
    lib = os.path.join(ROOT, "gh-icp_amd", "libghicp_hip.so")
    if os.path.exists(lib):  # the argument checks come before any device work
        import ctypes

        L = api.load()
        for name in ("ghicp_knn_mean_distance", "ghicp_sor_filter", "ghicp_dis_filter", "ghicp_box_filter"):
            fn = getattr(L, name)
            fn.restype = ctypes.c_int
            assert fn(*([ctypes.c_void_p(0)] * 10)) == 1  # GHICP_ERR_ARG on a NULL context


@pytest.mark.parametrize("types", ["shim", "pcl-eigen-interface"])
def test_dropin_filters_compile(tmp_path, types):
    """A reference program calling CFilter<pcl::PointXYZ>::SORFilter / DisFilter / ActiveObjectFilter compiles (and, once the library
    is built, links) against the drop-in headers in both type modes."""
    extra = [] if types == "shim" else ["-DGHICP_WITH_PCL", "-I", os.path.join(ROOT, "oracle", "ref_stubs")]
    obj = str(tmp_path / "test_filters_dropin.o")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include")] + extra +
                          [os.path.join(ROOT, "tests", "cpp", "test_filters_dropin.cpp"), "-c", "-o", obj])
    lib = os.path.join(ROOT, "gh-icp_amd", "libghicp_hip.so")
    if os.path.exists(lib):
        subprocess.check_call(["g++", obj, "-L", os.path.dirname(lib), "-lghicp_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "test_filters_dropin")])
