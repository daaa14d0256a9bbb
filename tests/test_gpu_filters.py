"""GPU parity of CFilter's cleaning filters (reference include/filter.hpp:90-140; ghicp_knn_mean_distance, ghicp_sor_filter,
ghicp_dis_filter, ghicp_box_filter) against the CPU restatement (tests/cpp/filters_cpu.cpp).  Everything is
exact: the per-point distances and the four statistics bit for bit, the kept indices as arrays."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import filters_restatement as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_sor(ctx, pts, mean_k, std_mul=1.0, label=""):
    """knn_mean_distance and sor_filter of `pts` against the restatement; returns (kept, stats4)."""
    pts = np.array(pts, np.float32)  # (a writable copy: the shared inputs are read-only)
    keep_o, st_o, dist_o = F.sor_filter(pts, mean_k, std_mul)
    dist_g = ctx.knn_mean_distance(pts, mean_k).cpu().numpy()
    np.testing.assert_array_equal(dist_g.view(np.uint32), dist_o.view(np.uint32), err_msg="distances %s n=%d mean_k=%d" % (label, len(pts), mean_k))
    keep_g, st_g = ctx.sor_filter(pts, mean_k, std_mul)
    np.testing.assert_array_equal(_bits(st_g)[3:], _bits(st_o)[3:])
    if np.isnan(st_o[0]):
        assert np.isnan(st_g[:3]).all(), (label, st_g)
    else:
        np.testing.assert_array_equal(_bits(st_g), _bits(st_o), err_msg="stats %s n=%d mean_k=%d: %r / %r" % (label, len(pts), mean_k, st_g, st_o))
    np.testing.assert_array_equal(keep_g.cpu().numpy(), keep_o, err_msg="kept %s n=%d mean_k=%d" % (label, len(pts), mean_k))
    return keep_o, st_o


def _random_cloud(n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    pts = rng.normal(size=(n, 3)).astype(np.float32) * np.array([3.0, 2.0, 0.7], np.float32)
    return pts


@pytest.mark.parametrize("mean_k", [1, 8, 50, 63])
def test_sor_sizes(ctx, mean_k):
    """n = mean_k (no valid point: all kept, NaN statistics), mean_k + 1 (the whole cloud is every point's list), one wave of candidates,
    one more, several cells"""
    for n in (mean_k, mean_k + 1, 64, 65, 257):
        keep, st = check_sor(ctx, _random_cloud(n, n), mean_k, 1.0, "random")
        if n <= mean_k:
            assert len(keep) == n and st[3] == 0
        else:
            assert st[3] == n and 0 < len(keep) <= n


@pytest.mark.parametrize("mean_k", [1, 8, 50, 63])
def test_sor_three_thousand_points(ctx, mean_k):
    keep, st = check_sor(ctx, _random_cloud(2999, mean_k), mean_k, 1.5, "random")
    assert 2000 < len(keep) < 2999 and st[2] > st[0] > 0


@pytest.mark.parametrize("stride", [3, 4, 8])
def test_sor_strides(ctx, stride):
    pts = np.full((257, stride), 1e6, np.float32)  # the columns after z are never read
    pts[:, :3] = _random_cloud(257, 5)
    keep, _ = check_sor(ctx, pts, 8, 1.0, "stride %d" % stride)
    np.testing.assert_array_equal(keep, F.sor_filter(pts[:, :3], 8, 1.0)[0])


def test_sor_lattice_ties(ctx):
    """a 0.25-spaced lattice: the mean_k-th place is shared by many equal d2"""
    g = np.arange(12, dtype=np.float32) * np.float32(0.25)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    for mean_k in (8, 50):
        check_sor(ctx, pts, mean_k, 1.0, "lattice")


def test_sor_repeated_and_identical_points(ctx):
    base = _random_cloud(400, 9)
    tripled = np.repeat(base, 3, axis=0)  # entry 1 (and 2) of every list is 0
    for mean_k in (1, 8):
        _, st = check_sor(ctx, tripled, mean_k, 1.0, "tripled")
    d = ctx.knn_mean_distance(tripled, 2).cpu().numpy()
    assert not d.any()
    same = np.tile(base[:1], (300, 1))  # threshold 0, nothing above it
    keep, st = check_sor(ctx, same, 50, 1.0, "identical")
    assert st.tolist() == [0.0, 0.0, 0.0, 300.0] and len(keep) == 300


def test_sor_line_and_cluster(ctx):
    rng = np.random.default_rng(21)
    line = np.zeros((1000, 3), np.float32)  # the grid is one cell thick in y and z
    line[:, 0] = rng.uniform(0, 10, 1000).astype(np.float32)
    for mean_k in (8, 50):
        check_sor(ctx, line, mean_k, 1.0, "line")
    # 300 points inside one cell, 200 sparse ones cells away: their lists fill from far shells, ring after ring
    cluster = (np.float32(1.2) + rng.normal(size=(300, 3)) * 0.004).astype(np.float32)
    sparse = rng.uniform(0, 10, (200, 3)).astype(np.float32)
    pts = np.concatenate([cluster, sparse])[rng.permutation(500)]
    keep, _ = check_sor(ctx, pts, 50, 1.0, "cluster")
    assert 300 <= len(keep) < 500


def test_sor_cube_with_outliers(ctx):
    pts, is_out = F.cube_with_outliers()
    pts = np.array(pts)  # (writable: torch wraps host arrays)
    keep, st = check_sor(ctx, pts, 8, 1.0, "cube")
    np.testing.assert_array_equal(keep, np.flatnonzero(~is_out).astype(np.int32))  # exactly the 40 leave
    again_d = ctx.knn_mean_distance(pts, 8).cpu().numpy()  # determinism: two runs, the same bits
    again_k, again_s = ctx.sor_filter(pts, 8, 1.0)
    np.testing.assert_array_equal(again_d.view(np.uint32), F.sor_filter(pts, 8, 1.0)[2].view(np.uint32))
    np.testing.assert_array_equal(again_k.cpu().numpy(), keep)
    np.testing.assert_array_equal(_bits(again_s), _bits(st))


def test_sor_full_size_scan(ctx, oracle, synth):
    """20 000 points of a voxel-filtered terrestrial scan at the reference's usual MeanK = 50, std = 2"""
    p = synth.tls_pair(120_000, pair_id=3)
    ds = p.target[oracle.voxel_filter(p.target, 0.1)][:, :3]
    assert len(ds) >= 20_000
    keep, st = check_sor(ctx, np.ascontiguousarray(ds[:20_000]), 50, 2.0, "scan")
    assert 15_000 < len(keep) < 20_000


def test_dis_and_box_filters(ctx):
    pts = F.dis_filter_case()
    for args in ((3.0, -1.0, 2.0), (0.5, -10.0, 10.0), (3.0, 5.0, 6.0), (1e3, -1e3, 1e3)):
        np.testing.assert_array_equal(ctx.dis_filter(pts, *args).cpu().numpy(), F.dis_filter(pts, *args), err_msg=str(args))
    keep = ctx.dis_filter(pts, 3.0, -1.0, 2.0).cpu().numpy()
    assert 0 in keep and 2 in keep and not np.isin([1, 3, 4, 5], keep).any()  # `x*x + y + y`: the point at y = -50 stays
    assert len(ctx.dis_filter(pts, 3.0, 5.0, 6.0)) == 0  # no z in (5, 6): m = 0
    wide = np.zeros((len(pts), 8), np.float32)
    wide[:, :3] = pts
    np.testing.assert_array_equal(ctx.dis_filter(wide, 3.0, -1.0, 2.0).cpu().numpy(), keep)
    rng = np.random.default_rng(5)
    cloud = rng.uniform(-2, 2, (3001, 3)).astype(np.float32)
    cloud[0] = (1.0, 0.5, 0.5)   # on a face of box 0: stays
    cloud[1] = (0.5, 0.5, 0.5)   # strictly inside: leaves
    boxes = np.array([[0, 0, 0, 1, 1, 1], [-2, -2, -2, -1, -1, -1], [0.1, 0.1, 0.1, 0.1, 0.1, 0.1]], np.float64)
    for b in (boxes, boxes[:1], np.zeros((0, 6)), np.array([[-9.0, -9, -9, 9, 9, 9]])):
        np.testing.assert_array_equal(ctx.box_filter(cloud, b).cpu().numpy(), F.box_filter(cloud, b), err_msg=str(b))
    keep = ctx.box_filter(cloud, boxes).cpu().numpy()
    assert keep[0] == 0 and keep[1] != 1 and len(keep) < 3001
    assert len(ctx.box_filter(cloud, np.zeros((0, 6)))) == 3001 and len(ctx.box_filter(cloud, [[-9, -9, -9, 9, 9, 9]])) == 0
    assert len(ctx.box_filter(cloud[:0], boxes)) == 0 and len(ctx.dis_filter(cloud[:0], 1.0, 0.0, 1.0)) == 0 and len(ctx.sor_filter(cloud[:0], 8, 1.0)[0]) == 0


def test_filter_arguments(ctx, api):
    pts = _random_cloud(100, 1)
    for bad in (0, 64, -1):
        with pytest.raises(api.GhicpError, match="ghicp error 1"):
            ctx.knn_mean_distance(pts, bad)
        with pytest.raises(api.GhicpError, match="ghicp error 1"):
            ctx.sor_filter(pts, bad, 1.0)
    five = np.zeros((100, 5), np.float32)
    with pytest.raises(api.GhicpError, match="ghicp error 1"):
        ctx.sor_filter(five, 8, 1.0)
    check_sor(ctx, pts, 8, 1.0, "after the refusals")


def test_filters_in_host_pointer_mode(ctx):
    """what the drop-in classes use: the library stages the caller's host arrays"""
    lib = ctx.lib
    vp = ctypes.c_void_p
    h = vp()
    assert lib.ghicp_ctx_create(0, ctypes.byref(h)) == 0
    try:
        assert lib.ghicp_ctx_set_host_pointers(h, 1) == 0
        pts, _ = F.cube_with_outliers()
        pts = np.ascontiguousarray(pts)
        n = len(pts)
        keep_o, st_o, dist_o = F.sor_filter(pts, 8, 1.0)
        dist = np.zeros(n, np.float32)
        assert lib.ghicp_knn_mean_distance(h, pts.ctypes.data_as(vp), ctypes.c_int64(n), 3, 8, dist.ctypes.data_as(vp)) == 0
        np.testing.assert_array_equal(dist.view(np.uint32), dist_o.view(np.uint32))
        keep, m, st = np.full(n, -1, np.int32), ctypes.c_int64(-1), np.zeros(4)
        assert lib.ghicp_sor_filter(h, pts.ctypes.data_as(vp), ctypes.c_int64(n), 3, 8, ctypes.c_double(1.0), keep.ctypes.data_as(vp), ctypes.byref(m),
                                    st.ctypes.data_as(vp)) == 0
        np.testing.assert_array_equal(keep[: m.value], keep_o)
        np.testing.assert_array_equal(_bits(st), _bits(st_o))
        assert lib.ghicp_dis_filter(h, pts.ctypes.data_as(vp), ctypes.c_int64(n), 3, ctypes.c_double(1.0), ctypes.c_double(0.2), ctypes.c_double(0.9),
                                    keep.ctypes.data_as(vp), ctypes.byref(m)) == 0
        np.testing.assert_array_equal(keep[: m.value], F.dis_filter(pts, 1.0, 0.2, 0.9))
        box = np.array([0.0, 0, 0, 0.5, 0.5, 0.5])
        assert lib.ghicp_box_filter(h, pts.ctypes.data_as(vp), ctypes.c_int64(n), 3, box.ctypes.data_as(vp), 1, keep.ctypes.data_as(vp), ctypes.byref(m)) == 0
        np.testing.assert_array_equal(keep[: m.value], F.box_filter(pts, box))
    finally:
        lib.ghicp_ctx_destroy(h)


@pytest.mark.parametrize("types", ["shim", "pcl-eigen-interface"])
def test_filters_dropin_on_gpu(ctx, tmp_path, types):
    """tests/cpp/test_filters_dropin.cpp: CFilter<pcl::PointXYZ>::SORFilter / DisFilter / ActiveObjectFilter as a reference program calls
    them, in both type modes; the kept counts and the kept points' coordinate sums against the restatement."""
    exe = tmp_path / "test_filters_dropin"
    libdir, libname = os.path.join(ROOT, "gh-icp_amd"), "ghicp_hip"
    if getattr(ctx, "simulated", False):  # GHICP_SIM=1: the same C ABI from tests/hipsim
        libdir, libname = os.path.join(ROOT, "tests", "hipsim", "_build"), "ghicp_sim"
    extra = [] if types == "shim" else ["-DGHICP_WITH_PCL", "-I", os.path.join(ROOT, "oracle", "ref_stubs")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include")] + extra + [os.path.join(ROOT, "tests", "cpp", "test_filters_dropin.cpp"),
                           "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-o", str(exe)])
    pts, _ = F.cube_with_outliers()
    with open(tmp_path / "cloud.bin", "wb") as f:
        f.write(struct.pack("i", len(pts)))
        f.write(np.ascontiguousarray(pts, np.float32).tobytes())
    box = [0.0, 0.0, 0.0, 0.5, 0.5, 0.5]
    out = subprocess.run([str(exe), str(tmp_path / "cloud.bin"), "8", "1.0", "1.0", "0.2", "0.9"] + [repr(v) for v in box], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines() if l.split()}
    want = {"SOR": F.sor_filter(pts, 8, 1.0)[0], "DIS": F.dis_filter(pts, 1.0, 0.2, 0.9), "BOX": F.box_filter(pts, box)}
    for tag, keep in want.items():
        assert int(lines[tag][0]) == len(keep) and 0 < len(keep) < len(pts), tag
        sums = np.zeros(3)
        for i in keep:  # the program's own order of additions
            sums += pts[i].astype(np.float64)
        np.testing.assert_array_equal(np.array([float(v) for v in lines[tag + "SUM"]]), sums, err_msg=tag)
