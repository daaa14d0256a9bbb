"""TEST INFRASTRUCTURE: ctypes front of the CPU restatement of CFilter's cleaning filters (tests/cpp/filters_cpu.cpp: SORFilter,
DisFilter, ActiveObjectFilter under DESIGN.md N9 / Q10 / Q11).  Built on first use with g++ -O2 -ffp-contract=off into tests/cpp/_build/."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "filters_cpu.cpp")
OUT = os.path.join(HERE, "cpp", "_build")
LIB = os.path.join(OUT, "libfilters_cpu.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
            os.makedirs(OUT, exist_ok=True)
            tmp = "%s.%d.tmp" % (LIB, os.getpid())
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-Wall", SRC, "-o", tmp])
            os.replace(tmp, LIB)
        _lib = C.CDLL(LIB)
        for f in ("fcpu_sor_filter", "fcpu_dis_filter", "fcpu_box_filter"):
            getattr(_lib, f).restype = C.c_longlong
    return _lib


def _cloud(xyz):
    x = np.ascontiguousarray(xyz, np.float32)
    assert x.ndim == 2 and x.shape[1] >= 3
    return x


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def knn_mean_distance(xyz, mean_k):
    x = _cloud(xyz)
    out = np.zeros(x.shape[0], np.float32)
    lib().fcpu_knn_mean_distance(_p(x, C.c_float), C.c_longlong(x.shape[0]), x.shape[1], int(mean_k), _p(out, C.c_float))
    return out


def knn_mean_distance_range(xyz, mean_k, i0, i1):
    """the distances of the queries [i0, i1) alone, against the whole cloud"""
    x = _cloud(xyz)
    out = np.zeros(i1 - i0, np.float32)
    lib().fcpu_knn_mean_distance_range(_p(x, C.c_float), C.c_longlong(x.shape[0]), x.shape[1], int(mean_k), C.c_longlong(i0), C.c_longlong(i1), _p(out, C.c_float))
    return out


def sor_stats(dist, std_mul, tiled=True):
    """(mean, stddev, threshold, valid count) of float distances: sums in PCL's sequential order, or in the order of N9."""
    d = np.ascontiguousarray(dist, np.float32)
    st = np.zeros(4)
    lib().fcpu_sor_stats(_p(d, C.c_float), C.c_longlong(d.size), C.c_double(std_mul), int(bool(tiled)), _p(st, C.c_double))
    return st


def sor_filter(xyz, mean_k, std_mul):
    """(kept indices int32, stats4 f64, distances f32)"""
    x = _cloud(xyz)
    n = x.shape[0]
    keep, st, dist = np.zeros(max(n, 1), np.int32), np.zeros(4), np.zeros(max(n, 1), np.float32)
    m = lib().fcpu_sor_filter(_p(x, C.c_float), C.c_longlong(n), x.shape[1], int(mean_k), C.c_double(std_mul), _p(keep, C.c_int32), _p(st, C.c_double),
                              _p(dist, C.c_float))
    return keep[:m].copy(), st, dist[:n].copy()


def dis_filter(xyz, xy_dis_max, z_min, z_max):
    x = _cloud(xyz)
    keep = np.zeros(max(x.shape[0], 1), np.int32)
    m = lib().fcpu_dis_filter(_p(x, C.c_float), C.c_longlong(x.shape[0]), x.shape[1], C.c_double(xy_dis_max), C.c_double(z_min), C.c_double(z_max),
                              _p(keep, C.c_int32))
    return keep[:m].copy()


def box_filter(xyz, boxes):
    x = _cloud(xyz)
    b = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1, 6))
    keep = np.zeros(max(x.shape[0], 1), np.int32)
    m = lib().fcpu_box_filter(_p(x, C.c_float), C.c_longlong(x.shape[0]), x.shape[1], _p(b, C.c_double), b.shape[0], _p(keep, C.c_int32))
    return keep[:m].copy()


# ---------------------------------------------------------------- inputs shared by tests/test_filters_cpu.py and tests/test_gpu_filters.py
@functools.lru_cache(maxsize=None)
def cube_with_outliers():
    """2 000 uniform points in the unit cube, then 40 points 5 to 10 units from its centre (shuffled into the cloud).
    Returns (cloud (2040, 3) f32, is_outlier (2040,) bool)."""
    rng = np.random.default_rng(20240607)
    cube = rng.random((2000, 3))
    v = rng.normal(size=(40, 3))
    far = 0.5 + v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(5.0, 10.0, (40, 1))
    pts = np.concatenate([cube, far]).astype(np.float32)
    out = np.arange(2040) >= 2000
    perm = rng.permutation(2040)
    pts, out = pts[perm], out[perm]
    pts.setflags(write=False)
    out.setflags(write=False)
    return pts, out


def dis_filter_case():
    """A cloud on which `x*x + y + y` and `x*x + y*y` decide differently in both directions (xy_dis_max = 3, -1 < z < 2)."""
    rng = np.random.default_rng(7)
    pts = rng.uniform(-4, 4, (600, 3)).astype(np.float32)
    pts[0] = (1.0, -50.0, 0.5)   # as written: 1 - 100 = -99 < 9 stays; a Euclidean test would drop it
    pts[1] = (0.5, 4.5, 0.5)     # as written: 0.25 + 9 = 9.25 >= 9 leaves; ...
    pts[2] = (0.5, 4.0, 0.5)     # 8.25 stays although x*x + y*y = 16.25
    pts[3] = (3.0, 0.0, 0.5)     # exactly 9: not smaller, leaves
    pts[4] = (0.0, 0.0, 2.0)     # z == z_max leaves
    pts[5] = (0.0, 0.0, -1.0)    # z == z_min leaves
    return pts
