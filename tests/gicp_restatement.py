"""TEST INFRASTRUCTURE: ctypes front of the CPU restatement of CRegistration::gicp_reg (tests/cpp/gicp_cpu.cpp).
Built on first use with g++ -O2 -ffp-contract=off into tests/cpp/_build/ against the CPU oracle (oracle/libghicp_oracle.so)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpp", "gicp_cpu.cpp")
OUT = os.path.join(HERE, "cpp", "_build")
LIB = os.path.join(OUT, "libgicp_cpu.so")
_lib = None


class GicpParams(C.Structure):
    """Layout of ghicp_gicp_params (include/ghicp_c.h)."""
    _fields_ = [("max_iter", C.c_int32), ("use_reciprocal", C.c_int32), ("use_trimmed", C.c_int32), ("covariance_k", C.c_int32),
                ("thre_dis", C.c_float), ("min_overlap", C.c_float), ("max_inner_iter", C.c_int32), ("pad_", C.c_int32),
                ("max_correspondence_distance", C.c_double), ("gicp_epsilon", C.c_double), ("transformation_epsilon", C.c_double),
                ("rotation_epsilon", C.c_double)]


class Stats(C.Structure):
    _fields_ = [("done", C.c_int32), ("iterations", C.c_int32), ("converged", C.c_int32), ("reason", C.c_int32),
                ("correspondences", C.c_int64), ("overlap", C.c_float), ("pad_", C.c_float), ("mse", C.c_double), ("fitness", C.c_double)]


def params(max_iter=50, reciprocal=False, trimmed=False, thre_dis=0.5, min_overlap=0.1, covariance_k=20, max_correspondence_distance=1e6,
           max_inner_iter=20):
    """gicp_reg's arguments and the constants of common_reg.cpp:253-265 (gicp_epsilon 1e-3, 1e-8 / 1e-6)."""
    return GicpParams(max_iter, int(reciprocal), int(trimmed), covariance_k, thre_dis, min_overlap, max_inner_iter, 0,
                      max_correspondence_distance, 1e-3, 1e-8, 1e-6)


def lib(oracle):
    global _lib
    if _lib is None:
        oracle.build()
        odir = os.path.join(ROOT, "oracle")
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(os.path.join(odir, "libghicp_oracle.so"))):
            os.makedirs(OUT, exist_ok=True)
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-w",
                                   "-I", os.path.join(HERE, "hipsim", "include"), "-I", os.path.join(ROOT, "gh-icp_amd", "csrc"),
                                   SRC, "-o", LIB + ".tmp", "-L", odir, "-l:libghicp_oracle.so", "-Wl,-rpath,$ORIGIN/../../../oracle"])
            os.replace(LIB + ".tmp", LIB)
        _lib = C.CDLL(LIB)
    return _lib


def _f32(x):
    return np.ascontiguousarray(np.asarray(x)[:, :3], np.float32)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def covariances(oracle, xyz, k, eps=1e-3):
    x = _f32(xyz)
    out = np.zeros((x.shape[0], 6), np.float64)
    lib(oracle).gcpu_covariances(_p(x, C.c_float), x.shape[0], 3, int(k), C.c_double(eps), _p(out, C.c_double))
    return out


def correspondences(oracle, src, tgt, covS, covT, T, max_dist=1e6):
    """One outer iteration's correspondence set under T: (source indices, target indices, M (c, 6))."""
    s, t = _f32(src), _f32(tgt)
    T = np.ascontiguousarray(T, np.float32)
    si = np.zeros(s.shape[0], np.int32)
    tj = np.zeros(s.shape[0], np.int32)
    M = np.zeros((s.shape[0], 6), np.float64)
    c = lib(oracle).gcpu_correspondences(_p(s, C.c_float), s.shape[0], 3, _p(t, C.c_float), t.shape[0], 3, _p(np.ascontiguousarray(covS), C.c_double),
                                         _p(np.ascontiguousarray(covT), C.c_double), _p(T, C.c_float), C.c_double(max_dist * max_dist),
                                         _p(si, C.c_int), _p(tj, C.c_int), _p(M, C.c_double))
    return si[:c].copy(), tj[:c].copy(), M[:c].copy()


def gn_sums(oracle, src, tgt, si, tj, M, x):
    """(H (6, 6), g (6), e): J^T M J, J^T M r, r^T M r at x, summed in source order without rounding."""
    s, t = _f32(src), _f32(tgt)
    si, tj, M = np.ascontiguousarray(si, np.int32), np.ascontiguousarray(tj, np.int32), np.ascontiguousarray(M, np.float64)
    x = np.ascontiguousarray(x, np.float64)
    H21, g, e = np.zeros(21), np.zeros(6), C.c_double(0)
    lib(oracle).gcpu_gn_sums(_p(s, C.c_float), 3, _p(t, C.c_float), 3, len(si), _p(si, C.c_int), _p(tj, C.c_int), _p(M, C.c_double),
                             _p(x, C.c_double), _p(H21, C.c_double), _p(g, C.c_double), C.byref(e))
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = H21
    H = H + np.triu(H, 1).T
    return H, g, e.value


def gicp(oracle, src, tgt, prm: GicpParams):
    """gicp_reg on the CPU.  dict(done, T (4,4) f32, transformed, stats fields, inner (steps per iteration))."""
    s, t = _f32(src), _f32(tgt)
    T = np.zeros(16, np.float32)
    out = np.zeros((s.shape[0], 3), np.float32)
    st = Stats()
    inner = np.zeros(max(prm.max_iter, 1), np.int32)
    done = lib(oracle).gcpu_gicp(_p(s, C.c_float), s.shape[0], 3, _p(t, C.c_float), t.shape[0], 3, C.byref(prm), _p(T, C.c_float),
                                 _p(out, C.c_float), C.byref(st), _p(inner, C.c_int))
    d = {k: getattr(st, k) for k, _ in Stats._fields_ if k != "pad_"}
    d.update(done=int(done), T=T.reshape(4, 4), transformed=out, inner=inner[:st.iterations].copy())
    return d
