"""TEST INFRASTRUCTURE: ctypes front of the CPU restatement of the generalized ICP that applies the trimmed rejector
(tests/cpp/gicp_trimmed_cpu.cpp, which includes tests/cpp/gicp_cpu.cpp).  Built on first use like gicp_restatement.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import gicp_restatement as G

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpp", "gicp_trimmed_cpu.cpp")
LIB = os.path.join(G.OUT, "libgicp_trimmed_cpu.so")
_lib = None


def lib(oracle):
    global _lib
    if _lib is None:
        oracle.build()
        odir = os.path.join(ROOT, "oracle")
        deps = [SRC, G.SRC, os.path.join(odir, "libghicp_oracle.so")]
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(G.OUT, exist_ok=True)
            tmp = "%s.%d.tmp" % (LIB, os.getpid())
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-w",
                                   "-I", os.path.join(HERE, "hipsim", "include"), "-I", os.path.join(ROOT, "gh-icp_amd", "csrc"),
                                   SRC, "-o", tmp, "-L", odir, "-l:libghicp_oracle.so", "-Wl,-rpath,$ORIGIN/../../../oracle"])
            os.replace(tmp, LIB)
        _lib = C.CDLL(LIB)
    return _lib


def gicp_trimmed(oracle, src, tgt, prm: G.GicpParams, trim_ratio, guess=None):
    """The trimmed loop on the CPU.  dict(done, T (4,4) f32, transformed, stats fields).  guess: (4,4) or None."""
    s, t = G._f32(src), G._f32(tgt)
    T = np.zeros(16, np.float32)
    out = np.zeros((s.shape[0], 3), np.float32)
    st = G.Stats()
    g = None if guess is None else np.ascontiguousarray(guess, np.float32).reshape(16)
    done = lib(oracle).gcpu_gicp_trimmed(G._p(s, C.c_float), s.shape[0], 3, G._p(t, C.c_float), t.shape[0], 3, C.byref(prm),
                                         None if g is None else G._p(g, C.c_float), C.c_float(trim_ratio), G._p(T, C.c_float),
                                         G._p(out, C.c_float), C.byref(st))
    d = {k: getattr(st, k) for k, _ in G.Stats._fields_ if k != "pad_"}
    d.update(done=int(done), T=T.reshape(4, 4), transformed=out)
    return d
