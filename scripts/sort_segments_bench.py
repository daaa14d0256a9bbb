"""Times the segmented radix sort (prims.hip, ghicp_sort_segments) at the batched front end's sizes with digits of at most 8 and of at most 9 bits:
32 clouds of 1 M packed voxel keys (8-byte keys only, 34 key bits above 25 index bits: five places of 8 bits against 9 9 8 8) and 32 clouds of
225 k cell keys with values (4-byte, 25 bits: four places against 9 8 8).  Wall clock around ghicp_ctx_synchronize, median of 11 calls after a
warm-up; prints one JSON line.        usage: python scripts/sort_segments_bench.py [out.json]"""
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
api = importlib.import_module("gh-icp_amd.api")


def run(ctx, kb, nseg, per, bit_begin, bits, with_vals, width):
    t = ctx.torch
    n = nseg * per
    rng = np.random.default_rng(1)
    k = rng.integers(0, 1 << (bit_begin + bits), n, dtype=np.uint64)
    kd = t.from_numpy((k if kb == 8 else k.astype(np.uint32)).view(np.int64 if kb == 8 else np.int32)).to(ctx.dev)
    ko = t.empty_like(kd)
    vd = t.arange(n, dtype=t.int32, device=ctx.dev) if with_vals else None
    vo = t.empty_like(vd) if with_vals else None
    off = (ctypes.c_int64 * (nseg + 1))(*[i * per for i in range(nseg + 1)])
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    times = []
    for it in range(14):
        ctx.lib.ghicp_ctx_synchronize(ctx.h)
        t0 = time.perf_counter()
        rc = ctx.lib.ghicp_sort_segments(ctx.h, kb, p(kd), p(ko), p(vd), p(vo), ctypes.c_int32(nseg), off, None, bit_begin, bits, width)
        ctx.lib.ghicp_ctx_synchronize(ctx.h)
        times.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0
    return round(float(np.median(times[3:])), 4)


def main():
    ctx = api.Context(0)
    out = {"voxel_32x1M_u64_34bits_ms": {str(w): run(ctx, 8, 32, 1_000_000, 25, 34, False, w) for w in (8, 9, 8, 9)},
           "grid_32x225k_u32_25bits_ms": {str(w): run(ctx, 4, 32, 225_000, 0, 25, True, w) for w in (8, 9, 8, 9)},
           "voxel_32x1M_u64_32bits_ms": {str(w): run(ctx, 8, 32, 1_000_000, 25, 32, False, w) for w in (8, 9)}}
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
