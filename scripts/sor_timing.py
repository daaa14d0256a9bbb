"""The statistical outlier filter (ghicp_sor_filter, CFilter::SORFilter) on one RAW cfg2 cloud of 1 M points at the reference's usual
MeanK = 50, std = 2.  Prints one JSON line (and writes it to --out): the time of the k-NN stage (ghicp_knn_mean_distance: grid build +
k_sor_knn) and of the whole filter; as a yardstick the existing register-list k-NN (ghicp_knn_normals, k = 20: grid build + k_knn +
k_normals) against the new kernel at mean_k = 19 (20 list entries) on the same cloud; on the CPU of the same box the brute-force
restatement on a slice of the queries (extrapolated to the cloud: it is n^2 work) and scipy's KD-tree (16 workers) on all of them.
Every GPU figure: one warm-up call, then --reps calls, median / min / max of the wall time around call + synchronise."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--mean-k", type=int, default=50)
    ap.add_argument("--std", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-queries", type=int, default=1000, help="queries of the brute-force restatement (0: skip the CPU legs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sor_timing.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (api.load() wants torch's HIP runtime first)

    api = importlib.import_module("gh-icp_amd.api")
    synth = importlib.import_module("gh-icp_amd.synth")
    raw = np.ascontiguousarray(synth.tls_pair(a.points, config_id=2).target[:, :3], np.float32)
    ctx = api.Context(0)
    d = ctx._xyz(raw)
    res = dict(points=len(raw), mean_k=a.mean_k, std_mul=a.std, reps=a.reps, library=os.path.relpath(api.LIB_PATH, ROOT))

    def timed(fn):
        fn()  # warm-up (allocations, first launches)
        ctx.sync()
        ts, out = [], None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fn()
            ctx.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts))), out

    res["grid_and_bounds"], _ = timed(lambda: ctx.knn_mean_distance(d, 1))  # (mean_k = 1: the grid build and a near-trivial search)
    res["knn_stage"], dist = timed(lambda: ctx.knn_mean_distance(d, a.mean_k))
    res["sor_filter"], (keep, st) = timed(lambda: ctx.sor_filter(d, a.mean_k, a.std))
    res["kept"], res["stats4"] = int(keep.shape[0]), [float(v) for v in st]
    res["yardstick_knn_normals_k20"], _ = timed(lambda: ctx.knn_normals(d, 20))
    res["yardstick_knn_stage_mean_k19"], _ = timed(lambda: ctx.knn_mean_distance(d, 19))
    dist = dist.cpu().numpy()
    ctx.close()
    if a.cpu_queries > 0:
        import filters_restatement as F
        from scipy.spatial import cKDTree

        F.lib()
        q = min(a.cpu_queries, len(raw))
        t0 = time.perf_counter()
        ref = F.knn_mean_distance_range(raw, a.mean_k, 0, q)
        ms = (time.perf_counter() - t0) * 1e3
        res["cpu_restatement"] = dict(queries=q, ms=ms, ms_extrapolated_to_cloud=ms * len(raw) / q, bit_equal_to_gpu=bool(np.array_equal(ref.view(np.uint32), dist[:q].view(np.uint32))))
        x = raw.astype(np.float64)
        t0 = time.perf_counter()
        tree = cKDTree(x)
        dd, _ = tree.query(x, a.mean_k + 1, workers=16)
        res["cpu_kdtree_16_workers_ms"] = (time.perf_counter() - t0) * 1e3
        res["kdtree_max_rel_diff"] = float(np.max(np.abs(dd[:, 1:].mean(axis=1) / np.maximum(dist, 1e-30) - 1.0)[dist > 0]))
        res["speedup_knn_stage_vs_kdtree"] = res["cpu_kdtree_16_workers_ms"] / res["knn_stage"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
