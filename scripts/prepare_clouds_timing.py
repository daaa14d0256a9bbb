"""Preparing 8 and 64 cfg2 clouds (0.1 m voxel filter; the clouds of scripts/gicp_clouds_timing.py and more variants of them) for the batched
stages, in ONE process on ONE stream, for three specs -- refine + normals k 15; GICP k 20; overlap 0.5:
  (a) the per-cloud calls: ghicp_cloud_prepare_refine / ghicp_cloud_prepare_gicp / ghicp_cloud_prepare_overlap, handle by handle
  (b) one ghicp_clouds_prepare for the list
Wall clock, median of --reps rounds after a warm-up round; the handles are recomputed before every measurement, so nothing is skipped.  Checks
that both leave the same state, byte for byte (info structs and all downloads), and records the host waits of (b) and the split of one (b)
under the library's event timing.  Writes one JSON line (--out, default profiles/prepare_clouds_timing.json)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rigid(deg, t):
    a = np.deg2rad(deg)
    m = np.eye(4)
    m[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    m[:3, 3] = t
    return m


SPECS = [("refine_normals15", dict(refine=True, normals_k=15)), ("gicp20", dict(gicp_k=20, gicp_eps=1e-3)), ("overlap0.5", dict(overlap_thre=0.5))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--counts", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepare_clouds_timing.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (api.load() wants torch's HIP runtime first)

    api = importlib.import_module("gh-icp_amd.api")
    synth = importlib.import_module("gh-icp_amd.synth")
    pair = synth.tls_pair(a.hits, config_id=2)
    rng = np.random.default_rng(7)
    nmax = max(a.counts)
    raws = []
    for i in range(nmax):  # alternating between the two scans, each variant moved and thinned on its own
        base = (pair.source, pair.target)[i % 2]
        v = i // 2
        M = rigid(7.0 * (v % 4) - 9.0 + 0.3 * (v // 4), (1.5 * (v % 4), -0.8 * (v % 4), 0.05 * v))
        keep = np.sort(rng.permutation(len(base))[: int(0.9 * len(base))])
        p = base[keep, :3].astype(np.float64)
        raws.append(np.ascontiguousarray((p @ M[:3, :3].T + M[:3, 3]).astype(np.float32)))
    ctx = api.Context(0)
    cfg = api.pair_config(api.FEATURE_NONE, api.CORR_NN, dof=6, voxel=0.1, max_iter=10)
    dev = [ctx._xyz(r) for r in raws]
    handles = [ctx.cloud_create(cfg, d) for d in dev]
    res = dict(hits=a.hits, voxel=0.1, reps=a.reps, downsampled=[int(h.info().m) for h in handles], runs=[])

    def per_cloud(hs, refine=False, normals_k=0, gicp_k=0, gicp_eps=1e-3, overlap_thre=None):
        for h in hs:
            if refine or normals_k > 0:
                h.prepare_refine(normals_k)
            if gicp_k > 0:
                h.prepare_gicp(gicp_k, gicp_eps)
            if overlap_thre is not None:
                h.prepare_overlap(overlap_thre)

    def state(hs):
        out = []
        for h in hs:
            parts = [bytes(h.prepared())]
            for which in range(8):
                try:
                    parts.append(h.download_prepared(which).cpu().numpy().tobytes())
                except api.GhicpError:
                    parts.append(None)
            out.append(parts)
        return out

    for count in a.counts:
        hs, ds = handles[:count], dev[:count]
        for name, spec in SPECS:
            ta, tb, waits = [], [], 0
            for rep in range(a.reps + 1):  # the first round warms up (allocations, first launches) and is not counted
                ctx.clouds_recompute(hs, ds)  # forgets the prepared state
                ctx.sync()
                t0 = time.perf_counter()
                per_cloud(hs, **spec)
                ctx.sync()
                t1 = time.perf_counter()
                sa = state(hs) if rep == a.reps else None
                ctx.clouds_recompute(hs, ds)
                ctx.sync()
                t2 = time.perf_counter()
                ctx.prepare_clouds(hs, **spec)
                ctx.sync()
                t3 = time.perf_counter()
                waits = ctx.prepare_host_waits()
                sb = state(hs) if rep == a.reps else None
                if rep:
                    ta.append((t1 - t0) * 1e3)
                    tb.append((t3 - t2) * 1e3)
            ctx.clouds_recompute(hs, ds)  # one more batch under the library's event timing: where the time of the chunks goes
            ctx.sync()
            ctx.kernel_timing(True)
            t0 = time.perf_counter()
            ctx.prepare_clouds(hs, **spec)
            ctx.sync()
            wall = (time.perf_counter() - t0) * 1e3
            grids_ms, grids_n = ctx.kernel_time("prepare_grids")
            knn_ms, knn_n = ctx.kernel_time("prepare_knn")
            ctx.kernel_timing(False)
            ms_a, ms_b = float(np.median(ta)), float(np.median(tb))
            res["runs"].append(dict(clouds=count, spec=name, per_cloud_ms=ms_a, batched_ms=ms_b, ratio_per_cloud_over_batched=ms_a / ms_b,
                                    batched_is_faster=bool(ms_b < ms_a), identical_results=bool(sa == sb), host_waits_batched=int(waits),
                                    batch_under_event_timing=dict(wall_ms=wall, grids_ms=grids_ms, grid_brackets=int(grids_n), knn_ms=knn_ms,
                                                                  knn_passes=int(knn_n), other_ms=wall - grids_ms - knn_ms)))
    ctx.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
