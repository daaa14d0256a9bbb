"""Point-to-point trimmed ICP WITH reciprocal correspondences of all 56 ordered pairs of 8 cfg2 clouds (0.1 m voxel filter) from poses
1 degree / 0.18 m off the truth (the clouds and pairs of scripts/gicp_clouds_timing.py), in ONE process on ONE stream:
  (a) per pair: ghicp_cloud_download of both clouds, ghicp_transform_cloud_f32 with the float-rounded pose, ghicp_icp with
      use_reciprocal = 1 -- the target's grids once per pair and two grids over the moved source per iteration, each with a host wait for
      its bounding box; the yardstick
  (b) ghicp_cloud_prepare_refine for the 8 clouds + one ghicp_refine_clouds_reciprocal
and checks that both give the same results, bit for bit.  Wall-clock medians of --reps rounds (default 5).  Writes one JSON line (--out,
default profiles/refine_reciprocal_timing.json): both times, their ratio, and -- from one more round of (b) under the library's event timing
-- the share of the chunks' time spent in the per-iteration grid build (boxes -> cell table; HIP events around that stage)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_reciprocal_timing.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (api.load() wants torch's HIP runtime first)

    api = importlib.import_module("gh-icp_amd.api")
    synth = importlib.import_module("gh-icp_amd.synth")
    pair = synth.tls_pair(a.hits, config_id=2)
    rng = np.random.default_rng(7)
    raws, pose = [], []  # pose[i]: base scan frame of cloud i -> the target scan's frame, composed with the cloud's own motion
    for base, to_target in ((pair.source, pair.gt), (pair.target, np.eye(4))):
        for v in range(4):
            M = rigid(7.0 * v - 9.0, (1.5 * v, -0.8 * v, 0.05 * v))
            keep = np.sort(rng.permutation(len(base))[: int(0.9 * len(base))])
            p = base[keep, :3].astype(np.float64)
            raws.append(np.ascontiguousarray((p @ M[:3, :3].T + M[:3, 3]).astype(np.float32)))
            pose.append(to_target @ np.linalg.inv(M))  # cloud frame -> target scan frame
    n = len(raws)
    pairs = [(i, j) for i in range(n) for j in range(n) if i != j]
    off = rigid(1.0, (0.15, -0.1, 0.03))
    inits = np.stack([off @ np.linalg.inv(pose[j]) @ pose[i] for i, j in pairs])
    ctx = api.Context(0)
    cfg = api.pair_config(api.FEATURE_NONE, api.CORR_NN, dof=6, voxel=0.1, max_iter=10)
    dev = [ctx._xyz(r) for r in raws]
    handles = [ctx.cloud_create(cfg, d) for d in dev]
    prm = api.icp_params(a.max_iter, True, True, api.ICP_POINT_TO_POINT, 0.3, 0.1, 15)
    res = dict(clouds=n, pairs=len(pairs), hits=a.hits, voxel=0.1, downsampled=[int(h.info().m) for h in handles], reps=a.reps, max_iter=int(prm.max_iter))

    def per_pair():
        out = []
        for (i, j), init in zip(pairs, inits):
            src = ctx.transform_cloud_f32(handles[i].download()["ds"], init.astype(np.float32))
            out.append(ctx.icp(src, handles[j].download()["ds"], prm, want_transformed=False))
        return out

    def prepare():
        for h in handles:
            h.prepare_refine(0)

    def batch():
        return ctx.refine_clouds_reciprocal(prm, [(handles[i], handles[j]) for i, j in pairs], inits)

    ta, tp, tb = [], [], []
    ra = rb = None
    for rep in range(a.reps + 1):  # the first round warms up (allocations, first launches) and is not counted
        ctx.clouds_recompute(handles, dev)  # forgets the prepared state: (b) pays for its 8 index builds in every round
        ctx.sync()
        t0 = time.perf_counter()
        ra = per_pair()
        ctx.sync()
        t1 = time.perf_counter()
        prepare()
        ctx.sync()
        t2 = time.perf_counter()
        rb = batch()
        ctx.sync()
        t3 = time.perf_counter()
        if rep:
            ta.append((t1 - t0) * 1e3)
            tp.append((t2 - t1) * 1e3)
            tb.append((t3 - t2) * 1e3)
    ctx.kernel_timing(True)  # one more batch under the library's event timing: the chunks, and inside them the per-iteration grid build
    t0 = time.perf_counter()
    batch()
    ctx.sync()
    tk_wall = (time.perf_counter() - t0) * 1e3
    loop_ms, chunks = ctx.kernel_time("refine")
    grid_ms, grid_builds = ctx.kernel_time("refine_recip_grid")
    ctx.kernel_timing(False)
    keys = ("done", "iterations", "converged", "reason", "overlap", "correspondences", "mse", "fitness")
    same = all(all(x[k] == y[k] for k in keys) and (not x["done"] or np.array_equal(x["T"], y["T"])) for x, y in zip(ra, rb))
    its = [r["iterations"] for r in rb]
    ms_a, ms_p, ms_b = float(np.median(ta)), float(np.median(tp)), float(np.median(tb))
    res["icp_reg_trimmed_reciprocal"] = dict(
        per_pair_ms=ms_a, batched_ms=ms_p + ms_b, prepare_ms=ms_p, batch_ms=ms_b, ratio_per_pair_over_batched=ms_a / (ms_p + ms_b),
        batched_is_faster=bool(ms_p + ms_b < ms_a), identical_results=bool(same), done=int(sum(r["done"] for r in rb)),
        iterations_sum=int(sum(its)), iterations_max=int(max(its)), grids_per_pair=2,
        host_round_trips=dict(batched=int(max(its)), per_pair_path_at_least=int(3 * sum(its))),  # per pair and iteration: two boxes and the status
        source_grid_builds=dict(batched_launch_sequences=int(grid_builds), per_pair_path=int(2 * sum(its))),
        batch_under_event_timing=dict(wall_ms=tk_wall, chunks_ms=loop_ms, chunks=int(chunks), grid_build_ms=grid_ms, grid_builds=int(grid_builds),
                                      grid_build_share_of_chunks=(grid_ms / loop_ms if loop_ms > 0 else None), host_ms=tk_wall - loop_ms))
    ctx.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
