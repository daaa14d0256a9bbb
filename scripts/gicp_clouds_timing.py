"""Generalized ICP of all 56 ordered pairs of 8 cfg2 clouds (0.1 m voxel filter) from poses 1 degree / 0.18 m off the truth (the clouds and
pairs of scripts/refine_timing.py), trimmed gate on, in ONE process on ONE stream:
  (a) per pair: ghicp_cloud_download of both clouds, ghicp_gicp_from with the float-rounded pose -- the k-NN covariances of both clouds and
      the target's grids are rebuilt for every pair; the yardstick
  (b) ghicp_cloud_prepare_gicp for the 8 clouds + one ghicp_gicp_clouds
and checks that both give the same results, bit for bit.  Writes one JSON line (--out, default profiles/gicp_clouds_timing.json): both
times, their ratio, the split of (b) into prepare and batch, launches per outer iteration, the kernel time of the chunks of (b)."""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gicp_clouds_timing.json"))
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
    prm = api.gicp_params(30, False, True, 0.3, 0.1, 20)  # the reference's constants: 20 inner steps, 1e-8 / 1e-6
    res = dict(clouds=n, pairs=len(pairs), hits=a.hits, voxel=0.1, downsampled=[int(h.info().m) for h in handles], reps=a.reps,
               max_iter=int(prm.max_iter), max_inner_iter=int(prm.max_inner_iter), covariance_k=int(prm.covariance_k))

    def per_pair():
        out = []
        for (i, j), init in zip(pairs, inits):
            out.append(ctx.gicp(handles[i].download()["ds"], handles[j].download()["ds"], prm, want_transformed=False, guess=init.astype(np.float32)))
        return out

    def prepare():
        for h in handles:
            h.prepare_gicp(prm.covariance_k, prm.gicp_epsilon)

    def batch():
        return ctx.gicp_clouds(prm, [(handles[i], handles[j]) for i, j in pairs], inits)

    ta, tp, tb = [], [], []
    ra = rb = None
    for rep in range(a.reps + 1):  # the first round warms up (allocations, first launches) and is not counted
        ctx.clouds_recompute(handles, dev)  # forgets the prepared state: (b) pays for its 8 covariance passes and index builds in every round
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
    ctx.kernel_timing(True)  # one more batch under the library's event timing: the share of the chunks' launch sequences in it
    t0 = time.perf_counter()
    batch()
    ctx.sync()
    tk_wall = (time.perf_counter() - t0) * 1e3
    loop_ms, chunks = ctx.kernel_time("gicp_clouds")
    ctx.kernel_timing(False)
    keys = ("done", "iterations", "converged", "reason", "overlap", "correspondences", "mse", "fitness")
    same = all(all(x[k] == y[k] for k in keys) and (not x["done"] or np.array_equal(x["T"], y["T"])) for x, y in zip(ra, rb))
    its = [r["iterations"] for r in rb]
    ms_a, ms_p, ms_b = float(np.median(ta)), float(np.median(tp)), float(np.median(tb))
    inner = int(prm.max_inner_iter)
    res["gicp_reg_gate"] = dict(
        per_pair_ms=ms_a, batched_ms=ms_p + ms_b, prepare_ms=ms_p, batch_ms=ms_b, ratio_per_pair_over_batched=ms_a / (ms_p + ms_b),
        batched_is_faster=bool(ms_p + ms_b < ms_a), identical_results=bool(same), done=int(sum(r["done"] for r in rb)),
        iterations_sum=int(sum(its)), iterations_max=int(max(its)),
        stream_ops_per_outer_iteration=dict(kernels=3 + 2 + 2 * inner + 1, memsets=1, status_copies=1, per_pair_path_times_pairs=len(pairs)),
        host_round_trips=dict(batched=int(max(its)), per_pair_path=int(sum(its))),
        covariance_passes=dict(batched=n, per_pair_path=2 * len(pairs)), index_builds=dict(batched=n, per_pair_path=len(pairs)),
        batch_under_event_timing=dict(wall_ms=tk_wall, chunks_ms=loop_ms, chunks=int(chunks), host_ms=tk_wall - loop_ms))
    ctx.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
