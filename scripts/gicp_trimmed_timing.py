"""What applying the trimmed rejector costs generalized ICP: the 56 ordered pairs of 8 cfg2 clouds of scripts/gicp_clouds_timing.py (0.1 m
voxel filter, poses 1 degree / 0.18 m off the truth, gate on), in ONE process on ONE stream, four ways:
  per pair  ghicp_gicp_from                 / ghicp_gicp_trimmed_from with trim_ratio 0 (each pair's overlap estimate)
  batched   ghicp_gicp_clouds               / ghicp_gicp_clouds_trimmed with trim_ratio 0, on handles prepared once
Trimming changes the correspondences and with them the number of outer iterations, so the figure compared is ms per outer iteration (the sum
over the pairs for the per-pair path, the longest pair's count for a batch, whose launch sequences serve all running pairs).  One more
trimmed batch and one more trimmed per-pair round run under the library's event timing: the share of the radix select (histogram reset ->
threshold) in them.  Checks that the trimmed batch gives the per-pair results, bit for bit.  Writes one JSON line (--out, default
profiles/gicp_trimmed_timing.json)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gicp_trimmed_timing.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (api.load() wants torch's HIP runtime first)

    api = importlib.import_module("gh-icp_amd.api")
    synth = importlib.import_module("gh-icp_amd.synth")
    pair = synth.tls_pair(a.hits, config_id=2)
    rng = np.random.default_rng(7)
    raws, pose = [], []  # the clouds and pairs of scripts/gicp_clouds_timing.py
    for base, to_target in ((pair.source, pair.gt), (pair.target, np.eye(4))):
        for v in range(4):
            M = rigid(7.0 * v - 9.0, (1.5 * v, -0.8 * v, 0.05 * v))
            keep = np.sort(rng.permutation(len(base))[: int(0.9 * len(base))])
            p = base[keep, :3].astype(np.float64)
            raws.append(np.ascontiguousarray((p @ M[:3, :3].T + M[:3, 3]).astype(np.float32)))
            pose.append(to_target @ np.linalg.inv(M))
    n = len(raws)
    pairs = [(i, j) for i in range(n) for j in range(n) if i != j]
    off = rigid(1.0, (0.15, -0.1, 0.03))
    inits = np.stack([off @ np.linalg.inv(pose[j]) @ pose[i] for i, j in pairs])
    ctx = api.Context(0)
    cfg = api.pair_config(api.FEATURE_NONE, api.CORR_NN, dof=6, voxel=0.1, max_iter=10)
    handles = [ctx.cloud_create(cfg, ctx._xyz(r)) for r in raws]
    ds = [h.download()["ds"] for h in handles]
    prm = api.gicp_params(30, False, True, 0.3, 0.1, 20)  # the reference's constants: 20 inner steps, 1e-8 / 1e-6
    for h in handles:
        h.prepare_gicp(prm.covariance_k, prm.gicp_epsilon)
    res = dict(clouds=n, pairs=len(pairs), hits=a.hits, voxel=0.1, downsampled=[int(h.info().m) for h in handles], reps=a.reps,
               max_iter=int(prm.max_iter), max_inner_iter=int(prm.max_inner_iter), covariance_k=int(prm.covariance_k), trim_ratio=0.0)

    def per_pair(ratio):
        return [ctx.gicp(ds[i], ds[j], prm, want_transformed=False, guess=init.astype(np.float32), trim_ratio=ratio) for (i, j), init in zip(pairs, inits)]

    def batch(ratio):
        return ctx.gicp_clouds(prm, [(handles[i], handles[j]) for i, j in pairs], inits, trim_ratio=ratio)

    def timed(fn, ratio):
        ts, r = [], None
        for rep in range(a.reps + 1):  # the first round warms up (allocations, first launches) and is not counted
            ctx.sync()
            t0 = time.perf_counter()
            r = fn(ratio)
            ctx.sync()
            if rep:
                ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), r

    out = {}
    for name, fn, its_of in (("per_pair", per_pair, lambda r: sum(x["iterations"] for x in r)), ("batched", batch, lambda r: max(x["iterations"] for x in r))):
        row = {}
        for tag, ratio in (("untrimmed", None), ("trimmed", 0.0)):
            ms, r = timed(fn, ratio)
            row[tag] = dict(ms=ms, outer_iterations=int(its_of(r)), ms_per_outer_iteration=ms / max(1, its_of(r)), done=int(sum(x["done"] for x in r)),
                            iterations_sum=int(sum(x["iterations"] for x in r)), kept_share_mean=float(np.mean([x["correspondences"] / len(ds[i]) for x, (i, _) in zip(r, pairs) if x["done"]])))
            out[name + "_" + tag] = r
        row["trimmed_over_untrimmed_per_outer_iteration"] = row["trimmed"]["ms_per_outer_iteration"] / row["untrimmed"]["ms_per_outer_iteration"]
        res[name] = row
    keys = ("done", "iterations", "converged", "reason", "overlap", "correspondences", "mse", "fitness")
    same = all(all(x[k] == y[k] for k in keys) and (not x["done"] or np.array_equal(x["T"], y["T"])) for x, y in zip(out["per_pair_trimmed"], out["batched_trimmed"]))
    res["identical_results"] = bool(same)
    # the share of the select under the library's event timing
    ctx.kernel_timing(True)
    t0 = time.perf_counter()
    batch(0.0)
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e3
    chunks_ms, chunks = ctx.kernel_time("gicp_clouds")
    sel_ms, sels = ctx.kernel_time("gicp_select")
    res["batched"]["select_under_event_timing"] = dict(wall_ms=wall, chunks_ms=chunks_ms, chunks=int(chunks), select_ms=sel_ms, selects=int(sels),
                                                       select_share_of_chunks=sel_ms / chunks_ms if chunks_ms else None)
    ctx.kernel_timing(False)
    ctx.kernel_timing(True)  # (switching it on resets the sums)
    t0 = time.perf_counter()
    per_pair(0.0)
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e3
    sel_ms, sels = ctx.kernel_time("gicp_select")
    res["per_pair"]["select_under_event_timing"] = dict(wall_ms=wall, select_ms=sel_ms, selects=int(sels), select_share_of_wall=sel_ms / wall)
    ctx.kernel_timing(False)
    for h in handles:
        h.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
