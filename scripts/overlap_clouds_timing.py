"""calOverlap of all 56 ordered pairs of 8 cfg2 clouds (0.1 m voxel filter; the clouds of scripts/gicp_clouds_timing.py), thre_dis = 0.5 (the
ICP default), in ONE process on ONE stream, twice: under the ground-truth poses, and with every pose pushed 900 m away (the hopeless case:
no pair shares anything).
  (a) per pair: ghicp_transform_cloud_f32 + ghicp_cal_overlap on device pointers (the down-sampled clouds, downloaded once beforehand) --
      the target's grid is rebuilt and the host waits once for every pair; the yardstick
  (b) ghicp_cloud_prepare_overlap for the 8 clouds + one ghicp_overlap_clouds
and checks that both give the same ratios, bit for bit.  Writes one JSON line (--out, default profiles/overlap_clouds_timing.json): both
times, their ratio, the split of (b) into prepare and batch."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THRE_DIS = 0.5


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap_clouds_timing.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (api.load() wants torch's HIP runtime first)

    api = importlib.import_module("gh-icp_amd.api")
    synth = importlib.import_module("gh-icp_amd.synth")
    pair = synth.tls_pair(a.hits, config_id=2)
    rng = np.random.default_rng(7)
    raws, pose = [], []  # pose[i]: cloud i's frame -> the target scan's frame
    for base, to_target in ((pair.source, pair.gt), (pair.target, np.eye(4))):
        for v in range(4):
            M = rigid(7.0 * v - 9.0, (1.5 * v, -0.8 * v, 0.05 * v))
            keep = np.sort(rng.permutation(len(base))[: int(0.9 * len(base))])
            p = base[keep, :3].astype(np.float64)
            raws.append(np.ascontiguousarray((p @ M[:3, :3].T + M[:3, 3]).astype(np.float32)))
            pose.append(to_target @ np.linalg.inv(M))
    n = len(raws)
    pairs = [(i, j) for i in range(n) for j in range(n) if i != j]
    truth = np.stack([np.linalg.inv(pose[j]) @ pose[i] for i, j in pairs])
    away = np.stack([rigid(0.0, (900.0, 0.0, 0.0)) @ M for M in truth])
    ctx = api.Context(0)
    cfg = api.pair_config(api.FEATURE_NONE, api.CORR_NN, dof=6, voxel=0.1, max_iter=10)
    dev = [ctx._xyz(r) for r in raws]
    handles = [ctx.cloud_create(cfg, d) for d in dev]
    ds = [h.download()["ds"] for h in handles]
    S, T = [handles[i] for i, _ in pairs], [handles[j] for _, j in pairs]
    res = dict(clouds=n, pairs=len(pairs), hits=a.hits, voxel=0.1, thre_dis=THRE_DIS, downsampled=[int(h.info().m) for h in handles], reps=a.reps)

    def per_pair(Rt):
        return [ctx.cal_overlap(ctx.transform_cloud_f32(ds[i], M.astype(np.float32)), ds[j], THRE_DIS) for (i, j), M in zip(pairs, Rt)]

    def prepare():
        for h in handles:
            h.prepare_overlap(THRE_DIS)

    for name, Rt in (("ground_truth_poses", truth), ("poses_900_m_away", away)):
        ta, tp, tb = [], [], []
        ra = rb = None
        for rep in range(a.reps + 1):  # the first round warms up (allocations, first launches) and is not counted
            ctx.clouds_recompute(handles, dev)  # forgets the prepared state: (b) pays for its 8 grid builds in every round
            ctx.sync()
            t0 = time.perf_counter()
            ra = per_pair(Rt)
            ctx.sync()
            t1 = time.perf_counter()
            prepare()
            ctx.sync()
            t2 = time.perf_counter()
            rb = ctx.overlap_clouds(S, T, THRE_DIS, Rt)
            ctx.sync()
            t3 = time.perf_counter()
            if rep:
                ta.append((t1 - t0) * 1e3)
                tp.append((t2 - t1) * 1e3)
                tb.append((t3 - t2) * 1e3)
        same = all(np.float32(x) == y for x, y in zip(ra, rb["ratio"]))
        ms_a, ms_p, ms_b = float(np.median(ta)), float(np.median(tp)), float(np.median(tb))
        res[name] = dict(per_pair_ms=ms_a, batched_ms=ms_p + ms_b, prepare_ms=ms_p, batch_ms=ms_b, ratio_per_pair_over_batched=ms_a / (ms_p + ms_b),
                         batched_is_faster=bool(ms_p + ms_b < ms_a), identical_results=bool(same), source_points=int(rb["n"].sum()),
                         hits=int(rb["hits"].sum()), pairs_with_hits=int((rb["hits"] > 0).sum()), ratio_min=float(rb["ratio"].min()),
                         ratio_max=float(rb["ratio"].max()), grid_builds=dict(batched=n, per_pair_path=len(pairs)))
    res["identical_results"] = bool(all(res[k]["identical_results"] for k in ("ground_truth_poses", "poses_900_m_away")))
    ctx.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
