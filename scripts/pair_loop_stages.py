#!/usr/bin/env python
"""Where a pair-iteration of the persistent pair loop spends its time: prints the stage timers of ghicp_ctx_pair_loop_stats (statistics sweep,
graph build, Kuhn-Munkres solve, tail after the solve; kernel timing on) beside the headline.

  python scripts/pair_loop_stages.py <bench result .json> [label]   the JSON line of a bench.py run and the slot figures it carries; the stage
                                                                    timers are not part of that line (bench.py reads the first eight values)
  python scripts/pair_loop_stages.py                                one small synthetic batch on the GPU, through the library's own call
"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def from_bench(path, label):
    d = json.loads(open(path).read().strip().splitlines()[-1])
    p = d.get("pair_loop_stats") or {}
    non_solve = p["mean_solve_ms"] * (1.0 / p["solve_share_of_slot_time"] - 1.0) if p.get("solve_share_of_slot_time") else float("nan")
    print("%s: %.1f registered pairs/s, %.1f all pairs/s, %.0f ms/step; slots %s, span %.0f ms, idle %.4f, mean solve %.3f ms, solve share %.4f"
          " -> non-solve %.3f ms per pair-iteration" % (label, d.get("value", 0), d.get("value_all_pairs", 0), d.get("ms_per_step", 0), p.get("slots_run"),
                                                        p.get("mean_launch_span_ms", 0), p.get("idle_slot_fraction", 0), p.get("mean_solve_ms", 0),
                                                        p.get("solve_share_of_slot_time", 0), non_solve))


def small_batch():
    import numpy as np

    api = importlib.import_module("gh-icp_amd.api")
    synth = importlib.import_module("gh-icp_amd.synth")
    ctx = api.Context(0)
    rng = np.random.default_rng(3)
    cfg = api.pair_config(api.FEATURE_BSC, api.CORR_KM, dof=6, est_iou=0.6, voxel=0.2, pattern=synth.bsc_pattern_glibc(), max_iter=30)
    p = synth.gauss_pair(n_kp=700)
    S, T = p.source[p.kp_source].astype(np.float64), p.target[p.kp_target].astype(np.float64)
    clouds = []
    for _ in range(64):
        ks, kt = int(rng.integers(400, 700)), int(rng.integers(400, 700))
        fS = rng.integers(0, 256, size=(4, ks, 56), dtype=np.uint8)
        fT = rng.integers(0, 256, size=(4, kt, 56), dtype=np.uint8)
        m = min(ks, kt)
        fT[0, :m] = fS[0, :m] ^ (rng.random((m, 56)) < 0.03).astype(np.uint8)
        clouds.append((ctx.cloud_from_features(cfg, S[:ks], fS, 100.0), ctx.cloud_from_features(cfg, T[:kt], fT, 100.0)))
    ctx.kernel_timing(True)
    ctx.register_clouds(cfg, clouds)
    st = ctx.pair_loop_stats()
    ctx.kernel_timing(False)
    print(json.dumps(st))
    ctx.close()


if __name__ == "__main__":
    if len(sys.argv) > 1:
        from_bench(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.basename(sys.argv[1]))
    else:
        small_batch()
