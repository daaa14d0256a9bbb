"""Generalized ICP (ghicp_gicp) on the clouds of DESIGN.md §4a: cfg2 after the 0.1 m voxel filter, the source pushed 1 degree / 0.18 m
off the truth.  Prints one JSON line: covariance time per cloud, GICP total / per outer iteration / per inner step, iterations,
accuracy against the truth, the single-thread CPU restatement's time, and icp_reg (trimmed) / ptplicp_reg on the same clouds with
the library that is loaded.  The time reference is the PARENT commit's library in the same job:
    GHICP_LIB=gh-icp_amd/libghicp_var_base.so python scripts/gicp_timing.py --icp-only --out base.json
    python scripts/gicp_timing.py --base base.json --out profiles/gicp_timing.json
--no-cpu skips the CPU restatement (profiler runs)."""
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


def rot_err(A, B):
    return float(np.linalg.norm(A[:3, :3] @ B[:3, :3].T - np.eye(3)))


def trans_err(A, B):
    return float(np.linalg.norm(A[:3, 3] - B[:3, 3]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--icp-only", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--base", default=None, help="JSON of the same script run on the parent commit's library (icp legs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (api.load() wants torch's HIP runtime first)

    api = importlib.import_module("gh-icp_amd.api")
    synth = importlib.import_module("gh-icp_amd.synth")
    from oracle import oracle as O

    pair = synth.tls_pair(config_id=2)
    S = pair.source[O.voxel_filter(pair.source, 0.1)][:, :3]
    T = pair.target[O.voxel_filter(pair.target, 0.1)][:, :3]
    ang = np.deg2rad(1.0)
    d = np.eye(4)
    d[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    d[:3, 3] = [0.15, -0.1, 0.03]
    coarse = d @ pair.gt
    S0 = np.ascontiguousarray(O.transform_cloud(S, coarse), np.float32)
    T = np.ascontiguousarray(T, np.float32)
    ctx = api.Context(0)
    dS, dT = ctx._xyz(S0), ctx._xyz(T)
    res = dict(clouds=dict(source=len(S0), target=len(T)), library=os.path.relpath(api.LIB_PATH, ROOT))

    def timed(fn):
        fn()  # warm-up (allocations, first launches)
        ctx.sync()
        ts = []
        out = None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fn()
            ctx.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), out

    for name, metric in (("icp_reg_trimmed", api.ICP_POINT_TO_POINT), ("ptplicp_reg_trimmed", api.ICP_POINT_TO_PLANE)):
        prm = api.icp_params(30, False, True, metric, 0.3, 0.1, 15)
        ms, r = timed(lambda: ctx.icp(dS, dT, prm))
        tot = r["T"].astype(np.float64) @ coarse
        res[name] = dict(ms=ms, iterations=r["iterations"], reason=r["reason"], ms_per_iteration=ms / max(1, r["iterations"]),
                         rot_err=rot_err(tot, pair.gt), trans_err=trans_err(tot, pair.gt))
    if not a.icp_only:
        prm = api.gicp_params(30, False, True, 0.3, 0.1, 20)
        cs, _ = timed(lambda: ctx.gicp_covariances(dS, 20))
        ct, _ = timed(lambda: ctx.gicp_covariances(dT, 20))
        ms, r = timed(lambda: ctx.gicp(dS, dT, prm))
        one, r1 = timed(lambda: ctx.gicp(dS, dT, api.gicp_params(1, False, True, 0.3, 0.1, 20, max_inner_iter=1)))
        it = max(1, r["iterations"])
        tot = r["T"].astype(np.float64) @ coarse
        g = dict(ms=ms, covariance_ms_source=cs, covariance_ms_target=ct, iterations=r["iterations"], reason=r["reason"],
                 correspondences=r["correspondences"], ms_per_outer_iteration=(ms - cs - ct) / it,
                 ms_one_iteration_one_inner_step=one, rot_err=rot_err(tot, pair.gt), trans_err=trans_err(tot, pair.gt), fitness=r["fitness"])
        if not a.no_cpu:
            import gicp_restatement as G

            G.lib(O)
            t0 = time.perf_counter()
            ro = G.gicp(O, S0, T, G.params(30, False, True, 0.3, 0.1, 20))
            g["cpu_restatement_ms"] = (time.perf_counter() - t0) * 1e3
            g["cpu_inner_steps"] = [int(v) for v in ro["inner"]]
            g["speedup_vs_cpu"] = g["cpu_restatement_ms"] / ms
            g["vs_cpu"] = dict(rot=rot_err(r["T"].astype(np.float64), ro["T"].astype(np.float64)),
                               trans=trans_err(r["T"].astype(np.float64), ro["T"].astype(np.float64)),
                               iterations=ro["iterations"], reason=ro["reason"])
        res["gicp_reg_trimmed"] = g
    if a.base:
        with open(a.base) as f:
            res["parent"] = {k: v for k, v in json.load(f).items() if k.endswith("_trimmed")}
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
