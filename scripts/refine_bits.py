"""Bits of the three batched refiners over cached clouds (ghicp_refine_clouds, ghicp_refine_clouds_reciprocal, ghicp_gicp_clouds), one SHA-256
per pair: what a refactor of refine.hip / refine_recip.hip / refine_gicp.hip / refine_dev.h / refine_run.h must not change.  Runs a fixed list
of small batches (inputs: the generators of tests/test_gpu_refine.py, test_gpu_refine_reciprocal.py and test_gpu_gicp_clouds.py) and digests
the raw bytes of every field of every pair's result: all stats, T (T_icp) and Rt_refined.
    GHICP_LIB=gh-icp_amd/libghicp_var_parent.so python scripts/refine_bits.py parent.json      # a library built by scripts/branch_lib.sh
    GHICP_SIM=1 [GHICP_LIB=<a libghicp_sim.so>] python scripts/refine_bits.py sim.json          # the host SIMT interpreter
Digests of two libraries are comparable within one backend only (sqrt, sin, cos differ between them)."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
api = importlib.import_module("gh-icp_amd.api")
synth = importlib.import_module("gh-icp_amd.synth")
import test_gpu_gicp_clouds as gg  # noqa: E402
import test_gpu_refine as rf  # noqa: E402
import test_gpu_refine_reciprocal as rr  # noqa: E402

SIM = os.environ.get("GHICP_SIM") == "1"
COMBOS = ((0, False), (0, True), (1, False), (1, True))  # metric x trimmed


def context():
    if not SIM:
        return api.Context(0)
    from hipsim import build, simctx

    if os.environ.get("GHICP_LIB"):
        build.build = lambda: os.environ["GHICP_LIB"]
    return simctx.make_context(api)


def sha(r):
    h = hashlib.sha256()
    for k in sorted(r):
        h.update(k.encode())
        h.update(np.ascontiguousarray(r[k]).tobytes())
    return h.hexdigest()


def put(res, tag, got):
    for p, r in enumerate(got):
        res["%s/%d" % (tag, p)] = sha(r)


def edge_clouds(ctx):
    """the launch-edge batch of the tests: sources of < 4 points, one block, 257-258 points, > 2048 points over one lattice target"""
    cfg = api.pair_config(api.FEATURE_NONE, api.CORR_NN, dof=6, voxel=0.2, max_iter=10)
    raws, tgt, init = rf.edge_raws()
    clouds = [ctx.cloud_create(cfg, x) for x in raws + [tgt]]
    ms = [int(c.info().m) for c in clouds]
    assert ms[0] < 4 and 4 <= ms[1] <= 256 and 257 <= ms[2] <= 258 and ms[3] > 2048, ms
    return clouds, init


def main(out_path):
    ctx = context()
    res = {}
    w = gg.GWorld(ctx, api, synth)  # test_gpu_refine's clouds and pairs, plus the GICP preparation
    w.prepare(rf.K)
    w.prepare_gicp()
    pairs = list(w.pairs)
    handles = lambda ps: [(w.clouds[s], w.clouds[t]) for s, t, _ in ps]  # noqa: E731
    inits = lambda ps: np.stack([p[2] for p in ps])  # noqa: E731
    inside = pairs[:3]
    inside.insert(1, w.refused)  # the refused pair shares a chunk with its neighbours
    no_init = [pairs[3], pairs[1]]
    empty = ctx.cloud_create(w.cfg, w.raw["A"][:0])
    empty.prepare_refine(rf.K)
    empty.prepare_gicp(gg.K, gg.EPS)
    hollow = [(empty, w.clouds["B"]), (w.clouds["C"], w.clouds["B"]), (w.clouds["A"], empty)]  # an empty source, a live pair, an empty target
    hollow_init = np.stack([pairs[0][2], pairs[3][2], pairs[0][2]])
    edges, edge_init = edge_clouds(ctx)
    for c in edges:
        c.prepare_refine(rf.K)
        c.prepare_gicp(gg.K, gg.EPS)
    edge_pairs = [(edges[i], edges[4]) for i in (3, 0, 1, 3, 2, 0)]
    edge_inits = np.stack([edge_init] * len(edge_pairs))

    # ---- ghicp_refine_clouds
    for metric, trimmed in COMBOS:
        prm = rf.params_of(api, metric, trimmed)
        tag = "icp_m%d_t%d" % (metric, trimmed)
        ps = pairs + ([w.refused] if trimmed else [])
        put(res, tag + "_init", ctx.refine_clouds(prm, handles(ps), inits(ps)))
        put(res, tag + "_noinit", ctx.refine_clouds(prm, handles(no_init), None))
        put(res, tag + "_hollow", ctx.refine_clouds(prm, hollow, hollow_init))
        put(res, tag + "_edges", ctx.refine_clouds(rf.params_of(api, metric, trimmed, max_iter=3), edge_pairs, edge_inits))
    prm = rf.params_of(api, 0, True)
    for mc in (0, 1, 2):
        put(res, "icp_m0_t1_mc%d" % mc, ctx.refine_clouds(prm, handles(pairs), inits(pairs), mc))
    put(res, "icp_m0_t1_refused_inside", ctx.refine_clouds(prm, handles(inside), inits(inside), 3))
    put(res, "icp_m0_t1_edges_mc2", ctx.refine_clouds(rf.params_of(api, 0, True, max_iter=3), edge_pairs, edge_inits, 2))

    # ---- ghicp_refine_clouds_reciprocal
    for metric, trimmed in COMBOS:
        prm = rr.params_of(api, metric, trimmed)
        tag = "recip_m%d_t%d" % (metric, trimmed)
        ps = pairs + ([w.refused] if trimmed else [])
        put(res, tag + "_init", ctx.refine_clouds_reciprocal(prm, handles(ps), inits(ps)))
        put(res, tag + "_hollow", ctx.refine_clouds_reciprocal(prm, hollow, hollow_init))
        put(res, tag + "_edges", ctx.refine_clouds_reciprocal(prm, edge_pairs, edge_inits))
    put(res, "recip_m0_t1_refused_inside", ctx.refine_clouds_reciprocal(rr.params_of(api, 0, True), handles(inside), inits(inside), 3))

    # ---- ghicp_gicp_clouds
    for trimmed in (False, True):
        prm = gg.gparams(api, trimmed)
        tag = "gicp_t%d" % trimmed
        ps = pairs + ([w.refused] if trimmed else [])
        put(res, tag + "_init", ctx.gicp_clouds(prm, handles(ps), inits(ps)))
        put(res, tag + "_noinit", ctx.gicp_clouds(prm, handles(no_init), None))
        put(res, tag + "_hollow", ctx.gicp_clouds(prm, hollow, hollow_init))
        put(res, tag + "_edges", ctx.gicp_clouds(gg.gparams(api, trimmed, max_dist=0.4), edge_pairs, edge_inits))
    put(res, "gicp_t1_refused_inside", ctx.gicp_clouds(gg.gparams(api, True), handles(inside), inits(inside), 3))
    put(res, "gicp_t1_mc2", ctx.gicp_clouds(gg.gparams(api, True), handles(pairs), inits(pairs), 2))

    for c in list(w.clouds.values()) + edges + [empty]:
        c.close()
    ctx.close()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("%d pairs -> %s" % (len(res), out_path))


if __name__ == "__main__":
    main(sys.argv[1])
