"""Bits of the GH-ICP loop, one SHA-256 per case: what a refactor of loop.hip / pair_loop.hip / loop_dev.h must not change.  Registers a fixed list
of small pairs at the code's tile edges (inputs: the generators of tests/test_gpu_loop_fused.py) and digests the raw bytes of every field of
every iteration record, the iteration count, the 4x4 and the match list (batch cases: what ghicp_register_clouds returns per pair).
    GHICP_LIB=gh-icp_amd/libghicp_var_parent.so python scripts/loop_bits.py parent.json        # a library built by scripts/branch_lib.sh
    GHICP_SIM=1 [GHICP_LIB=<a libghicp_sim.so>] python scripts/loop_bits.py sim.json            # the host SIMT interpreter (no staged-KM cases)
Digests of two libraries are comparable within one backend only (pow, sqrt differ between them)."""
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
import test_gpu_loop_fused as gen  # noqa: E402
from oracle import oracle  # noqa: E402

SIM = os.environ.get("GHICP_SIM") == "1"
FEATS = (("bsc", api.FEATURE_BSC), ("fpfh", api.FEATURE_FPFH), ("none", api.FEATURE_NONE))


def context(**env):
    """a context of its own: the switches are read from the environment when a context is created"""
    os.environ.update(env)
    try:
        if not SIM:
            return api.Context(0)
        from hipsim import build, simctx

        if os.environ.get("GHICP_LIB"):
            build.build = lambda: os.environ["GHICP_LIB"]
        return simctx.make_context(api)
    finally:
        for k in env:
            del os.environ[k]


def sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def fd_of(feature, rng, ks, kt):
    if feature == api.FEATURE_BSC:
        return gen._fake_bsc_fd(rng, ks, kt).astype(np.int16)
    return (0.2 + 0.6 * rng.random((ks, kt))).astype(np.float32) if feature == api.FEATURE_FPFH else None


def one(ctx, S, T, bbx, feature, corr, ks, kt, max_iter=8):
    import torch

    FD = fd_of(feature, np.random.default_rng(100 + ks * 7 + kt), ks, kt)
    pg = api.default_params(feature, corr, 6, 0.9 if feature == api.FEATURE_NONE else 0.6, 1.5, bbx, max_iter=max_iter)
    r = ctx.register(pg, S[:ks], T[:kt], None if FD is None else torch.from_numpy(FD).to(ctx.dev), want_matchlist=True)
    return sha(np.int64(r["iters"]), *[np.asarray(rec[k]) for rec in r["trace"] for k in sorted(rec)], r["Rt"], r["matchlist"])


def batch(ctx, S, T, bbx, feature, corr, shapes, max_iter=8):
    """the pairs of `shapes` in ONE ghicp_register_clouds call, from keypoints and random feature strings / histograms"""
    rng = np.random.default_rng(7)
    cfg = api.pair_config(feature, corr, dof=6, est_iou=0.6, voxel=0.2, pattern=synth.bsc_pattern_glibc(), max_iter=max_iter)
    feat = {api.FEATURE_BSC: lambda k: rng.integers(0, 256, size=(4, k, 56), dtype=np.uint8),
            api.FEATURE_FPFH: lambda k: (0.05 + rng.random((k, 33))).astype(np.float32), api.FEATURE_NONE: lambda k: None}[feature]
    pairs = [(ctx.cloud_from_features(cfg, S[:ks], feat(ks), bbx), ctx.cloud_from_features(cfg, T[:kt], feat(kt), bbx)) for ks, kt in shapes]
    out = ctx.register_clouds(cfg, pairs)
    d = sha(*[np.asarray(x) for r in out for x in (np.int64(r.iterations), np.int64(r.converged), list(r.Rt), np.float64(r.rmse_after))])
    for a, b in pairs:
        a.close()
        b.close()
    return d


def main(out_path):
    oracle.build()
    fixture = getattr(gen.pair, "__wrapped__", None) or gen.pair.__pytest_wrapped__.obj
    S, T, bbx = fixture(synth, oracle)
    res = {}
    # the persistent pair loop: fused, unfused, and with a slot large enough to stage kpT in LDS
    for tag, env in (("fused", {}), ("unfused", {"GHICP_LOOP_FUSE": "0"}), ("minlds", {"GHICP_LOOP_MIN_LDS": "46080"})):
        ctx = context(**env)
        for ks, kt in ((257, 255), (300, 513), (513, 300), (65, 64), (3, 5)):
            res["pl_bsc_km_%dx%d_%s" % (ks, kt, tag)] = one(ctx, S, T, bbx, api.FEATURE_BSC, api.CORR_KM, ks, kt)
        if tag != "minlds":
            res["pl_fpfh_km_130x150_" + tag] = one(ctx, S, T, bbx, api.FEATURE_FPFH, api.CORR_KM, 130, 150)
            res["pl_none_km_150x130_" + tag] = one(ctx, S, T, bbx, api.FEATURE_NONE, api.CORR_KM, 150, 130)
        ctx.close()
    # the per-stage kernels: NN and NNR; a batch takes pick_chunks with batch > 1, and blocks beyond a pair's extent return early
    ctx = context()
    for fname, feature in FEATS:
        for cname, corr in (("nn", api.CORR_NN), ("nnr", api.CORR_NNR)):
            res["staged_%s_%s_257x255" % (fname, cname)] = one(ctx, S, T, bbx, feature, corr, 257, 255)
            res["staged_%s_%s_batch3" % (fname, cname)] = batch(ctx, S, T, bbx, feature, corr, ((257, 255), (64, 65), (300, 513)))
    if not SIM:  # graphs beyond the LDS-resident solver (k_km_csr, k_km_scan_desc, k_km_weights): too slow for the interpreter
        N = next(n for n in range(1, 65535) if ctx.lib.ghicp_km4_lds_bytes(n, 0) > 160 * 1024 - 256)
        Sb = 20.0 * np.random.default_rng(3).standard_normal((N, 3))
        a = np.deg2rad(12.0)
        Tb = Sb @ np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]).T + np.array([1.5, -0.8, 0.3])
        for fname, feature in FEATS:
            res["staged_%s_km_%dx%d_and_64x65" % (fname, N, N)] = batch(ctx, Sb, Tb, bbx, feature, api.CORR_KM, ((N, N), (64, 65)), 3)
    ctx.close()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("%d cases -> %s" % (len(res), out_path))


if __name__ == "__main__":
    main(sys.argv[1])
