"""Bits of the batched front end, one SHA-256 per cloud handle: what a refactor of batch.hip / batch_nms.hip / batch_dev.h must not change.  Runs
ghicp_clouds_recompute over a fixed list of small batches (inputs: the generators of tests/test_gpu_batch.py and of Part B of tests/test_gpu_nms.py)
and digests, per handle, the downloaded ds, kp, kp_xyz, feat and (n, m, k, candidates, variants, bbx_magnitude).
    GHICP_LIB=gh-icp_amd/libghicp_var_parent.so python scripts/frontend_bits.py parent.json    # a library built by scripts/branch_lib.sh
    GHICP_SIM=1 [GHICP_LIB=<a libghicp_sim.so>] python scripts/frontend_bits.py sim.json        # the host SIMT interpreter (no large-extent case)
Digests of two libraries are comparable within one backend only."""
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
import test_gpu_nms as nms  # noqa: E402
from oracle import oracle  # noqa: E402

SIM = os.environ.get("GHICP_SIM") == "1"


def context():
    if not SIM:
        return api.Context(0)
    from hipsim import build, simctx

    if os.environ.get("GHICP_LIB"):
        build.build = lambda: os.environ["GHICP_LIB"]
    return simctx.make_context(api)


def wedge(raw, n):
    """the n points of lowest azimuth: a sector of the scan at the scan's own density (the first n rows would be a few sparse rings)"""
    return np.ascontiguousarray(raw[np.argsort(np.arctan2(raw[:, 1], raw[:, 0]), kind="stable")[:n]])


def seventy(P=500):
    """the clouds of test_batch_of_more_than_64_clouds"""
    scan = wedge(synth.tls_pair(70 * P, pair_id=26).source, 70 * P)  # the whole scan, by azimuth
    raws = [np.ascontiguousarray(scan[i * P:(i + 1) * P]) for i in range(70)]
    raws[3], raws[40] = raws[3][:0], raws[40][:1]
    return raws


def digest(c):
    i, d = c.info(), c.download()
    h = hashlib.sha256()
    for key in ("ds", "kp", "kp_xyz", "feat"):
        h.update(b"-" if d[key] is None else np.ascontiguousarray(d[key].cpu().numpy()).tobytes())
    h.update(np.array([i.n, i.m, i.k, i.candidates, i.variants], np.int64).tobytes() + np.float32(i.bbx_magnitude).tobytes())
    return h.hexdigest()


def run(ctx, cfg, raws, keypoints=True):
    handles = [ctx.cloud_create(cfg, raws[0][:0]) for _ in raws]
    ctx.clouds_recompute(handles, raws)
    ks = [h.info().k for h in handles]
    assert not keypoints or max(ks) >= 3, ks  # the case is not vacuous
    out = [digest(h) for h in handles]
    for h in handles:
        h.close()
    return out


def main(out_path):
    oracle.build()
    ctx = context()
    pat = synth.bsc_pattern_glibc()
    res = {}
    a, b, g = synth.tls_pair(40_000, pair_id=21), synth.tls_pair(25_000, pair_id=22), synth.gauss_pair(3000)
    raws = [wedge(a.source, 4000), wedge(a.target, 4000), wedge(b.source, 4000), g.source, wedge(b.target, 2500), a.source[:1]]
    for tag, feat, corr, dof in (("bsc6", api.FEATURE_BSC, api.CORR_NN, 6), ("bsc4", api.FEATURE_BSC, api.CORR_NN, 4),
                                 ("fpfh", api.FEATURE_FPFH, api.CORR_NNR, 6), ("none", api.FEATURE_NONE, api.CORR_NN, 6)):
        res["equal_" + tag] = run(ctx, api.pair_config(feat, corr, dof=dof, voxel=0.2, pattern=pat, max_iter=40), raws)
    bsc = api.pair_config(api.FEATURE_BSC, api.CORR_NN, dof=6, voxel=0.2, pattern=pat, max_iter=40)
    p = synth.tls_pair(20_000, pair_id=24)
    empty = np.zeros((0, 3), np.float32)
    res["edge_cases"] = run(ctx, bsc, [empty, p.source[:1], np.tile(p.source[:1], (50, 1)), p.source, empty])
    res["two_empty"] = run(ctx, bsc, [empty, empty], keypoints=False)
    # a chain of NMS decisions longer than one launch sequence of the rounds
    ribbons = [nms._ribbon(300, grow=2.0 ** -14), nms._ribbon(150, grow=2.0 ** -14, mirror=True)]  # (200 columns: the shortest that takes two sequences)
    ds, curv, cand, _ = nms._reference(oracle, ribbons[0])
    assert nms.sync_depth(ds, curv, cand, nms.R) > nms.FB_NMS_ROUNDS
    assert nms._timed_batch(ctx, nms._cfg(api), ribbons) > 2  # two sequences of rounds at least, and the rank pass
    res["ribbons_two_sequences"] = run(ctx, nms._cfg(api), ribbons)
    res["batch_of_one"] = run(ctx, bsc, raws[:1])
    res["seventy_clouds"] = run(ctx, bsc, seventy())
    res["voxel_0_cloud_by_cloud"] = run(ctx, api.pair_config(api.FEATURE_BSC, api.CORR_NN, dof=6, voxel=0.0, pattern=pat, max_iter=40), [raws[0][:1500], raws[4][:1000]])
    if not SIM:  # clouds of large extent: the batch exceeds the cell budget and halves itself (test_batch_large_extent_splits_instead_of_failing)
        rng = np.random.default_rng(5)
        dense = synth.tls_pair(20_000, pair_id=25).source
        far = [(rng.random((400, 3), dtype=np.float32) - 0.5) * np.float32(300.0) for _ in range(6)]
        res["large_extent"] = run(ctx, bsc, [np.ascontiguousarray(np.concatenate([dense[i::6], far[i]]).astype(np.float32)) for i in range(6)], keypoints=False)
    ctx.close()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("%d cases, %d handles -> %s" % (len(res), sum(len(v) for v in res.values()), out_path))


if __name__ == "__main__":
    main(sys.argv[1])
