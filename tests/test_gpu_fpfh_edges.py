"""FPFH (gh-icp_amd/csrc/fpfh.hip: k_knn, k_knn_batch, k_normals, k_spfh, k_fpfh, k_gather_rows33) and its feature distance (fd.hip: k_fd_fpfh)
against a brute-force float32 restatement (tests/fpfh_restatement.py) on the clouds of tests/fpfh_edge_cases.py: fewer points than
neighbours, partial blocks, duplicates, ties at the k-th distance, planes, lines, far-away and tiny clouds, points on cell faces, rows of
4 floats, and a batch in which clouds of 1, 7 and 19 points sit between scans.  tests/test_fpfh_restatement_cpu.py proves the restatement
against the oracle on the same clouds first; here the oracle is a second witness.

No tolerance on histograms, gathered rows and feature distances: uint32 views are compared.  The one tolerance is 1e-6 on the cosine between
the GPU's normal and numpy's f64 eigh, on the rows where that normal is defined (fpfh_restatement.normal_filter; the CPU test counts them).
A feature distance of two rows of which one has no variance is 0 / 0: NaN is asserted exactly where the restatement has NaN, and the bits
are compared everywhere else (the payload of a NaN is not part of the contract).

Also runs on the host SIMT interpreter (GHICP_SIM=1): 22 s for the whole file there, of which the batch takes 10 s (on the batch's clouds
of 12 000 points the restatement computes the keypoints' rows only, fpfh_restatement.fpfh_brute_rows)."""
import ctypes as C

import numpy as np
import pytest

import fpfh_edge_cases as E
import fpfh_restatement as R

pytestmark = pytest.mark.gpu

U = np.uint32
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(U)


def _gpu(ctx, xyz):
    n, h = ctx.fpfh(xyz)
    return n.cpu().numpy(), h.cpu().numpy()


@pytest.mark.parametrize("name", [n for n in E.NAMES if n != "small_0"])
def test_fpfh_edge_case(ctx, oracle, synth, name):
    p = E.build(name, synth, oracle.voxel_filter)
    m = p.shape[0]
    ng, hg = _gpu(ctx, p)
    assert ng.shape == (m, 3) and hg.shape == (m, 33)
    assert np.isfinite(hg).all() and np.isfinite(ng).all()  # m = 1: incr = 100 / 0 must never be added
    # the restatement: brute-force neighbours, the GPU's own normals
    ref = R.fpfh_brute(p, ng, atan2f=oracle.atan2f)
    np.testing.assert_array_equal(_bits(hg), _bits(ref))
    # the oracle: normals (the existing contract, N2 / N3) and histograms
    no, ho = oracle.fpfh(p)
    np.testing.assert_array_equal(_bits(ng), _bits(no))
    np.testing.assert_array_equal(_bits(hg), _bits(ho))
    blocks = hg.reshape(m, 3, 11)
    assert ((np.abs(blocks.sum(2) - 100.0) < 1e-3) | (blocks == 0).all(2)).all()
    # rows of 4 floats, and a second run
    n4, h4 = _gpu(ctx, E.rows4(p))
    np.testing.assert_array_equal(_bits(h4), _bits(hg))
    np.testing.assert_array_equal(_bits(n4), _bits(ng))
    n2, h2 = _gpu(ctx, p)
    np.testing.assert_array_equal(_bits(h2), _bits(hg))
    np.testing.assert_array_equal(_bits(n2), _bits(ng))
    if name not in E.NORMAL_EXEMPT:
        nn, nd, nk = R.knn_brute(p)
        n64, lam = R.normals_f64(p, nn, nk)
        keep = R.normal_filter(p, n64, lam)
        assert keep.mean() >= E.KEEP_FLOOR.get(name, 0.9)
        cos = (n64 * ng).sum(1)[keep]
        assert (cos >= 1.0 - 1e-6).all(), cos.min()  # the same line and the same orientation
    if name in E.PLANES:  # closed form: the axis, and all of each block in its middle bin
        want = np.zeros(3, F)
        want[E.PLANES.index(name)] = -1.0
        np.testing.assert_array_equal(ng, np.tile(want, (m, 1)))
        np.testing.assert_array_equal(hg, np.tile(E.plane_row(), (m, 1)))


def test_fpfh_of_no_points_touches_nothing(ctx, api):
    t = ctx.torch
    x = ctx._xyz(E.small(5))
    nrm = t.full((5, 3), 7.0, dtype=t.float32, device=ctx.dev)
    hist = t.full((5, 33), 7.0, dtype=t.float32, device=ctx.dev)
    for stride in (3, 4):
        ctx._check(ctx.lib.ghicp_fpfh(ctx.h, api._ptr(x), C.c_int64(0), stride, 20, 20, api._ptr(nrm), api._ptr(hist)))
    assert (nrm.cpu().numpy() == 7.0).all() and (hist.cpu().numpy() == 7.0).all()


@pytest.mark.parametrize("k", [0, 1, 7, 8])
def test_fpfh_keypoints_gather(ctx, api, k):
    """ghicp_fpfh_keypoints (device pointers): k * 33 = 264 elements cross the 256-thread block at k = 8; repeated indices, the last row"""
    t = ctx.torch
    m = 57
    hist = np.random.default_rng(9).random((m, 33)).astype(F)
    idx = np.array([m - 1, 0, 13, 13, m - 1, 56, 1, 13], np.int32)[:k]
    out = t.full((k + 2, 33), -3.0, dtype=t.float32, device=ctx.dev)
    dh, di = ctx._dev(hist, t.float32), ctx._dev(np.concatenate([idx, np.array([10 ** 9], np.int32)]), t.int32)  # a wild index behind the list
    ctx._check(ctx.lib.ghicp_fpfh_keypoints(ctx.h, api._ptr(dh), api._ptr(di), C.c_int64(k), api._ptr(out)))
    got = out.cpu().numpy()
    np.testing.assert_array_equal(_bits(got[:k]), _bits(hist[idx]))
    assert (got[k:] == -3.0).all()  # nothing behind the k rows is written


def _keypoint_neighbour_first(raw, oracle, cfg):
    """The same scan with another point in front.  The voxel filter's output starts with a copy of input point 0 (its phantom voxel 0), so
    row 0 of the down-sampled cloud -- the first point of its cloud in the batch's concatenated array, where a search that picks the
    cloud of a point wrongly goes wrong -- is this point: the down-sampled point nearest to a keypoint, whose SPFH that keypoint weights."""
    keep = oracle.voxel_filter(raw, cfg.voxel)
    ds = raw[keep]
    kp, _ = oracle.keypoints(ds, cfg.neighborhood_radius, cfg.reg.radius_nonmax, cfg.ratio_max, cfg.min_neighbors)
    d = ((ds.astype(np.float64) - ds[kp[kp.size // 2]]) ** 2).sum(1)
    d[kp[kp.size // 2]] = d[0] = np.inf
    r = int(keep[np.argmin(d)])
    return np.ascontiguousarray(np.concatenate([raw[r:r + 1], raw[:r], raw[r + 1:]]))


def _batch_raws(synth, oracle, cfg):
    a = synth.tls_pair(20_000, pair_id=41)
    s1 = _keypoint_neighbour_first(np.ascontiguousarray(a.source[:, :3]), oracle, cfg)
    s2 = _keypoint_neighbour_first(np.ascontiguousarray(a.target[:, :3]), oracle, cfg)
    rng = np.random.default_rng(77)
    lo, hi = s1.min(0), s1.max(0)
    mid, half = 0.5 * (lo + hi), 0.25 * (hi - lo)
    seven = (mid + rng.uniform(-1.0, 1.0, (7, 3)) * half).astype(F)  # inside the first scan's bounding box
    nineteen = (mid + rng.uniform(-1.0, 1.0, (19, 3)) * half).astype(F)
    doubled = np.ascontiguousarray(np.repeat(s1, 2, axis=0))
    return [s1, seven, s2, s1[100:101].copy(), doubled, nineteen]


def test_fpfh_batch_against_restatement(ctx, api, synth, oracle):
    """One ghicp_clouds_recompute over scans with clouds of 7, 1 and 19 points between them: every handle's features are the restatement's
    FPFH of that handle's own down-sampled cloud, so no neighbour index left its cloud; the reversed batch gives the same features.
    Every scan follows a cloud smaller than k in one of the two orders, and its first point is a neighbour that a keypoint weights."""
    cfg = api.pair_config(api.FEATURE_FPFH, api.CORR_NNR, dof=6, voxel=0.2, max_iter=40)
    raws = _batch_raws(synth, oracle, cfg)
    clouds = [ctx.cloud_create(cfg, raws[0][:100]) for _ in raws]
    ctx.clouds_recompute(clouds, raws)

    def down(c):
        i, d = c.info(), c.download()
        ds = d["ds"].cpu().numpy() if d["ds"] is not None else np.zeros((0, 3), F)
        kp = d["kp"].cpu().numpy() if d["kp"] is not None else np.zeros(0, np.int32)
        return i, ds, kp, d["feat"].cpu().numpy()

    first = []
    for b, c in enumerate(clouds):
        i, ds, kp, feat = down(c)
        assert ds.shape == (i.m, 3) and kp.shape == (i.k,) and feat.shape == (i.k, 33)
        first.append((ds, kp, feat))
        ng, hg = _gpu(ctx, ds)
        ref, nn, nd = R.fpfh_brute_rows(ds, ng, kp, atan2f=oracle.atan2f)
        np.testing.assert_array_equal(_bits(feat), _bits(ref))
        np.testing.assert_array_equal(_bits(feat), _bits(hg[kp]))
        if b in (0, 2, 4):
            assert i.m > 1000 and i.k > 10  # the comparison is not vacuous
            assert ((nn == 0) & (nd > 0)).any()  # a keypoint weights the SPFH of the cloud's first point
    ms = [f[0].shape[0] for f in first]
    # clouds smaller than k between the scans (the voxel filter's phantom voxel 0 adds a copy of point 0: 7 -> 8, 19 -> 20 rows)
    assert ms[1] < 20 and ms[3] == 1 and ms[5] <= 20
    rev = [ctx.cloud_create(cfg, raws[0][:100]) for _ in raws]
    ctx.clouds_recompute(rev[::-1], raws[::-1])
    for c, (ds, kp, feat) in zip(rev, first):
        _, ds2, kp2, feat2 = down(c)
        np.testing.assert_array_equal(_bits(ds2), _bits(ds))
        np.testing.assert_array_equal(kp2, kp)
        np.testing.assert_array_equal(_bits(feat2), _bits(feat))
    for c in clouds + rev:
        c.close()


@pytest.mark.parametrize("ks,kt", E.FD_SHAPES)
def test_fd_fpfh_edges(ctx, ks, kt):
    hS, hT = E.fd_case(ks, kt)
    ref = R.fd_fpfh_ref(hS, hT)
    got = ctx.fd_fpfh(hS, hT).cpu().numpy()
    assert got.shape == (ks, kt)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    np.testing.assert_array_equal(_bits(got)[ok], _bits(ref)[ok])
