"""calOverlap of many pairs of cached clouds in one launch (ghicp_cloud_prepare_overlap / ghicp_overlap_clouds / ghicp_overlap_matrix).  Every
pair of a batch must come out exactly -- hits and ratio, bit for bit -- as the per-pair path gives it: ghicp_cloud_download,
ghicp_transform_cloud_f32 with the float-rounded pose, ghicp_cal_overlap against the target's down-sampled cloud; whatever the other pairs of
the call are, whatever their order and whatever the chunking.  Every comparison here is exact.

The small clouds go through the handles' voxel filter at a 1 mm voxel, which keeps every point: the filter always keeps input point 0 and
drops any OTHER point of the corner voxel of the bounding box (key 0, filter.hpp:52-83), so the clouds below put their point 0 on that
corner; Clouds.add asserts that the handle holds as many points as it was given."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_refine import STAT_KEYS, displaced, params_of

pytestmark = pytest.mark.gpu

VOXEL = 1e-3
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 513)  # sources of the edge batch: none, one lane, a wave -1 / 0 / +1, a block -1 / 0 / +1, three blocks


def cube(rng, n, side=4.0):
    p = rng.uniform(0.0, side, (n, 3)).astype(np.float32)
    return on_corner(p)


def on_corner(p):
    p = np.ascontiguousarray(p, np.float32)
    if len(p):
        p[0] = p.min(axis=0)  # point 0 on the corner of the bounding box (module docstring)
    return p


def small_pose(rng, deg=3.0, shift=0.2):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(rng.uniform(-deg, deg))
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
    M[:3, 3] = rng.uniform(-shift, shift, 3)
    return M


class Clouds:
    """Handles with their down-sampled points (as the handle holds them) and the per-pair reference, computed once per (source, target,
    pose, thre_dis) and never changed."""

    def __init__(self, ctx, api, voxel=VOXEL):
        self.ctx, self.api = ctx, api
        self.cfg = api.pair_config(api.FEATURE_NONE, api.CORR_NN, dof=6, voxel=voxel, max_iter=10)
        self.h, self.ds, self._ref = {}, {}, {}

    def add(self, name, pts, exact=True):
        c = self.ctx.cloud_create(self.cfg, pts)
        if exact:
            assert int(c.info().m) == len(pts), (name, int(c.info().m), len(pts))
        self.h[name] = c
        self.refresh(name)
        return c

    def refresh(self, name):
        d = self.h[name].download()["ds"]
        self.ds[name] = d if d is not None else self.ctx.torch.zeros((0, 3), dtype=self.ctx.torch.float32, device=self.ctx.dev)

    def close(self):
        for c in self.h.values():
            c.close()

    def reference(self, s, t, Rt, thre):
        """(ratio, moved source) of ghicp_transform_cloud_f32 + ghicp_cal_overlap on the downloaded clouds"""
        M = np.eye(4) if Rt is None else Rt
        key = (s, t, M.tobytes(), thre)
        if key not in self._ref:
            moved = self.ctx.transform_cloud_f32(self.ds[s], np.ascontiguousarray(M, np.float64).astype(np.float32))
            self._ref[key] = (np.float32(self.ctx.cal_overlap(moved, self.ds[t], thre)), moved.cpu().numpy())
        return self._ref[key]

    def batch(self, pairs, thre, max_concurrent=0, with_poses=True):
        Rt = np.stack([np.eye(4) if p[2] is None else p[2] for p in pairs]) if with_poses and pairs else None
        return self.ctx.overlap_clouds([self.h[p[0]] for p in pairs], [self.h[p[1]] for p in pairs], thre, Rt, max_concurrent)


def ratio_of(hits, n):
    """(float)((0.01 + hits) / (double)n), common_reg.cpp:313; 0 for an empty source"""
    return np.float32((0.01 + int(hits)) / float(n)) if n > 0 else np.float32(0.0)


def assert_same_as_per_pair(w, pairs, thre, got):
    assert len(got["hits"]) == len(got["n"]) == len(got["ratio"]) == len(pairs)
    assert got["hits"].dtype == np.int64 and got["n"].dtype == np.int64 and got["ratio"].dtype == np.float32
    for p, (s, t, Rt) in enumerate(pairs):
        ratio, _ = w.reference(s, t, Rt, thre)
        n = len(w.ds[s])
        assert got["n"][p] == n
        assert got["ratio"][p] == ratio, "pair %d (%s in %s): ratio %r, the per-pair path gives %r" % (p, s, t, got["ratio"][p], ratio)
        assert got["ratio"][p] == ratio_of(got["hits"][p], n), "pair %d: hits %d do not give ratio %r" % (p, got["hits"][p], got["ratio"][p])
        assert 0 <= got["hits"][p] <= n


def assert_same_records(a, b):
    for k in ("hits", "n", "ratio"):
        np.testing.assert_array_equal(a[k], b[k])


def brute_hits(moved, tgt, thre):
    """float32 throughout, d2 formed as the kernel forms it: dx*dx; += dy*dy; += dz*dz"""
    if len(moved) == 0 or len(tgt) == 0:
        return 0
    r2 = np.float32(thre) * np.float32(thre)
    d = moved[:, None, :].astype(np.float32) - tgt[None, :, :].astype(np.float32)
    d2 = d[..., 0] * d[..., 0]
    d2 = d2 + d[..., 1] * d[..., 1]
    d2 = d2 + d[..., 2] * d[..., 2]
    assert d2.dtype == np.float32
    return int((d2 < r2).any(axis=1).sum())


# ------------------------------------------------------------------------------------------------ 1. block and wave edges in one batch
@pytest.fixture(scope="module")
def edges(ctx, api):
    rng = np.random.default_rng(11)
    w = Clouds(ctx, api)
    for n in SIZES:
        w.add("s%d" % n, cube(rng, n))
    for n in (300, 600):
        w.add("t%d" % n, cube(rng, n)).prepare_overlap(0.3)
    w.pairs = [("s%d" % n, "t%d" % m, small_pose(rng)) for n in SIZES for m in (300, 600)]
    yield w
    w.close()


def test_block_and_wave_edges_in_one_batch(edges, oracle):
    w, thre = edges, 0.3
    got = w.batch(w.pairs, thre)
    print("sizes", got["n"].tolist(), "hits", got["hits"].tolist())
    assert got["n"].tolist() == [n for n in SIZES for _ in range(2)]
    assert_same_as_per_pair(w, w.pairs, thre, got)
    assert 0 < got["hits"][-1] < 513 and 0 < got["hits"][-3] < 257  # the large sources are neither all in nor all out
    for p, (s, t, Rt) in enumerate(w.pairs):
        ratio, moved = w.reference(s, t, Rt, thre)
        tgt = w.ds[t].cpu().numpy()
        assert got["hits"][p] == brute_hits(moved, tgt, thre), p
        if len(moved):  # (the oracle, like the reference, divides by the size of the source: no answer for an empty one; the library's is 0)
            assert got["ratio"][p] == np.float32(oracle.cal_overlap(moved, tgt, thre)), p
        else:
            assert got["hits"][p] == 0 and got["ratio"][p] == 0.0
    # the same pairs in another order, and under every chunking, give the same records
    perm = np.random.default_rng(3).permutation(len(w.pairs))
    shuffled = w.batch([w.pairs[i] for i in perm], thre)
    for k in ("hits", "n", "ratio"):
        np.testing.assert_array_equal(shuffled[k], got[k][perm])
    n = len(w.pairs)
    for mc in (1, 2, n, n + 1):
        assert_same_records(w.batch(w.pairs, thre, mc), got)


# ------------------------------------------------------------------------------------------------ 2. the strict threshold
def test_threshold_is_strict(ctx, api):
    w = Clouds(ctx, api)
    try:
        w.add("T", np.array([[-60, -60, -60], [0, 0, 0], [60, 50, 40], [-30, 20, 55]], np.float32)).prepare_overlap(0.5)
        below = np.nextafter(np.float32(0.5), np.float32(0.0))
        assert below < np.float32(0.5) and np.float32(below * below) < np.float32(0.25)
        w.add("at", np.array([[0.5, 0, 0]], np.float32))
        w.add("below", np.array([[below, 0, 0]], np.float32))
        pairs = [("at", "T", None), ("below", "T", None)]
        for with_poses in (False, True):  # the identity as NULL and as an explicit matrix
            got = w.batch(pairs, 0.5, with_poses=with_poses)
            assert got["hits"].tolist() == [0, 1] and got["n"].tolist() == [1, 1]
            assert got["ratio"].tolist() == [np.float32(0.01), np.float32(1.01)]
            assert_same_as_per_pair(w, pairs, 0.5, got)
    finally:
        w.close()


# ------------------------------------------------------------------------------------------------ 3. 27-cell reach and the padded border
def test_neighbour_cells_and_the_padded_border(ctx, api):
    """Target box [0, 2]^3, cell 0.5: 5 cells per axis (the last one holds the face x = 2 alone); the padded grid ends one cell beyond."""
    thre = 0.5
    w = Clouds(ctx, api)
    try:
        tgt = np.array([[0, 0, 0], [2, 2, 2], [0.999, 1.2, 1.2], [0.999, 1.3, 0.7], [1.999, 0.3, 0.3]], np.float32)  # just inside the faces x = 1 and x = 2
        w.add("T", tgt).prepare_overlap(thre)
        cases = dict(
            neighbour=([1.2, 1.2, 1.2], 1),        # in the cell beyond the face x = 1, 0.201 from a target point: found through the 27 cells
            diagonal=([1.2, 1.55, 1.05], 1),       # a neighbour in x, y and z at once: 0.2, 0.25, 0.35 -> d = 0.474
            too_far=([1.45, 1.55, 1.05], 0),       # the same cells at 0.451, 0.25, 0.35 -> d = 0.622
            outside_hit=([2.3, 0.3, 0.3], 1),      # beyond the box, inside the padded grid: clamped to the last cell, 0.301 from (1.999, .3, .3)
            one_cell_out=([2.8, 1.0, 1.0], 0),     # one full cell outside the bounding box (fx = 5.6 <= 6): searched, nothing there
            below_box=([-0.4, 0.1, 0.1], 1),       # fx = -0.8 >= -1: searched, 0.424 from the corner point
            below_pad=([-0.8, 0.5, 0.5], 0),       # fx = -1.6: outside the padded grid
            far=([900.0, 1.0, 1.0], 0))            # 900 m away
        for name, (p, _) in cases.items():
            w.add(name, np.array([p], np.float32))
        allp = np.array([c[0] for c in cases.values()], np.float32)
        w.add("all", on_corner(np.concatenate([allp.min(axis=0, keepdims=True), allp])))  # + the corner of their box, (-0.8, 0.1, 0.1): outside the pad, a miss
        pairs = [(name, "T", None) for name in cases] + [("all", "T", None)]
        got = w.batch(pairs, thre)
        want = [c[1] for c in cases.values()]
        assert got["hits"].tolist() == want + [sum(want)], dict(zip(list(cases) + ["all"], got["hits"].tolist()))
        assert_same_as_per_pair(w, pairs, thre, got)
        # moved there by the pose instead of sitting there: the same answers
        shift = np.eye(4)
        shift[:3, 3] = (900.0, -3.0, 2.5)
        back = np.array([[p[0] - 900.0, p[1] + 3.0, p[2] - 2.5] for p, _ in cases.values()], np.float32)
        for name, p in zip(cases, back):
            w.add("m_" + name, p[None])
        moved_pairs = [("m_" + name, "T", shift) for name in cases]
        got_m = w.batch(moved_pairs, thre)
        assert_same_as_per_pair(w, moved_pairs, thre, got_m)
        assert got_m["hits"][-1] == 0 and got_m["hits"][4] == 0  # far and one_cell_out stay misses wherever the float rounding of the shift puts them
    finally:
        w.close()


# ------------------------------------------------------------------------------------------------ 4. sharing
def test_shared_targets_self_overlap_and_empty_sides(ctx, api):
    thre = 0.3
    rng = np.random.default_rng(21)
    w = Clouds(ctx, api)
    try:
        for name, n in (("A", 300), ("B", 600), ("C", 257), ("D", 64), ("E", 0)):
            w.add(name, cube(rng, n)).prepare_overlap(thre)
        poses = [small_pose(rng) for _ in range(6)]
        pairs = [("A", "B", poses[0]), ("C", "B", poses[1]), ("D", "B", poses[2]), ("A", "B", poses[3]), ("C", "B", None),  # one target, five pairs
                 ("B", "A", poses[4]),                                                                                       # B is a source and a target
                 ("B", "B", None), ("C", "C", None),                                                                        # a cloud in itself
                 ("A", "E", poses[5]), ("D", "E", None),                                                                    # empty target
                 ("E", "B", poses[0]), ("E", "E", None)]                                                                    # empty source
        got = w.batch(pairs, thre)
        print("hits", got["hits"].tolist(), "ratio", got["ratio"].tolist())
        assert_same_as_per_pair(w, pairs, thre, got)
        assert got["hits"][6] == got["n"][6] == 600 and got["hits"][7] == got["n"][7] == 257
        assert got["ratio"][6] == np.float32(600.01 / 600.0)
        assert got["hits"][8] == 0 and got["ratio"][8] == np.float32(0.01 / 300.0) and got["n"][8] == 300
        assert got["hits"][9] == 0 and got["ratio"][9] == np.float32(0.01 / 64.0)
        assert (got["hits"][10], got["n"][10], got["ratio"][10]) == (0, 0, 0.0) and (got["hits"][11], got["n"][11], got["ratio"][11]) == (0, 0, 0.0)
        assert got["hits"][0] != got["hits"][3]  # the pose matters
        assert_same_records(w.batch(pairs, thre, 5), got)
        # only pairs that launch nothing
        none = w.batch(pairs[8:], thre)
        for k in ("hits", "n", "ratio"):
            np.testing.assert_array_equal(none[k], got[k][8:])
        empty = w.batch([], thre)
        assert len(empty["hits"]) == 0
    finally:
        w.close()


# ------------------------------------------------------------------------------------------------ 5. a realistic pair
@pytest.fixture(scope="module")
def scans(ctx, api, synth):
    pair = synth.tls_pair(20_000, pair_id=11)
    w = Clouds(ctx, api, voxel=0.2)
    w.add("A", pair.source, exact=False)
    w.add("B", pair.target, exact=False)
    w.raw = dict(A=pair.source, B=pair.target)
    w.gt = pair.gt
    yield w
    w.close()


def test_scan_pair_at_the_truth_displaced_and_far(scans):
    w, thre = scans, 0.3
    w.h["B"].prepare_overlap(thre)
    pairs = [("A", "B", w.gt.copy()), ("A", "B", displaced(w.gt, 6.0, (1.2, 0.0, 0.0))), ("A", "B", displaced(w.gt, 0.0, (900.0, 0.0, 0.0)))]
    got = w.batch(pairs, thre)
    print("down-sampled", len(w.ds["A"]), len(w.ds["B"]), "hits", got["hits"].tolist(), "ratio", got["ratio"].tolist())
    assert len(w.ds["A"]) > 1024  # several blocks
    assert_same_as_per_pair(w, pairs, thre, got)
    assert got["ratio"][0] > got["ratio"][1] and got["hits"][2] == 0
    assert_same_records(w.batch(pairs, thre, 1), got)


# ------------------------------------------------------------------------------------------------ 6. the matrix
def pair_pose(Pi, Pj):
    """inv(P_j) * P_i of two rigid poses as include/ghicp_c.h states it: R_j^T R_i and R_j^T (t_i - t_j) in f64, every sum of three terms
    added left to right, bottom row 0 0 0 1"""
    Pi, Pj = np.asarray(Pi, np.float64), np.asarray(Pj, np.float64)
    M = np.zeros((4, 4))
    d = [Pi[k, 3] - Pj[k, 3] for k in range(3)]
    for r in range(3):
        for c in range(3):
            M[r, c] = (Pj[0, r] * Pi[0, c] + Pj[1, r] * Pi[1, c]) + Pj[2, r] * Pi[2, c]
        M[r, 3] = (Pj[0, r] * d[0] + Pj[1, r] * d[1]) + Pj[2, r] * d[2]
    M[3, 3] = 1.0
    return M


def test_matrix_is_overlap_clouds_on_the_stated_pair_poses(ctx, api):
    thre = 0.3
    rng = np.random.default_rng(31)
    world = rng.uniform(0.0, 4.0, (900, 3))
    w = Clouds(ctx, api)
    try:
        names, poses = ["c0", "c1", "c2", "c3"], []
        for i, name in enumerate(names):
            P = small_pose(rng, deg=40.0, shift=3.0)  # cloud -> world
            part = world[rng.permutation(len(world))[: 300 + 100 * i]]
            local = (part - P[:3, 3]) @ P[:3, :3]  # world -> cloud
            w.add(name, on_corner(local.astype(np.float32))).prepare_overlap(thre)
            poses.append(P)
        clouds = [w.h[n] for n in names]
        M = ctx.overlap_matrix(clouds, thre, np.stack(poses))
        assert M.shape == (4, 4) and M.dtype == np.float32
        ij = [(i, j) for i in range(4) for j in range(4) if i != j]
        pairs = [(names[i], names[j], pair_pose(poses[i], poses[j])) for i, j in ij]
        got = w.batch(pairs, thre)
        assert_same_as_per_pair(w, pairs, thre, got)
        for (i, j), r in zip(ij, got["ratio"]):
            assert M[i, j] == r, (i, j)
        np.testing.assert_array_equal(np.diag(M), np.ones(4, np.float32))
        print("matrix\n", M)
        assert (M[~np.eye(4, dtype=bool)] > 0.2).all()  # parts of one world under their true poses do overlap
        # no poses = all identity = the clouds as they lie
        M0 = ctx.overlap_matrix(clouds, thre)
        np.testing.assert_array_equal(M0, ctx.overlap_matrix(clouds, thre, np.stack([np.eye(4)] * 4)))
        plain = w.batch([(names[i], names[j], None) for i, j in ij], thre, with_poses=False)
        for (i, j), r in zip(ij, plain["ratio"]):
            assert M0[i, j] == r
        assert not np.array_equal(M0, M)
        np.testing.assert_array_equal(ctx.overlap_matrix(clouds[:1], thre), np.ones((1, 1), np.float32))
        # every handle is a target: one that is not prepared for this thre_dis is refused and nothing is written
        w.add("fresh", cube(rng, 100))
        for bad in ([w.h["fresh"]], clouds[:3] + [w.h["fresh"]]):
            H = (C.c_void_p * len(bad))(*[c.h.value for c in bad])
            out = np.full((len(bad), len(bad)), -7.0, np.float32)
            assert ctx.lib.ghicp_overlap_matrix(ctx.h, C.c_float(thre), len(bad), H, None, out.ctypes.data_as(C.c_void_p)) == 1
            assert (out == -7.0).all()
        with pytest.raises(api.GhicpError):
            ctx.overlap_matrix(clouds, 0.5)
    finally:
        w.close()


# ------------------------------------------------------------------------------------------------ 7. state of the handle
def raw_call(ctx, api, S, T, thre):
    """ghicp_overlap_clouds into a record array pre-filled with a sentinel: (return code, the records untouched?)"""
    n = len(S)
    res = (api.OverlapResult * n)()
    C.memset(res, 0xA5, C.sizeof(res))
    before = bytes(res)
    HS = (C.c_void_p * n)(*[c.h.value for c in S])
    HT = (C.c_void_p * n)(*[c.h.value for c in T])
    rc = ctx.lib.ghicp_overlap_clouds(ctx.h, C.c_float(thre), n, HS, HT, None, 0, res)
    return rc, bytes(res) == before


def test_refused_arguments_leave_the_output_untouched(ctx, api):
    rng = np.random.default_rng(41)
    w = Clouds(ctx, api)
    try:
        rawT = cube(rng, 400)
        S, T, U = w.add("S", cube(rng, 200)), w.add("T", rawT), w.add("U", cube(rng, 100))
        T.prepare_overlap(0.3)
        ok = w.batch([("S", "T", None)], 0.3)
        assert raw_call(ctx, api, [S, S], [T, U], 0.3) == (1, True)   # an unprepared target (the second pair: the first must not have been written)
        assert raw_call(ctx, api, [S], [T], 0.5) == (1, True)         # prepared for 0.3, asked for 0.5
        assert raw_call(ctx, api, [S], [T], np.nextafter(np.float32(0.3), np.float32(1.0))) == (1, True)  # the floats are compared exactly
        assert raw_call(ctx, api, [S], [T], 0.0) == (1, True) and raw_call(ctx, api, [S], [T], -0.3) == (1, True)
        assert raw_call(ctx, api, [S], [T], float("nan")) == (1, True)
        stored = ctx.cloud_from_features(w.cfg, T.download()["kp_xyz"], None, T.info().bbx_magnitude)  # holds no points
        with pytest.raises(api.GhicpError):
            stored.prepare_overlap(0.3)
        assert raw_call(ctx, api, [stored], [T], 0.3) == (1, True) and raw_call(ctx, api, [S], [stored], 0.3) == (1, True)
        stored.close()
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(api.GhicpError):
                U.prepare_overlap(bad)
        assert raw_call(ctx, api, [S], [U], 0.3) == (1, True)  # ... and a refused preparation prepares nothing
        T.prepare_overlap(0.5)  # another thre_dis replaces the grid
        assert raw_call(ctx, api, [S], [T], 0.3) == (1, True)
        assert_same_as_per_pair(w, [("S", "T", None)], 0.5, w.batch([("S", "T", None)], 0.5))
        T.prepare_overlap(0.3)
        T.prepare_overlap(0.3)  # the same again: nothing happens
        assert_same_records(w.batch([("S", "T", None)], 0.3), ok)
        T.recompute(rawT)  # forgets the grid, until it is prepared again
        assert raw_call(ctx, api, [S], [T], 0.3) == (1, True)
        T.prepare_overlap(0.3)
        assert_same_records(w.batch([("S", "T", None)], 0.3), ok)
        assert raw_call(ctx, api, [S], [T], 0.3)[0] == 0  # and the context is as good as before
    finally:
        w.close()


def test_prepare_refine_and_prepare_gicp_keep_the_overlap_grid_and_the_other_way_round(scans, ctx, api):
    """One pair of test_gpu_refine.py's kind through ctx.refine_clouds before and after the target is prepared for the overlap, and the
    overlap before and after the target is prepared for the two refiners: neither disturbs the other."""
    w, thre, KN = scans, 0.3, 12
    A = w.h["A"]
    init = displaced(w.gt, 0.5, (0.08, -0.05, 0.02))
    prm = params_of(api, 1, True, max_iter=3, k=KN)  # point-to-plane needs the target's normals, the trimmed gate runs its own overlap
    B = ctx.cloud_create(w.cfg, w.raw["B"])          # a fresh handle of the target: nothing prepared
    B2 = ctx.cloud_create(w.cfg, w.raw["B"])
    try:
        def refine(T):
            (r,) = ctx.refine_clouds(prm, [(A, T)], init[None])
            return r

        def overlap(T):
            return ctx.overlap_clouds([A], [T], thre, init[None])

        def same_refine(x, y):
            for k in STAT_KEYS:
                assert x[k] == y[k], k
            np.testing.assert_array_equal(x["T"], y["T"])
            np.testing.assert_array_equal(x["Rt_refined"], y["Rt_refined"])

        B.prepare_refine(KN)
        r0 = refine(B)
        assert r0["done"] == 1 and r0["iterations"] >= 1
        with pytest.raises(api.GhicpError):  # prepare_refine builds no overlap grid
            overlap(B)
        B.prepare_overlap(thre)
        o0 = overlap(B)
        assert_same_as_per_pair(w, [("A", "B", init)], thre, o0)
        assert 0 < o0["hits"][0] < o0["n"][0]
        same_refine(refine(B), r0)          # prepare_overlap left the grids and normals alone
        B.prepare_gicp(10, 1e-3)
        B.prepare_refine(KN)
        assert_same_records(overlap(B), o0)  # both keep the overlap grid
        same_refine(refine(B), r0)
        # the other order: overlap first, then the refiners' state
        B2.prepare_overlap(thre)
        with pytest.raises(api.GhicpError):  # prepare_overlap builds no 1-NN grids
            refine(B2)
        assert_same_records(overlap(B2), o0)
        B2.prepare_gicp(10, 1e-3)
        B2.prepare_refine(KN)
        same_refine(refine(B2), r0)
        assert_same_records(overlap(B2), o0)
        ctx.clouds_recompute([B2], [w.raw["B"]])  # the batched front end forgets the grid, as ghicp_cloud_recompute does
        with pytest.raises(api.GhicpError):
            overlap(B2)
        B2.prepare_overlap(thre)
        assert_same_records(overlap(B2), o0)
    finally:
        B.close()
        B2.close()
