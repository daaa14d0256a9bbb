"""Generalized ICP from an initial pose (ghicp_gicp_from) and its batched form over cached clouds (ghicp_cloud_prepare_gicp /
ghicp_gicp_clouds).  The single-pair call is held to an independent CPU check of its guess semantics (covariances in the source's own
frame, search on the moved points) and to the ground-truth bounds of test_gpu_gicp.py; every pair of a batch must then come out exactly as
ghicp_gicp_from gives it on the downloaded clouds, whatever the other pairs of its chunk do.  The pairs finish after different numbers of
outer iterations on purpose: a pair that has left its loop must be left alone while its neighbours go on.

The tests over the three cached scans (all-pairs, multi-view registration) carry `multiview` in their names.  On the host SIMT interpreter
every inner step of every pair is 512 workgroups, so they take one to two minutes each there; tests/test_sim_cpu.py leaves tests of that
name to the GPU and to a direct `GHICP_SIM=1 pytest tests/test_gpu_gicp_clouds.py -m gpu`.  The single-pair tests and the launch-edge batch
are light and run in its sweep as well."""
import numpy as np
import pytest

import gicp_restatement as G
from conftest import rot_err, trans_err
from test_gpu_refine import STAT_KEYS, World, displaced, lattice
from test_gpu_refine import params_of as icp_params_of
from test_icp_cpu import small_pair

pytestmark = pytest.mark.gpu

MAX_ITER = 6
INNER = 4
K = 10
EPS = 1e-3
# Convergence thresholds of the batch tests: with the reference's 1e-8 m / 1e-6 no pair of these noisy scans settles within MAX_ITER outer
# iterations; at 1e-4 m / 1e-4 the pairs that start near the truth stop after a few and the far pair runs into max_iter.  Which pair stops
# when is asserted, not assumed (test_multiview_batch_is_bit_identical_to_the_per_pair_path).
TEPS, REPS = 1e-4, 1e-4


def gparams(api, trimmed, max_iter=MAX_ITER, k=K, thre_dis=0.3, max_dist=1e6, teps=TEPS, reps=REPS):
    p = api.gicp_params(max_iter, False, trimmed, thre_dis, 0.1, k, max_dist, INNER)
    p.gicp_epsilon, p.transformation_epsilon, p.rotation_epsilon = EPS, teps, reps
    return p


def f32(M):
    return np.ascontiguousarray(M, np.float64).astype(np.float32)


class GWorld(World):
    """test_gpu_refine's three cached clouds and pairs, with the per-pair GICP results (ghicp_gicp_from on the downloaded clouds), computed
    once per parameter set and never changed."""

    def __init__(self, ctx, api, synth):
        super().__init__(ctx, api, synth)
        self._gref = {}
        self.gprepared = None

    def prepare_gicp(self, k=K, eps=EPS):
        if self.gprepared != (k, eps):
            for c in self.clouds.values():
                c.prepare_gicp(k, eps)
            self.gprepared = (k, eps)

    def gicp_reference(self, trimmed, pair):
        s, t, init = pair
        key = (trimmed, s, t, None if init is None else init.tobytes())
        if key not in self._gref:
            self._gref[key] = self.ctx.gicp(self.ds[s], self.ds[t], gparams(self.api, trimmed), want_transformed=False,
                                            guess=None if init is None else f32(init))
        return self._gref[key]

    def gicp_batch(self, trimmed, pairs, max_concurrent=0, with_init=True):
        self.prepare_gicp()
        return self.ctx.gicp_clouds(gparams(self.api, trimmed), [(self.clouds[s], self.clouds[t]) for s, t, _ in pairs],
                                    np.stack([p[2] for p in pairs]) if with_init else None, max_concurrent)


@pytest.fixture(scope="module")
def world(ctx, api, synth):
    w = GWorld(ctx, api, synth)
    yield w
    for c in w.clouds.values():
        c.close()


def assert_same_as_per_pair(world, trimmed, pairs, got):
    assert len(got) == len(pairs)
    for p, (pair, g) in enumerate(zip(pairs, got)):
        r = world.gicp_reference(trimmed, pair)
        for k in STAT_KEYS:
            assert g[k] == r[k], "pair %d: %s = %r, the per-pair path gives %r" % (p, k, g[k], r[k])
        if r["done"]:
            np.testing.assert_array_equal(g["T"], r["T"])
        else:  # ghicp_gicp_from leaves T untouched when it refuses; the batch reports the rounded init
            np.testing.assert_array_equal(g["T"], np.eye(4, dtype=np.float32) if pair[2] is None else f32(pair[2]))
        np.testing.assert_array_equal(g["Rt_refined"], g["T"].astype(np.float64))


def assert_same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for k in STAT_KEYS:
            assert x[k] == y[k], k
        np.testing.assert_array_equal(x["T"], y["T"])


# ------------------------------------------------------------------------------------------------ 1. the single-pair call
def _same_single(a, b):
    for k in STAT_KEYS:
        assert a[k] == b[k], k
    np.testing.assert_array_equal(a["T"], b["T"])
    np.testing.assert_array_equal(a["transformed"].cpu().numpy(), b["transformed"].cpu().numpy())


@pytest.fixture(scope="module")
def small(synth):
    return small_pair(synth)


def test_identity_guess_is_the_call_without_a_guess(ctx, api, small):
    src, tgt, _ = small
    for trimmed in (False, True):
        prm = gparams(api, trimmed, thre_dis=0.2)
        _same_single(ctx.gicp(src, tgt, prm, guess=np.eye(4)), ctx.gicp(src, tgt, prm))


def test_guess_moves_the_points_and_keeps_the_covariances_in_the_source_frame(ctx, api, oracle, small):
    """One outer iteration from a guess: the correspondences are those of the CPU restatement given the covariances of the UNMOVED clouds and
    the guess as transformation_ (it searches from the moved points and rotates C_S by the guess's R)."""
    src, tgt, gt = small
    guess32 = f32(displaced(gt, 3.0, (0.2, -0.15, 0.05)))
    covS, covT = G.covariances(oracle, src, K, EPS), G.covariances(oracle, tgt, K, EPS)
    max_dist = 0.15
    si, _, _ = G.correspondences(oracle, src, tgt, covS, covT, guess32, max_dist)
    print("correspondences within %.2f m of the guess-moved source: %d of %d" % (max_dist, len(si), len(src)))
    assert 0 < len(si) < len(src)  # some but not all points are kept
    r = ctx.gicp(src, tgt, gparams(api, False, max_iter=1, max_dist=max_dist), guess=guess32)
    assert r["done"] == 1 and r["iterations"] == 1
    assert r["correspondences"] == len(si)
    assert len(G.correspondences(oracle, src, tgt, covS, covT, np.eye(4, dtype=np.float32), max_dist)[0]) != len(si)  # the guess matters


@pytest.mark.parametrize("off", [(0.5, (0.08, -0.05, 0.02)), (0.0, (0.0, 0.0, 0.0))])  # the displaced poses of the close pairs of the batch
def test_from_a_displaced_pose_within_the_ground_truth_bounds(ctx, api, small, off):
    src, tgt, gt = small
    for trimmed in (False, True):
        r = ctx.gicp(src, tgt, gparams(api, trimmed, thre_dis=0.2, teps=1e-8, reps=1e-6), guess=displaced(gt, *off))
        T = r["T"].astype(np.float64)
        print("from %r trimmed=%d: iterations %d reason %d rot_err %.2e trans_err %.2e" % (off, trimmed, r["iterations"], r["reason"], rot_err(T, gt), trans_err(T, gt)))
        assert r["done"] == 1
        assert rot_err(T, gt) < 2e-3 and trans_err(T, gt) < 0.02  # the bounds of test_gpu_gicp.py against ground truth
        np.testing.assert_array_equal(r["transformed"].cpu().numpy(), ctx.transform_cloud_f32(src, r["T"]).cpu().numpy())  # transformed = T16 * S


def test_refusal_is_decided_on_the_moved_source(ctx, api, small):
    src, tgt, gt = small
    prm = gparams(api, True, thre_dis=0.2)
    far = gt.copy()
    far[0, 3] += 900.0
    r = ctx.gicp(src, tgt, prm, guess=far)
    assert r["done"] == 0 and r["overlap"] < 0.1 and r["iterations"] == 0 and not r["T"].any()  # T untouched
    assert ctx.gicp(src, tgt, prm, guess=np.eye(4))["done"] == 1
    # the gate is calOverlap of the moved source
    g32 = f32(displaced(gt, 0.5, (0.08, -0.05, 0.02)))
    assert ctx.gicp(src, tgt, prm, guess=g32)["overlap"] == ctx.cal_overlap(ctx.transform_cloud_f32(src, g32), tgt, 0.2)


def test_fewer_than_four_correspondences_return_the_guess(ctx, api, small):
    src, tgt, gt = small
    g32 = f32(displaced(gt, 0.5, (0.08, -0.05, 0.02)))
    r = ctx.gicp(src[:3], tgt, gparams(api, False), guess=g32)
    assert (r["done"], r["converged"], r["reason"], r["iterations"], r["correspondences"]) == (1, 0, 5, 0, 3)
    np.testing.assert_array_equal(r["T"], g32)
    np.testing.assert_array_equal(r["transformed"].cpu().numpy(), ctx.transform_cloud_f32(src[:3], g32).cpu().numpy())


def test_bad_guesses_are_argument_errors(ctx, api, small):
    src, tgt, _ = small
    prm = gparams(api, False)
    for i, v in ((1, np.nan), (7, np.inf), (12, 1e-3), (15, 0.5)):
        g = np.eye(4, dtype=np.float32).reshape(16).copy()
        g[i] = v
        with pytest.raises(api.GhicpError):
            ctx.gicp(src, tgt, prm, guess=g)
    assert ctx.gicp(src[:50], tgt, prm, guess=np.eye(4))["done"] == 1  # and the context is as good as before


# ------------------------------------------------------------------------------------------------ 2. batch = per pair
@pytest.mark.parametrize("trimmed", [False, True])
def test_multiview_batch_is_bit_identical_to_the_per_pair_path(world, trimmed):
    pairs = list(world.pairs) + ([world.refused] if trimmed else [])
    got = world.gicp_batch(trimmed, pairs)
    its = [g["iterations"] for g in got if g["done"]]
    print("iterations per pair:", its, "reasons:", [g["reason"] for g in got], "overlap:", [g["overlap"] for g in got])
    assert len(set(its)) > 1, "every pair ran %r iterations: the fixture no longer tests the freeze" % its
    assert got[4]["reason"] == 1 and got[4]["iterations"] == MAX_ITER and min(its) < MAX_ITER  # stopped by max_iter next to converged pairs
    assert_same_as_per_pair(world, trimmed, pairs, got)
    if trimmed:
        assert got[-1]["done"] == 0 and all(g["done"] == 1 for g in got[:-1])
        assert all(got[p]["overlap"] > 0.1 for p in range(5))
    for p in world.close:
        s, t, _ = pairs[p]
        Rt = got[p]["Rt_refined"]
        print("pair %d: rot_err %.2e trans_err %.2e" % (p, rot_err(Rt, world.gt[s, t]), trans_err(Rt, world.gt[s, t])))


def test_multiview_batch_without_initial_poses_is_ghicp_gicp_per_pair(world):
    pairs = [world.pairs[3], world.pairs[1]]  # (C, B) twice
    got = world.gicp_batch(False, pairs, with_init=False)
    assert_same_as_per_pair(world, False, [(s, t, None) for s, t, _ in pairs], got)
    assert_same_results(got[:1], got[1:])


# ------------------------------------------------------------------------------------------------ 3. independence from chunking
def test_multiview_results_do_not_depend_on_the_chunking(world):
    whole = world.gicp_batch(True, world.pairs, 0)
    assert len(set(g["iterations"] for g in whole)) > 1
    assert_same_results(world.gicp_batch(True, world.pairs, 1), whole)
    assert_same_results(world.gicp_batch(True, world.pairs, 2), whole)  # chunks of 2, 2, 1


def test_multiview_a_refused_pair_leaves_its_neighbours_alone(world):
    pairs = list(world.pairs[:3])
    pairs.insert(1, world.refused)
    got = world.gicp_batch(True, pairs, 3)  # the refused pair shares a chunk with pairs 0 and 2
    r = got[1]
    assert r["done"] == 0 and r["iterations"] == 0 and r["overlap"] < 0.1
    np.testing.assert_array_equal(r["T"], f32(world.refused[2]))
    assert r["overlap"] == world.gicp_reference(True, world.refused)["overlap"]
    assert_same_results(got[:1] + got[2:], world.gicp_batch(True, world.pairs[:3], 3))


# ------------------------------------------------------------------------------------------------ 4. edges of the 2-D launch
def test_edges_of_the_two_dimensional_launch(ctx, api):
    cfg = api.pair_config(api.FEATURE_NONE, api.CORR_NN, dof=6, voxel=0.2, max_iter=10)
    tgt = lattice(3000, 1)
    init = displaced(np.eye(4), 0.3, (0.03, -0.02, 0.01))
    inv = np.linalg.inv(init)
    # < 4; one block; just into the second block; ten blocks.  (The voxel filter keeps its first input point once more unless a point falls
    # into the corner voxel, so m is n or n + 1: the classes are asserted on the m the handles report.)
    sizes = [2, 100, 257, 2500]
    rng = np.random.default_rng(2)
    raws = [((tgt[rng.permutation(len(tgt))[:n]].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3])).astype(np.float32) for n in sizes]
    clouds = [ctx.cloud_create(cfg, x) for x in raws + [tgt]]
    try:
        ms = [int(c.info().m) for c in clouds]
        print("down-sampled sizes:", ms)
        assert ms[0] < 4 and 4 <= ms[1] <= 256 and 257 <= ms[2] <= 258 and ms[3] > 2048 and ms[4] > 2048
        for c in clouds:
            c.prepare_gicp(K, EPS)
        prm = gparams(api, False, max_dist=0.4)
        T = clouds[4]
        # the small pairs sit between and after large ones: the blocks beyond their cdiv(ns, 256) must do nothing
        order = [3, 0, 1, 3, 2, 0]
        inits = np.stack([init] * len(order))
        got = ctx.gicp_clouds(prm, [(clouds[i], T) for i in order], inits)
        tds = T.download()["ds"]
        for i, g in zip(order, got):
            r = ctx.gicp(clouds[i].download()["ds"], tds, prm, want_transformed=False, guess=f32(init))
            for k in STAT_KEYS:
                assert g[k] == r[k], (ms[i], k, g[k], r[k])
            np.testing.assert_array_equal(g["T"], r["T"])
        small = got[1]
        assert (small["done"], small["reason"], small["iterations"], small["converged"], small["correspondences"]) == (1, 5, 0, 0, ms[0])
        np.testing.assert_array_equal(small["T"], f32(init))
        assert all(g["iterations"] >= 1 and g["correspondences"] >= 4 for i, g in zip(order, got) if i != 0)
        assert_same_results(ctx.gicp_clouds(prm, [(clouds[i], T) for i in order], inits, 2), got)
    finally:
        for c in clouds:
            c.close()


# ------------------------------------------------------------------------------------------------ 5. state of the handle
def test_multiview_prepare_again_other_parameters_and_prepare_refine(world, ctx, api):
    two = [world.pairs[1], world.pairs[3]]  # both onto B
    first = world.gicp_batch(True, two)
    for c in world.clouds.values():
        c.prepare_gicp(K, EPS)  # twice: nothing changes
    assert_same_results(world.gicp_batch(True, two), first)
    world.clouds["B"].prepare_gicp(K + 1, EPS)  # other covariances replace the old ones
    with pytest.raises(api.GhicpError):
        ctx.gicp_clouds(gparams(api, True), [(world.clouds["C"], world.clouds["B"])], two[0][2][None])
    world.clouds["B"].prepare_gicp(K, 2 * EPS)
    with pytest.raises(api.GhicpError):
        ctx.gicp_clouds(gparams(api, True), [(world.clouds["C"], world.clouds["B"])], two[0][2][None])
    world.clouds["B"].prepare_gicp(K, EPS)
    assert_same_results(world.gicp_batch(True, two), first)
    # prepare_refine after prepare_gicp keeps the covariances, prepare_gicp after prepare_refine keeps the normals: an ICP batch and a GICP
    # batch on the same handles both still match their per-pair paths
    KN = 12
    key = (1, True)  # point-to-plane needs the normals
    for c in world.clouds.values():
        c.prepare_refine(KN)
    assert_same_results(world.gicp_batch(True, two), first)
    for c in world.clouds.values():
        c.prepare_gicp(K + 2, EPS)
        c.prepare_gicp(K, EPS)
    prm = icp_params_of(api, *key, max_iter=3, k=KN)
    got = ctx.refine_clouds(prm, [(world.clouds[s], world.clouds[t]) for s, t, _ in two], np.stack([p[2] for p in two]))
    for (s, t, init), g in zip(two, got):
        r = ctx.icp(ctx.transform_cloud_f32(world.ds[s], f32(init)), world.ds[t], prm, want_transformed=False)
        for k in STAT_KEYS:
            assert g[k] == r[k], k
        np.testing.assert_array_equal(g["T"], r["T"])
    assert_same_as_per_pair(world, True, two, world.gicp_batch(True, two))


def test_multiview_errors_leave_nothing_half_written(world, ctx, api):
    pairs = world.pairs
    world.prepare_gicp()
    handles = [(world.clouds[s], world.clouds[t]) for s, t, _ in pairs]
    inits = np.stack([p[2] for p in pairs])
    prm = gparams(api, True)
    fresh = ctx.cloud_create(world.cfg, world.raw["B"])
    try:
        with pytest.raises(api.GhicpError):  # an unprepared target (last pair: the earlier ones must not have been started)
            ctx.gicp_clouds(prm, handles[:2] + [(world.clouds["A"], fresh)], inits[:3])
        with pytest.raises(api.GhicpError):  # an unprepared source
            ctx.gicp_clouds(prm, handles[:2] + [(fresh, world.clouds["B"])], inits[:3])
        fresh.prepare_refine(0)  # grids alone are not enough
        with pytest.raises(api.GhicpError):
            ctx.gicp_clouds(prm, [(world.clouds["A"], fresh)], inits[:1])
        d = fresh.download()
        stored = ctx.cloud_from_features(world.cfg, d["kp_xyz"], None, fresh.info().bbx_magnitude)
        with pytest.raises(api.GhicpError):  # no points in a handle rebuilt from stored features
            stored.prepare_gicp(K, EPS)
        with pytest.raises(api.GhicpError):
            ctx.gicp_clouds(prm, handles[:1] + [(stored, world.clouds["B"])], inits[:2])
        stored.close()
        for bad in ((0, EPS), (21, EPS), (K, 0.0)):
            with pytest.raises(api.GhicpError):
                fresh.prepare_gicp(*bad)
        fresh.prepare_gicp(K, EPS)
        ok = ctx.gicp_clouds(prm, [(world.clouds["C"], fresh)], inits[1:2])  # fresh holds B
        fresh.recompute(world.raw["B"])
        with pytest.raises(api.GhicpError):  # recompute invalidates the covariances
            ctx.gicp_clouds(prm, [(world.clouds["C"], fresh)], inits[1:2])
        fresh.prepare_gicp(K, EPS)
        ctx.clouds_recompute([fresh], [world.raw["B"]])
        with pytest.raises(api.GhicpError):
            ctx.gicp_clouds(prm, [(world.clouds["C"], fresh)], inits[1:2])
        fresh.prepare_gicp(K, EPS)
        assert_same_results(ctx.gicp_clouds(prm, [(world.clouds["C"], fresh)], inits[1:2]), ok)
        assert_same_as_per_pair(world, True, [pairs[1]], ok)
    finally:
        fresh.close()
    again = [pairs[1], pairs[3]]
    assert_same_as_per_pair(world, True, again, world.gicp_batch(True, again))  # and the context is as good as before
