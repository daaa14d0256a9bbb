"""Batched fine registration over cached clouds (ghicp_cloud_prepare_refine / ghicp_refine_clouds): every pair of a batch must come out
exactly as the per-pair path gives it -- ghicp_cloud_download, ghicp_transform_cloud_f32 with the float-rounded initial pose, ghicp_icp --
whatever the other pairs of its chunk do.  The pairs below finish after different numbers of iterations on purpose: a pair that has
converged must be left alone while its neighbours go on (the single-pair loop simply stops launching)."""
import numpy as np
import pytest

from conftest import rot_err, trans_err

pytestmark = pytest.mark.gpu

MAX_ITER = 8
K = 12
STAT_KEYS = ("done", "iterations", "converged", "reason", "correspondences", "overlap", "mse", "fitness")


def displaced(gt, deg, t):
    a = np.deg2rad(deg)
    d = np.eye(4)
    d[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    d[:3, 3] = t
    return d @ gt


def params_of(api, metric, trimmed, max_iter=MAX_ITER, reciprocal=False, k=K):
    return api.icp_params(max_iter, reciprocal, trimmed, metric, 0.3, 0.1, k)


def product_f64(T32, init64):
    """double(T_icp) * double(float(Rt_init)), the four terms of every entry added in order (as the library's host code does)."""
    a, b = T32.astype(np.float64), init64.astype(np.float32).astype(np.float64)
    out = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += float(a[i, k]) * float(b[k, j])
            out[i, j] = s
    return out


class World:
    """Three cached clouds (A, B: one scan pair; C: a displaced, thinned, noisy copy of B), the pairs with their initial poses, and the
    per-pair reference results, computed once per parameter set and never changed."""

    def __init__(self, ctx, api, synth):
        self.ctx, self.api = ctx, api
        pair = synth.tls_pair(60_000, pair_id=11)
        rng = np.random.default_rng(5)
        a = np.deg2rad(2.0)
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        t = np.array([0.10, -0.05, 0.02])
        B = pair.target[:, :3]
        C = ((B.astype(np.float64) - t) @ R).astype(np.float32)
        C = C[rng.permutation(len(C))[: int(0.8 * len(C))]]
        C = (C + rng.normal(0, 0.003, C.shape)).astype(np.float32)
        gt_cb = np.eye(4)
        gt_cb[:3, :3], gt_cb[:3, 3] = R, t
        self.raw = dict(A=pair.source, B=pair.target, C=C)
        self.gt = {("A", "B"): pair.gt, ("B", "A"): np.linalg.inv(pair.gt), ("C", "B"): gt_cb}
        self.cfg = api.pair_config(api.FEATURE_NONE, api.CORR_NN, dof=6, voxel=0.2, max_iter=10)
        self.clouds = {k: ctx.cloud_create(self.cfg, v) for k, v in self.raw.items()}
        self.ds = {k: c.download()["ds"] for k, c in self.clouds.items()}
        self.prepared = None
        # two pairs share the target B; B is a source and a target; the sources differ in size; (C, B) comes twice with different poses --
        # once at the truth (a few iterations), once half a degree / 0.1 m off; the scan pair starts close to its truth in both directions;
        # the last pair starts far off and is stopped by max_iter.  (Few iterations per pair on purpose: on the host interpreter every
        # iteration of a pair is 512 workgroups per accumulation kernel, whatever the size of the clouds.)
        self.pairs = [("A", "B", displaced(self.gt["A", "B"], 0.1, (0.02, -0.01, 0.0))),
                      ("C", "B", displaced(self.gt["C", "B"], 0.5, (0.08, -0.05, 0.02))),
                      ("B", "A", displaced(self.gt["B", "A"], -0.1, (0.02, -0.01, 0.0))),
                      ("C", "B", self.gt["C", "B"].copy()),
                      ("A", "B", displaced(self.gt["A", "B"], 6.0, (1.2, -0.8, 0.1)))]
        self.close = [1, 3]
        self.refused = ("A", "B", displaced(self.gt["A", "B"], 0.0, (900.0, 0.0, 0.0)))
        self._ref = {}

    def prepare(self, k):
        if self.prepared != k:
            for c in self.clouds.values():
                c.prepare_refine(k)
            self.prepared = k

    def reference(self, prm_key, pair):
        """ctx.icp on the downloaded clouds: what one ghicp_icp call per pair gives."""
        s, t, init = pair
        key = (prm_key, s, t, init.tobytes())
        if key not in self._ref:
            prm = params_of(self.api, *prm_key)
            src = self.ctx.transform_cloud_f32(self.ds[s], init.astype(np.float32))
            self._ref[key] = self.ctx.icp(src, self.ds[t], prm, want_transformed=False)
        return self._ref[key]

    def refine(self, prm_key, pairs, max_concurrent=0):
        self.prepare(K)
        prm = params_of(self.api, *prm_key)
        return self.ctx.refine_clouds(prm, [(self.clouds[s], self.clouds[t]) for s, t, _ in pairs], np.stack([p[2] for p in pairs]), max_concurrent)


@pytest.fixture(scope="module")
def world(ctx, api, synth):
    w = World(ctx, api, synth)
    yield w
    for c in w.clouds.values():
        c.close()


def assert_same_as_reference(world, prm_key, pairs, got):
    assert len(got) == len(pairs)
    for p, (pair, g) in enumerate(zip(pairs, got)):
        r = world.reference(prm_key, pair)
        for k in STAT_KEYS:
            assert g[k] == r[k], "pair %d: %s = %r, the per-pair path gives %r" % (p, k, g[k], r[k])
        init = pair[2]
        if r["done"]:
            np.testing.assert_array_equal(g["T"], r["T"])
        else:  # ghicp_icp leaves T untouched when it refuses; the batch reports the identity
            np.testing.assert_array_equal(g["T"], np.eye(4, dtype=np.float32))
        np.testing.assert_array_equal(g["Rt_refined"], product_f64(g["T"], init))


def assert_same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for k in STAT_KEYS:
            assert x[k] == y[k], k
        np.testing.assert_array_equal(x["T"], y["T"])
        np.testing.assert_array_equal(x["Rt_refined"], y["Rt_refined"])


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("trimmed", [False, True])
def test_batch_is_bit_identical_to_the_per_pair_path(world, metric, trimmed):
    key = (metric, trimmed)
    pairs = list(world.pairs) + ([world.refused] if trimmed else [])
    got = world.refine(key, pairs)
    its = [g["iterations"] for g in got if g["done"]]
    print("iterations per pair:", its, "reasons:", [g["reason"] for g in got], "overlap:", [g["overlap"] for g in got])
    assert len(set(its)) > 1, "every pair ran %r iterations: the fixture no longer tests the freeze" % its
    assert got[4]["reason"] == 1 and got[4]["iterations"] == MAX_ITER and min(its) < MAX_ITER  # stopped by max_iter next to converged pairs
    assert_same_as_reference(world, key, pairs, got)
    if trimmed:
        assert got[-1]["done"] == 0 and all(g["done"] == 1 for g in got[:-1])
        # the trimmed rejector is at work in the displaced pairs; the pair that starts at the truth has every point inside the radius
        # (ratio (0.01 + n) / n > 1) and runs untrimmed, as in ghicp_icp
        assert all(0.0 < got[p]["overlap"] < 1.0 for p in (0, 1, 2, 4)) and got[3]["overlap"] >= 1.0
        for p in world.close:  # the bounds of test_icp_matches_cpu against ground truth
            s, t, _ = pairs[p]
            Rt = got[p]["Rt_refined"]
            print("pair %d: rot_err %.2e trans_err %.2e" % (p, rot_err(Rt, world.gt[s, t]), trans_err(Rt, world.gt[s, t])))
            assert rot_err(Rt, world.gt[s, t]) < 2e-3 and trans_err(Rt, world.gt[s, t]) < 0.02


def test_results_do_not_depend_on_the_chunking(world):
    key = (0, True)
    whole = world.refine(key, world.pairs, 0)
    assert len(set(g["iterations"] for g in whole)) > 1
    assert_same_results(world.refine(key, world.pairs, 1), whole)
    assert_same_results(world.refine(key, world.pairs, 2), whole)  # chunks of 2, 2, 1


def test_a_refused_pair_leaves_its_neighbours_alone(world):
    key = (0, True)
    pairs = list(world.pairs[:3])
    pairs.insert(1, world.refused)
    got = world.refine(key, pairs, 3)  # the refused pair shares a chunk with pairs 0 and 2
    r = got[1]
    assert r["done"] == 0 and r["iterations"] == 0 and r["overlap"] < 0.1
    np.testing.assert_array_equal(r["T"], np.eye(4, dtype=np.float32))
    np.testing.assert_array_equal(r["Rt_refined"], world.refused[2].astype(np.float32).astype(np.float64))
    assert r["overlap"] == world.reference(key, world.refused)["overlap"]
    assert_same_results(got[:1] + got[2:], world.refine(key, world.pairs[:3], 3))


def test_errors_leave_nothing_half_written(world, ctx, api, synth):
    key = (1, True)
    pairs = world.pairs
    handles = [(world.clouds[s], world.clouds[t]) for s, t, _ in pairs]
    inits = np.stack([p[2] for p in pairs])
    fresh = ctx.cloud_create(world.cfg, world.raw["B"])
    try:
        with pytest.raises(api.GhicpError):  # a target that was never prepared (last pair: the earlier ones must not have been started)
            ctx.refine_clouds(params_of(api, 0, True), handles[:2] + [(world.clouds["A"], fresh)], inits[:3])
        world.prepare(K)
        with pytest.raises(api.GhicpError):  # normals for another k
            ctx.refine_clouds(params_of(api, 1, True, k=K + 1), handles, inits)
        fresh.prepare_refine(0)
        ctx.refine_clouds(params_of(api, 0, True), [(world.clouds["A"], fresh)], inits[:1])  # point-to-point needs no normals
        with pytest.raises(api.GhicpError):  # point-to-plane on a target prepared without normals
            ctx.refine_clouds(params_of(api, 1, True), [(world.clouds["A"], fresh)], inits[:1])
        with pytest.raises(api.GhicpError):
            ctx.refine_clouds(params_of(api, 0, True, reciprocal=True), handles, inits)
        d = fresh.download()
        stored = ctx.cloud_from_features(world.cfg, d["kp_xyz"], None, fresh.info().bbx_magnitude)
        with pytest.raises(api.GhicpError):  # no points in a handle rebuilt from stored features
            stored.prepare_refine(0)
        with pytest.raises(api.GhicpError):
            ctx.refine_clouds(params_of(api, 0, True), [(stored, fresh)], inits[:1])
        stored.close()
        fresh.prepare_refine(K)
        fresh.recompute(world.raw["B"])
        with pytest.raises(api.GhicpError):  # recompute invalidates the prepared state
            ctx.refine_clouds(params_of(api, 1, True), [(world.clouds["A"], fresh)], inits[:1])
        ctx.clouds_recompute([fresh], [world.raw["B"]])
        with pytest.raises(api.GhicpError):
            ctx.refine_clouds(params_of(api, 0, True), [(world.clouds["A"], fresh)], inits[:1])
    finally:
        fresh.close()
    again = [pairs[1], pairs[3]]
    assert_same_as_reference(world, key, again, world.refine(key, again))  # and the context is as good as before


def test_prepare_again_and_after_recompute(world, ctx, api):
    key = (1, True)
    two = [world.pairs[1], world.pairs[3]]  # both onto B
    first = world.refine(key, two)
    for c in world.clouds.values():
        c.prepare_refine(K)  # twice: nothing changes
    assert_same_results(world.refine(key, two), first)
    world.clouds["B"].prepare_refine(5)  # other normals, the grids are kept
    world.clouds["B"].prepare_refine(K)
    assert_same_results(world.refine(key, two), first)
    # a handle that held A becomes B: prepared again, it serves as the target B
    h = ctx.cloud_create(world.cfg, world.raw["A"])
    try:
        h.prepare_refine(K)
        h.recompute(world.raw["B"])
        h.prepare_refine(K)
        prm = params_of(api, *key)
        got = ctx.refine_clouds(prm, [(world.clouds[s], h) for s, _, _ in two], np.stack([p[2] for p in two]))
        assert_same_results(got, first)
    finally:
        h.close()


def lattice(n, seed):
    """n points 0.5 m apart with +-0.1 m of jitter: no two share a 0.2 m voxel, so the handle's m is n (test_gpu_gicp_clouds.py uses it too)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    g = np.stack(np.meshgrid(*([np.arange(side)] * 3), indexing="ij"), -1).reshape(-1, 3)[:n]
    return (g * 0.5 + rng.uniform(-0.1, 0.1, (n, 3))).astype(np.float32)


def edge_raws():
    """Sources at the edges of the 2-D launch over one lattice target: fewer than 4 points; one block; just into a second block of 256; a
    second block of the radix select (cdiv(ns, 2048)).  A fifth of every source lies 9 m to the side, beyond the target (its lattice spans
    7 m): the overlap stays below 1, so the trimmed rejector and its select are at work; the initial pose is a little off the one the sources
    were made with, so the loop has something to do.  Returns the four sources, the target and the initial pose."""
    tgt = lattice(3000, 1)
    made = displaced(np.eye(4), 0.3, (0.03, -0.02, 0.01))
    inv = np.linalg.inv(made)
    rng = np.random.default_rng(2)
    raws = []
    for n in (2, 100, 257, 2500):
        x = tgt[rng.permutation(len(tgt))[:n]].astype(np.float64)
        x[: n // 5, 0] += 9.0
        raws.append((x @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
    return raws, tgt, displaced(made, 0.2, (0.02, 0.01, -0.01))


@pytest.fixture(scope="module")
def edge_clouds(ctx, api):
    """edge_raws as prepared handles.  The voxel filter keeps its first input point once more unless a point falls into the corner voxel, so m
    is n or n + 1: the classes are asserted on the m the handles report."""
    cfg = api.pair_config(api.FEATURE_NONE, api.CORR_NN, dof=6, voxel=0.2, max_iter=10)
    raws, tgt, init = edge_raws()
    clouds = [ctx.cloud_create(cfg, x) for x in raws + [tgt]]
    ms = [int(c.info().m) for c in clouds]
    print("down-sampled sizes:", ms)
    assert ms[0] < 4 and 4 <= ms[1] <= 256 and 257 <= ms[2] <= 258 and ms[3] > 2048 and ms[4] > 2048
    for c in clouds:
        c.prepare_refine(K)
    yield clouds, ms, init, [c.download()["ds"] for c in clouds]
    for c in clouds:
        c.close()


@pytest.mark.parametrize("metric,trimmed", [(0, True), (1, False)])
def test_edges_of_the_two_dimensional_launch(ctx, api, edge_clouds, metric, trimmed):
    clouds, ms, init, ds = edge_clouds
    prm = params_of(api, metric, trimmed, max_iter=3)
    T = clouds[4]
    # the small pairs sit between and after large ones: the blocks beyond their cdiv(ns, 256), min(cdiv(ns, 4), 512) and cdiv(ns, 2048) must do nothing
    order = [3, 0, 1, 3, 2, 0]
    inits = np.stack([init] * len(order))
    got = ctx.refine_clouds(prm, [(clouds[i], T) for i in order], inits)
    ref = {i: ctx.icp(ctx.transform_cloud_f32(ds[i], init.astype(np.float32)), ds[4], prm, want_transformed=False) for i in set(order)}
    for i, g in zip(order, got):
        r = ref[i]
        for k in STAT_KEYS:
            assert g[k] == r[k], (ms[i], k, g[k], r[k])
        assert r["done"] == 1
        np.testing.assert_array_equal(g["T"], r["T"])
        np.testing.assert_array_equal(g["Rt_refined"], product_f64(g["T"], init))
    print("iterations:", [g["iterations"] for g in got], "reasons:", [g["reason"] for g in got], "correspondences:", [g["correspondences"] for g in got])
    assert all(g["iterations"] >= 1 for i, g in zip(order, got) if i != 0)  # the pairs above the minimum went through the loop
    if trimmed:
        assert all(0.0 < g["overlap"] < 1.0 for i, g in zip(order, got) if i != 0), [g["overlap"] for g in got]
    assert_same_results(ctx.refine_clouds(prm, [(clouds[i], T) for i in order], inits, 2), got)
