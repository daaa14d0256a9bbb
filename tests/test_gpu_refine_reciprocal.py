"""Batched fine registration with reciprocal correspondences (ghicp_refine_clouds_reciprocal): every pair of a batch must come out exactly
as the per-pair path gives it -- ghicp_cloud_download, ghicp_transform_cloud_f32 with the float-rounded initial pose, ghicp_icp with
use_reciprocal = 1 -- whatever the other pairs of its chunk do.  The reference of every check is that per-pair path (pinned to the CPU
oracle by tests/test_gpu_icp.py); the new entry point is never checked against itself, except where a test is ABOUT the independence of a
pair from its neighbours and its chunking.  The scheme (World, three cached clouds, pairs that finish after different iteration counts) is
that of tests/test_gpu_refine.py; the small lattice clouds below put the per-iteration grid build at its edges."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# iteration limit per (metric, trimmed): point-to-plane and the trimmed rejector need fewer iterations, and in every parameter set at least one
# pair must still be stopped by the limit next to pairs that converge before it (limits from the iteration counts the per-pair path reports)
MAX_ITER_OF = {(0, False): 8, (1, False): 5, (0, True): 6, (1, True): 3}
K = 12
STAT_KEYS = ("done", "iterations", "converged", "reason", "correspondences", "overlap", "mse", "fitness")


def displaced(gt, deg, t):
    a = np.deg2rad(deg)
    d = np.eye(4)
    d[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    d[:3, 3] = t
    return d @ gt


def params_of(api, metric, trimmed, reciprocal=True, k=K):
    return api.icp_params(MAX_ITER_OF[metric, bool(trimmed)], reciprocal, trimmed, metric, 0.3, 0.1, k)


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


def per_pair(ctx, ds_s, ds_t, init, prm):
    """The reference: one ghicp_icp call on the downloaded clouds, the source moved by the float-rounded pose first."""
    return ctx.icp(ctx.transform_cloud_f32(ds_s, init.astype(np.float32)), ds_t, prm, want_transformed=False)


def assert_pair_equals(g, r, init, what=""):
    for k in STAT_KEYS:  # (a pair that ends without correspondences reports mse = NaN in both paths: compared as NaN == NaN)
        assert g[k] == r[k] or (g[k] != g[k] and r[k] != r[k]), "%s: %s = %r, the per-pair path gives %r" % (what, k, g[k], r[k])
    if r["done"]:
        np.testing.assert_array_equal(g["T"], r["T"])
    else:  # ghicp_icp leaves T untouched when it refuses; the batch reports the identity
        np.testing.assert_array_equal(g["T"], np.eye(4, dtype=np.float32))
    np.testing.assert_array_equal(g["Rt_refined"], product_f64(g["T"], init))


def assert_same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for k in STAT_KEYS:
            assert x[k] == y[k] or (x[k] != x[k] and y[k] != y[k]), k
        np.testing.assert_array_equal(x["T"], y["T"])
        np.testing.assert_array_equal(x["Rt_refined"], y["Rt_refined"])


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
        # as in tests/test_gpu_refine.py: two pairs share the target B; B is a source and a target; (C, B) comes twice with different poses;
        # the last pair starts far off and is stopped by max_iter
        self.pairs = [("A", "B", displaced(self.gt["A", "B"], 0.1, (0.02, -0.01, 0.0))),
                      ("C", "B", displaced(self.gt["C", "B"], 0.5, (0.08, -0.05, 0.02))),
                      ("B", "A", displaced(self.gt["B", "A"], -0.1, (0.02, -0.01, 0.0))),
                      ("C", "B", self.gt["C", "B"].copy()),
                      ("A", "B", displaced(self.gt["A", "B"], 6.0, (1.2, -0.8, 0.1)))]
        self.refused = ("A", "B", displaced(self.gt["A", "B"], 0.0, (900.0, 0.0, 0.0)))
        self._ref = {}

    def prepare(self, k):
        if self.prepared != k:
            for c in self.clouds.values():
                c.prepare_refine(k)
            self.prepared = k

    def reference(self, prm_key, pair):
        s, t, init = pair
        key = (prm_key, s, t, init.tobytes())
        if key not in self._ref:
            self._ref[key] = per_pair(self.ctx, self.ds[s], self.ds[t], init, params_of(self.api, *prm_key))
        return self._ref[key]

    def handles(self, pairs):
        return [(self.clouds[s], self.clouds[t]) for s, t, _ in pairs]

    def refine(self, prm_key, pairs, max_concurrent=0):
        self.prepare(K)
        return self.ctx.refine_clouds_reciprocal(params_of(self.api, *prm_key), self.handles(pairs), np.stack([p[2] for p in pairs]), max_concurrent)


@pytest.fixture(scope="module")
def world(ctx, api, synth):
    w = World(ctx, api, synth)
    yield w
    for c in w.clouds.values():
        c.close()


def assert_same_as_reference(world, prm_key, pairs, got):
    assert len(got) == len(pairs)
    for p, (pair, g) in enumerate(zip(pairs, got)):
        assert_pair_equals(g, world.reference(prm_key, pair), pair[2], "pair %d" % p)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("trimmed", [False, True])
def test_batch_is_bit_identical_to_the_per_pair_path(world, api, metric, trimmed):
    key = (metric, trimmed)
    pairs = list(world.pairs) + ([world.refused] if trimmed else [])
    got = world.refine(key, pairs)
    its = [g["iterations"] for g in got if g["done"]]
    print("iterations per pair:", its, "reasons:", [g["reason"] for g in got], "correspondences:", [g["correspondences"] for g in got])
    assert_same_as_reference(world, key, pairs, got)
    # the fixture bites: pairs leave the loop after different numbers of iterations, one of them stopped by max_iter next to converged ones,
    # and the reciprocal test removes correspondences (ghicp_refine_clouds, without the flag, keeps more)
    assert len(set(its)) > 1, "every pair ran %r iterations: the fixture no longer tests the freeze" % its
    assert any(g["reason"] == 1 and g["iterations"] == MAX_ITER_OF[key] for g in got) and min(its) < MAX_ITER_OF[key]
    plain = world.ctx.refine_clouds(params_of(api, metric, trimmed, reciprocal=False), world.handles(pairs), np.stack([p[2] for p in pairs]))
    assert any(g["done"] and g["correspondences"] != q["correspondences"] for g, q in zip(got, plain))
    if trimmed:
        assert got[-1]["done"] == 0 and all(g["done"] == 1 for g in got[:-1])


def test_results_do_not_depend_on_the_chunking(world):
    key = (0, True)
    whole = world.refine(key, world.pairs, 0)
    assert len(set(g["iterations"] for g in whole)) > 1
    assert_same_as_reference(world, key, world.pairs, whole)
    assert_same_results(world.refine(key, world.pairs, 1), whole)
    assert_same_results(world.refine(key, world.pairs, 2), whole)  # chunks of 2, 2, 1


def test_frozen_neighbours_are_left_alone(world, ctx, api):
    """A pair that converges early, a pair the overlap gate refuses, a pair whose source is empty (its overlap is empty: no launch at all) and
    a pair that runs to max_iter in ONE chunk: each comes out as when it runs alone.  The points of the pairs that have left the loop still
    ride along in every iteration's sort."""
    key = (0, True)
    world.prepare(K)
    empty = ctx.cloud_create(world.cfg, world.raw["A"][:0])
    try:
        prm = params_of(api, *key)
        pairs = [world.pairs[3], world.refused, world.pairs[0]]
        handles = world.handles(pairs)
        inits = [p[2] for p in pairs]
        handles.insert(2, (empty, world.clouds["B"]))
        inits.insert(2, np.eye(4))
        got = ctx.refine_clouds_reciprocal(prm, handles, np.stack(inits), 4)
        print("iterations:", [g["iterations"] for g in got], "done:", [g["done"] for g in got], "reasons:", [g["reason"] for g in got])
        assert got[0]["iterations"] < got[3]["iterations"] == MAX_ITER_OF[key] and got[3]["reason"] == 1 and got[1]["done"] == 0 and got[2]["iterations"] == 0
        for p in range(4):
            (alone,) = ctx.refine_clouds_reciprocal(prm, [handles[p]], inits[p][None])
            assert_same_results([got[p]], [alone])
        for p, q in ((0, 0), (1, 1), (3, 2)):  # and as the per-pair path gives it
            assert_pair_equals(got[p], world.reference(key, pairs[q]), pairs[q][2], "pair %d" % p)
    finally:
        empty.close()


@pytest.mark.parametrize("metric,trimmed", [(0, True), (1, False)])
def test_without_the_flag_the_new_call_is_ghicp_refine_clouds(world, api, metric, trimmed):
    world.prepare(K)
    pairs = [world.pairs[1], world.pairs[3]] + ([world.refused] if trimmed else [])
    prm = params_of(api, metric, trimmed, reciprocal=False)
    inits = np.stack([p[2] for p in pairs])
    assert_same_results(world.ctx.refine_clouds_reciprocal(prm, world.handles(pairs), inits), world.ctx.refine_clouds(prm, world.handles(pairs), inits))


# ------------------------------------------------------------------------------------------------ edge shapes: small lattice clouds
def lattice(nx, ny, nz, step=1.0, origin=(0.0, 0.0, 0.0)):
    """Points on a regular lattice, x slowest; the first point is the box's minimum corner (the voxel filter keeps it as its first group)."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return (g * step + np.asarray(origin)).astype(np.float32)


class Lattices:
    """Handles over clouds the voxel filter keeps whole (voxel well below the lattice step): the down-sampled sizes are the raw sizes."""

    def __init__(self, ctx, api):
        self.ctx, self.api = ctx, api
        self.cfg = api.pair_config(api.FEATURE_NONE, api.CORR_NN, dof=6, voxel=0.1, max_iter=10)
        base = lattice(8, 8, 4)  # 256 points, spacing 1.0
        far = np.array([[3.0, 2.0, 400.0]], np.float32)
        raw = dict(
            L255=base[:255], L256=base, L257=np.concatenate([base, [[8.0, 0.0, 0.0]]]).astype(np.float32),
            # ties: a lattice of step 0.5 (coordinates are multiples of 0.25) and the same lattice half a step along x
            tieS=lattice(6, 5, 4, 0.5), tieT=lattice(6, 5, 4, 0.5, (0.25, 0.0, 0.0)),
            line=np.stack([np.arange(260) * 0.25, np.zeros(260), np.zeros(260)], 1).astype(np.float32) + np.float32(1.0),
            outlier=np.concatenate([base, far]).astype(np.float32),
            few=np.array([[1.0, 1.0, 0.0], [5.0, 2.0, 1.0], [2.0, 6.0, 3.0], [6.0, 6.0, 1.0]], np.float32))
        self.clouds = {k: ctx.cloud_create(self.cfg, v) for k, v in raw.items()}
        self.ds = {}
        for k, c in self.clouds.items():
            self.ds[k] = c.download()["ds"]
            assert int(c.info().m) == len(raw[k]) == self.ds[k].shape[0], "the voxel filter dropped points of %s" % k
            c.prepare_refine(0)

    def check(self, pairs, prm, max_concurrent=0):
        """pairs: (source name, target name, init).  The batch against the per-pair path; returns the batch's results."""
        got = self.ctx.refine_clouds_reciprocal(prm, [(self.clouds[s], self.clouds[t]) for s, t, _ in pairs], np.stack([p[2] for p in pairs]), max_concurrent)
        for p, ((s, t, init), g) in enumerate(zip(pairs, got)):
            assert_pair_equals(g, per_pair(self.ctx, self.ds[s], self.ds[t], init, prm), init, "pair %d (%s -> %s)" % (p, s, t))
        print([(g["iterations"], g["reason"], g["correspondences"]) for g in got])
        return got

    def close(self):
        for c in self.clouds.values():
            c.close()


@pytest.fixture(scope="module")
def lat(ctx, api):
    w = Lattices(ctx, api)
    yield w
    w.close()


SMALL = displaced(np.eye(4), 1.0, (0.15, -0.1, 0.05))


@pytest.mark.parametrize("trimmed", [False, True])
def test_sources_that_straddle_a_block(lat, api, trimmed):
    """255, 256 and 257 down-sampled points: one block exactly full, one point short, one point into a second block -- sources of different
    sizes side by side in one chunk, and one in a chunk of its own."""
    prm = api.icp_params(4, True, trimmed, 0, 0.6, 0.1, 0)
    pairs = [("L255", "L257", SMALL), ("L256", "L257", displaced(np.eye(4), -1.0, (0.1, 0.2, 0.0))), ("L257", "L256", SMALL), ("L256", "L255", np.eye(4))]
    got = lat.check(pairs, prm)
    assert_same_results(lat.check(pairs, prm, 3), got)


@pytest.mark.parametrize("max_iter", [1, 3])
def test_exact_ties_go_to_the_lower_index(lat, api, max_iter):
    """Every target point lies exactly between two source points (0.25 on either side along x, all coordinates multiples of 0.25: the float
    distances are equal): forward search and back-search must both take the lower index, as the single-pair kernels do."""
    prm = api.icp_params(max_iter, True, False, 0, 0.6, 0.1, 0)
    got = lat.check([("tieS", "tieT", np.eye(4)), ("tieT", "tieS", np.eye(4))], prm)
    if max_iter == 1:  # the ties are in the first iteration only (the first step moves the source off the half-way position): a source point
        # keeps its target only where it is the lower-indexed of the two candidates
        assert all(0 < g["correspondences"] < lat.ds["tieS"].shape[0] for g in got)


def test_a_self_pair_keeps_every_correspondence(lat, api):
    prm = api.icp_params(3, True, False, 0, 0.6, 0.1, 0)
    (g,) = lat.check([("L257", "L257", np.eye(4))], prm)
    assert g["correspondences"] == 257


def test_degenerate_moved_sources(lat, api):
    """All points on a line along one axis (two box extents are zero), and a source with one point hundreds of metres from the rest: the box
    is huge, the pair's cell budget forces the cell up, most points share a few cells and the coarse hand-off runs."""
    prm = api.icp_params(4, True, False, 0, 0.6, 0.1, 0)
    lat.check([("line", "L256", SMALL), ("outlier", "L257", SMALL), ("L256", "line", np.eye(4)), ("L255", "outlier", SMALL)], prm)


@pytest.mark.parametrize("trimmed", [False, True])
def test_a_target_of_a_few_points(lat, api, trimmed):
    """Almost every source point shares its nearest target point with many others: the reciprocal test leaves at most one correspondence per
    target point.  Whatever ghicp_icp reports -- GHICP_ICP_NO_CORRESPONDENCES included -- the batch reports."""
    prm = api.icp_params(4, True, trimmed, 0, 1.5, 0.01, 0)
    got = lat.check([("L257", "few", np.eye(4)), ("L255", "few", SMALL), ("few", "L256", SMALL)], prm)
    assert all(g["correspondences"] <= 4 for g in got)


def test_one_handle_in_several_roles(lat, api):
    """The same handle as the source of two pairs with different poses, and as source and target within one chunk."""
    prm = api.icp_params(4, True, True, 0, 0.6, 0.1, 0)
    lat.check([("L257", "L256", SMALL), ("L257", "L256", displaced(np.eye(4), -2.0, (0.0, 0.3, 0.1))), ("L256", "L257", SMALL)], prm)


# ------------------------------------------------------------------------------------------------ errors
def test_errors_leave_nothing_half_written(world, ctx, api):
    key = (1, True)
    pairs = world.pairs
    handles = world.handles(pairs)
    inits = np.stack([p[2] for p in pairs])
    fresh = ctx.cloud_create(world.cfg, world.raw["B"])
    try:
        with pytest.raises(api.GhicpError):  # a target that was never prepared (last pair: the earlier ones must not have been started)
            ctx.refine_clouds_reciprocal(params_of(api, 0, True), handles[:2] + [(world.clouds["A"], fresh)], inits[:3])
        world.prepare(K)
        with pytest.raises(api.GhicpError):  # normals for another k
            ctx.refine_clouds_reciprocal(params_of(api, 1, True, k=K + 1), handles, inits)
        fresh.prepare_refine(0)
        with pytest.raises(api.GhicpError):  # point-to-plane on a target prepared without normals
            ctx.refine_clouds_reciprocal(params_of(api, 1, True), [(world.clouds["A"], fresh)], inits[:1])
        with pytest.raises(api.GhicpError):  # the old call still refuses the flag
            ctx.refine_clouds(params_of(api, 0, True, reciprocal=True), handles, inits)
        d = fresh.download()
        stored = ctx.cloud_from_features(world.cfg, d["kp_xyz"], None, fresh.info().bbx_magnitude)
        with pytest.raises(api.GhicpError):  # no points in a handle rebuilt from stored features
            ctx.refine_clouds_reciprocal(params_of(api, 0, True), [(stored, fresh)], inits[:1])
        stored.close()
        fresh.prepare_refine(K)
        fresh.recompute(world.raw["B"])
        with pytest.raises(api.GhicpError):  # recompute invalidates the prepared state
            ctx.refine_clouds_reciprocal(params_of(api, 1, True), [(world.clouds["A"], fresh)], inits[:1])
    finally:
        fresh.close()
    again = [pairs[1], pairs[3]]
    assert_same_as_reference(world, key, again, world.refine(key, again))  # and the context is as good as before
