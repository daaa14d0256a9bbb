"""Batched prepare (ghicp_clouds_prepare): the prepared state of MANY handles in one launch sequence per chunk must be, byte for byte, what
ghicp_cloud_prepare_refine / ghicp_cloud_prepare_gicp / ghicp_cloud_prepare_overlap leave cloud by cloud -- every descriptor
(ghicp_cloud_get_prepared) and every buffer (the eight parts of ghicp_cloud_download_prepared).  Every case makes two sets of handles from the
same raw clouds, prepares one per cloud and one by the batch, and compares them exactly.

The handles are made without the voxel filter (voxel = 0), so a handle holds exactly the points it was given; `make` asserts it."""
import numpy as np
import pytest

from test_gpu_refine import params_of

pytestmark = pytest.mark.gpu

PARTS = range(8)  # GHICP_PREP_FINE_PTS .. GHICP_PREP_COVARIANCES


def blob(rng, n, side=3.0, at=(0.0, 0.0, 0.0)):
    return (rng.uniform(0.0, side, (n, 3)) + np.asarray(at)).astype(np.float32)


def plane_in_box(rng, n, box=6.0):
    """a dense planar patch inside a large, almost empty box: the volume guess of the fine cell is far too coarse, so it is halved several
    times (a uniform blob is not halved at all)"""
    p = np.zeros((n, 3))
    p[:, :2] = rng.uniform(0.0, 1.5, (n, 2))
    p[:, 2] = rng.normal(0.0, 0.002, n)
    p[:8] = box * np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)])
    return p.astype(np.float32)


def surface(rng, n, noise=0.0):
    xy = rng.uniform(0.0, 6.0, (n, 2))
    z = 0.4 * np.sin(xy[:, 0]) + 0.3 * np.cos(1.3 * xy[:, 1])
    return (np.column_stack([xy, z]) + rng.normal(0, noise, (n, 3))).astype(np.float32)


def make(ctx, api, raws):
    cfg = api.pair_config(api.FEATURE_NONE, api.CORR_NN, dof=6, voxel=0.0, max_iter=10)
    out = []
    for r in raws:
        c = ctx.cloud_create(cfg, np.ascontiguousarray(r, np.float32).reshape(-1, 3))
        assert int(c.info().m) == len(r)
        out.append(c)
    return out


def per_cloud(clouds, refine=False, normals_k=0, gicp_k=0, gicp_eps=1e-3, overlap_thre=None):
    """the three per-cloud calls in the order ghicp_clouds_prepare documents"""
    for c in clouds:
        if refine or normals_k > 0:
            c.prepare_refine(normals_k)
        if gicp_k > 0:
            c.prepare_gicp(gicp_k, gicp_eps)
        if overlap_thre is not None:
            c.prepare_overlap(overlap_thre)


def snapshot(api, c):
    """the info struct and the eight parts as bytes (None: not held)"""
    parts = []
    for which in PARTS:
        try:
            parts.append(c.download_prepared(which).cpu().numpy().tobytes())
        except api.GhicpError:
            parts.append(None)
    return bytes(c.prepared()), parts


def assert_same_state(api, A, B, what=""):
    assert len(A) == len(B)
    for i, (a, b) in enumerate(zip(A, B)):
        ia, pa = snapshot(api, a)
        ib, pb = snapshot(api, b)
        assert ia == ib, "%s cloud %d: the info structs differ" % (what, i)
        for which in PARTS:
            assert (pa[which] is None) == (pb[which] is None), "%s cloud %d part %d: held by one set only" % (what, i, which)
            assert pa[which] == pb[which], "%s cloud %d part %d: bytes differ" % (what, i, which)


def close(*sets):
    for s in sets:
        for c in s:
            c.close()


FULL = dict(refine=True, normals_k=15, gicp_k=15, gicp_eps=1e-3, overlap_thre=0.5)


# ------------------------------------------------------------------------------------------------ 1. every byte equal, one chunk
@pytest.fixture(scope="module")
def edge_raws():
    rng = np.random.default_rng(17)
    raws = [blob(rng, n) for n in (0, 1, 2, 5, 255, 256, 257)]  # empty; fewer than 3 neighbours (0.577 normals); < k; block edges
    raws.append(blob(rng, 5000, side=6.0, at=(10.0, -3.0, 1.0)))
    raws.append(plane_in_box(rng, 3000))  # several halvings ...
    raws.append(blob(rng, 1200, side=2.0))  # ... next to none: they stop in different rounds
    raws.append(raws[7].copy())  # the same raw cloud in two handles
    return raws


@pytest.mark.parametrize("spec", [FULL, dict(FULL, normals_k=12, gicp_k=20)], ids=["one_search", "two_searches"])
def test_every_byte_equals_the_per_cloud_calls(ctx, api, edge_raws, spec):
    A, B = make(ctx, api, edge_raws), make(ctx, api, edge_raws)
    per_cloud(A, **spec)
    ctx.prepare_clouds(B, **spec)
    assert_same_state(api, A, B)
    for c, r in zip(B, edge_raws):
        p = c.prepared()
        assert (p.refine_ready, p.normals_k, p.gicp_ready, p.gicp_k, p.overlap_ready) == (1, spec["normals_k"], 1, spec["gicp_k"], 1)
        assert p.fine.n == p.coarse.n == p.overlap.n == (len(r) if len(r) else 0)
    # the planar patch was halved, the blobs were not: the rounds of the chunk really differ per cloud
    vol_cell = lambda r: max(float(np.cbrt(np.prod(r.max(0) - r.min(0) + 1e-3) / len(r) * 8.0)), 0.02)
    assert 1.0 / B[8].prepared().fine.inv < 0.3 * vol_cell(edge_raws[8])
    assert 1.0 / B[9].prepared().fine.inv > 0.9 * vol_cell(edge_raws[9])
    # rows of a grid: a permutation of the cloud's own indices, every cell table ends at m
    for c, r in zip(B, edge_raws):
        if len(r) == 0:
            continue
        for pts_part, start_part in ((0, 1), (2, 3), (4, 5)):
            w = c.download_prepared(pts_part).cpu().numpy()[:, 3].copy().view(np.uint32)
            assert np.array_equal(np.sort(w), np.arange(len(r), dtype=np.uint32))
            st = c.download_prepared(start_part).cpu().numpy()
            assert st[0] == 0 and st[-1] == len(r)
    assert ctx.prepare_host_waits() <= 2 + 6  # boxes, at most six rounds of the fine cell, the end: independent of the number of clouds
    close(A, B)


def test_a_batch_of_one(ctx, api, edge_raws):
    A, B = make(ctx, api, edge_raws[6:7]), make(ctx, api, edge_raws[6:7])
    per_cloud(A, **FULL)
    ctx.prepare_clouds(B, **FULL)
    assert_same_state(api, A, B)
    close(A, B)


# ------------------------------------------------------------------------------------------------ 2. chunk crossing, list order
def test_sixty_five_clouds_cross_a_chunk_and_the_order_does_not_matter(ctx, api):
    rng = np.random.default_rng(23)
    raws = [blob(rng, 40 + (7 * i) % 23, side=1.0 + 0.1 * (i % 5), at=(i, -i, 0.5 * i)) for i in range(65)]
    A, B, R = make(ctx, api, raws), make(ctx, api, raws), make(ctx, api, raws)
    spec = dict(FULL, normals_k=10, gicp_k=10)
    per_cloud(A, **spec)
    ctx.prepare_clouds(B, **spec)
    ctx.prepare_clouds(R[::-1], **spec)
    assert_same_state(api, A, B, "list order")
    assert_same_state(api, A, R, "reversed list")
    close(A, B, R)


# ------------------------------------------------------------------------------------------------ 3. keep / replace rules
def test_state_rules_follow_the_per_cloud_calls(ctx, api):
    rng = np.random.default_rng(31)
    raws = [surface(rng, 300), blob(rng, 0), blob(rng, 700, side=2.0)]
    A, B = make(ctx, api, raws), make(ctx, api, raws)
    steps = [dict(refine=True), dict(normals_k=15), dict(normals_k=10), dict(gicp_k=20, gicp_eps=1e-3), dict(gicp_k=10, gicp_eps=1e-2),
             dict(overlap_thre=0.5), dict(overlap_thre=0.3), dict(overlap_thre=0.3), dict(FULL), dict(FULL), dict(), dict(refine=True)]
    for n, spec in enumerate(steps):
        before = [snapshot(api, c) for c in B] if not spec else None
        per_cloud(A, **spec)
        ctx.prepare_clouds(B, **spec)
        assert_same_state(api, A, B, "step %d %r" % (n, spec))
        if not spec:  # a spec asking for nothing changes nothing
            assert before == [snapshot(api, c) for c in B]
    p = B[0].prepared()  # refine with k = 0 after normals: their k is 0, the part is no longer held
    assert p.refine_ready == 1 and p.normals_k == 0 and p.gicp_ready == 1 and p.overlap_ready == 1
    with pytest.raises(api.GhicpError, match="ghicp error 1"):
        B[0].download_prepared(api.PREP_NORMALS)
    # recompute invalidates everything; then the covariances first (the grids come from that call, no normals), then the rest
    raws2 = [blob(rng, 350, side=2.5), surface(rng, 500), blob(rng, 3)]
    for c, r in zip(A, raws2):
        c.recompute(r)
    ctx.clouds_recompute(B, raws2)
    for c in B:
        p = c.prepared()
        assert (p.refine_ready, p.normals_k, p.gicp_ready, p.overlap_ready) == (0, 0, 0, 0)
    for n, spec in enumerate([dict(gicp_k=20), dict(FULL)]):
        per_cloud(A, **spec)
        ctx.prepare_clouds(B, **spec)
        assert_same_state(api, A, B, "after recompute, step %d" % n)
    # handles in different states in one list: one keeps what it has, one gets the rest
    A[0].recompute(raws2[0])
    B[0].recompute(raws2[0])
    A[0].prepare_overlap(0.5)
    B[0].prepare_overlap(0.5)
    per_cloud(A, **FULL)
    ctx.prepare_clouds(B, **FULL)
    assert_same_state(api, A, B, "mixed states")
    close(A, B)


# ------------------------------------------------------------------------------------------------ 4. consumers
def test_consumers_see_no_difference(ctx, api):
    rng = np.random.default_rng(41)
    base = surface(rng, 2600, noise=0.002)
    raws = []
    for i in range(4):
        a = np.deg2rad(1.5 * i)
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        keep = rng.permutation(len(base))[:2000]
        raws.append(((base[keep].astype(np.float64) @ R.T) + [0.03 * i, -0.02 * i, 0.01 * i] + rng.normal(0, 0.002, (2000, 3))).astype(np.float32))
    A, B = make(ctx, api, raws), make(ctx, api, raws)
    spec = dict(refine=True, normals_k=12, gicp_k=10, gicp_eps=1e-3, overlap_thre=0.3)
    per_cloud(A, **spec)
    ctx.prepare_clouds(B, **spec)
    idx = [(i, j) for i in range(4) for j in range(4) if i != j]
    assert len(idx) == 12
    pairs = lambda H: [(H[i], H[j]) for i, j in idx]

    def same(ra, rb):
        assert len(ra) == len(rb) == 12
        for x, y in zip(ra, rb):
            assert x.keys() == y.keys()
            for k in x:
                assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k

    for metric, trimmed in ((api.ICP_POINT_TO_POINT, True), (api.ICP_POINT_TO_PLANE, False)):
        prm = params_of(api, metric, trimmed, max_iter=4, k=12)
        same(ctx.refine_clouds(prm, pairs(A)), ctx.refine_clouds(prm, pairs(B)))
    prm = params_of(api, api.ICP_POINT_TO_POINT, False, max_iter=3, reciprocal=True, k=12)
    same(ctx.refine_clouds_reciprocal(prm, pairs(A)), ctx.refine_clouds_reciprocal(prm, pairs(B)))
    g = api.gicp_params(3, False, False, 0.3, 0.1, 10, 1e6, 3)
    g.gicp_epsilon = 1e-3
    same(ctx.gicp_clouds(g, pairs(A)), ctx.gicp_clouds(g, pairs(B)))
    oa = ctx.overlap_clouds([A[i] for i, _ in idx], [A[j] for _, j in idx], 0.3)
    ob = ctx.overlap_clouds([B[i] for i, _ in idx], [B[j] for _, j in idx], 0.3)
    for k in ("hits", "n", "ratio"):
        assert np.array_equal(oa[k], ob[k])
    assert oa["hits"].min() > 0
    assert np.array_equal(ctx.overlap_matrix(A, 0.3), ctx.overlap_matrix(B, 0.3))
    close(A, B)


# ------------------------------------------------------------------------------------------------ 5. errors
def test_errors_leave_every_handle_as_it_was(ctx, api):
    rng = np.random.default_rng(53)
    H = make(ctx, api, [blob(rng, 120), blob(rng, 90)])
    ctx.prepare_clouds(H[:1], refine=True, normals_k=8)
    cfg = api.pair_config(api.FEATURE_NONE, api.CORR_NN, dof=6, voxel=0.0, max_iter=10)
    stored = ctx.cloud_from_features(cfg, rng.uniform(0, 1, (3, 3)), None, 1.0)
    state = lambda: [snapshot(api, c) for c in H]
    before = state()
    bad = [
        (H + [stored], dict(FULL)),                       # a handle rebuilt from stored features
        (H + [H[0]], dict(FULL)),                         # a duplicate
        (H + [None], dict(FULL)),                         # a NULL handle
        (H, dict(FULL, normals_k=21)),
        (H, dict(FULL, gicp_k=21)),
        (H, dict(FULL, overlap_thre=0.0)),
        (H, dict(FULL, gicp_eps=0.0)),
    ]
    for lst, spec in bad:
        with pytest.raises(api.GhicpError, match="ghicp error 1"):
            ctx.prepare_clouds(lst, **spec)
        assert state() == before, spec
    ctx.prepare_clouds([], **FULL)  # n_clouds = 0 is fine
    assert state() == before
    for which in (api.PREP_FINE_PTS, api.PREP_NORMALS):
        assert H[0].download_prepared(which).shape[0] == 120
    for which in (api.PREP_OVERLAP_PTS, api.PREP_OVERLAP_START, api.PREP_COVARIANCES):  # parts not held
        with pytest.raises(api.GhicpError, match="ghicp error 1"):
            H[0].download_prepared(which)
    with pytest.raises(api.GhicpError, match="ghicp error 1"):
        H[1].download_prepared(api.PREP_FINE_START)
    stored.close()
    close(H)
