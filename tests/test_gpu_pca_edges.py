"""k_pca_cells / k_fb_pca_cells (csrc/pca_dev.h, grid.h) against a grid-free brute force (tests/frontend_restatement.py) on clouds crafted to
reach every regime of gh_pca_cell_body and gh_grid_desc: the np x g lane split, the second pass over a cell's query points, the four hit
masks and the tail past 128 candidates per lane, the resident tile and the streamed fallback, k < 3, the strict radius test, the faces
of the cell table, the widened and the coarsened cell, and the deal of more than 512 runs.  Every case asserts through grid_regimes that
the regime is present in its cloud.

Per case: neighbour counts equal the brute force exactly; per point |lambda_gpu - lambda_ref| <= 2^-22 lambda1_ref (derived: N2 rounds each
scatter entry by at most 2^-23 max|S_ij| <= 2^-23 lambda1, a symmetric perturbation moves an eigenvalue by at most its Frobenius norm
<= 1.5 * 2^-23 lambda1, the final float rounding adds 2^-24 lambda1); the curvature is the formula of pca.h:240-247 on the GPU's own
eigenvalues, exactly; and where the oracle's counts equal the brute force, the oracle is compared under test_pca_curvature's allowance."""
import os

import numpy as np
import pytest

import frontend_restatement as FR

pytestmark = pytest.mark.gpu

F = np.float32
SIM = os.environ.get("GHICP_SIM") == "1"
CELL = float(F(0.5) * F(1.0001))  # the PCA cell at radius 0.5 (below 256 cells per axis)
PITCH = np.array([0.01, 0.006, 0.003])
DIRS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (-1, -1, 0), (1, 0, 1), (-1, 0, -1), (0, 1, 1), (0, -1, -1)]


def _offsets(k, rng):
    """k distinct positions of an anisotropic 9 x 9 x 9 lattice (pitch 10 / 6 / 3 mm: much smaller than a cell, wider than a 1 mm voxel), jittered"""
    assert k <= 729
    idx = rng.choice(729, k, replace=False)
    o = np.stack([idx % 9 - 4, idx // 9 % 9 - 4, idx // 81 - 4], axis=1) * PITCH
    return o + rng.uniform(-2e-4, 2e-4, (k, 3))


def _cluster(cell, k, rng):
    return (np.asarray(cell, np.float64) + 0.5) * CELL + _offsets(k, rng)


def _structures(specs, rng, pitch=5, per_row=6, extra=()):
    """One cluster of np points in the centre of a cell per spec (np, satellites), the satellites in up to 12 adjacent cells (<= 100 each);
    the clusters `pitch` cells apart; a point at the origin pins the table's corner (and is a point with one neighbour: itself)."""
    parts = [np.zeros((1, 3))]
    for s, (npq, sat) in enumerate(specs):
        c = np.array([2 + pitch * (s % per_row), 2 + pitch * (s // per_row % per_row), 2 + pitch * (s // (per_row * per_row))])
        parts.append(_cluster(c, npq, rng))
        ncell = max(1, -(-sat // 100))
        assert ncell <= len(DIRS)
        for t in range(ncell if sat else 0):
            k = sat // ncell + (1 if t < sat % ncell else 0)
            parts.append(_cluster(c + DIRS[t], k, rng))
    parts += list(extra)
    return np.ascontiguousarray(np.concatenate(parts).astype(F))


def _sat_for(npq):
    g = FR.lane_split(min(npq, 64))
    sat = 7
    while g > 1 and (npq + sat) % g == 0:
        sat += 1
    return sat


# ---------------------------------------------------------------- the clouds (shared with the batched test)
LANE_NP = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64]
PASS_NP = [65, 128, 129]
PER_LANE = [(20, 62), (20, 64), (20, 65), (40, 64), (40, 96), (40, 128), (40, 129), (40, 150), (20, 300), (40, 448)]  # (np, block total)
BOUNDARY_TOTAL = [447, 448, 449, 512, 513]
MIN_N = 16  # the batched test's min_neighbors: isolated clusters of 16 (rejected) and 17 (accepted) points


def _threshold_clusters(rng, row):
    """isolated clusters whose neighbour count is exactly their size: four of MIN_N points, sixteen of MIN_N + 1, on a row of their own"""
    return [_cluster((2 + 5 * t, 2 + 5 * row, 40), MIN_N + (t >= 4), rng) for t in range(20)]


def cloud_lane_split():
    rng = np.random.default_rng(101)
    return _structures([(v, _sat_for(v)) for v in LANE_NP], rng, extra=_threshold_clusters(rng, 0))


def cloud_second_pass():
    rng = np.random.default_rng(102)
    return _structures([(v, 10) for v in PASS_NP], rng, extra=_threshold_clusters(rng, 0))


def cloud_masks():
    rng = np.random.default_rng(103)
    return _structures([(a, t - a) for a, t in PER_LANE], rng, extra=_threshold_clusters(rng, 1))


def cloud_boundary():
    rng = np.random.default_rng(104)
    col = np.arange(1100)
    z = 2 * CELL + 0.01 + col * ((3 * CELL - 0.02) / 1100)
    column = np.stack([12.5 * CELL + (col % 9 - 4) * 0.01, 32.5 * CELL + (col // 9 % 9 - 4) * 0.01, z], axis=1)  # cells (12, 32, 2..4)
    return _structures([(30, t - 30) for t in BOUNDARY_TOTAL], rng, extra=[column] + _threshold_clusters(rng, 2))


def cloud_few():
    rng = np.random.default_rng(105)
    pair = np.array([[4.0, 4.0, 4.0], [4.1, 4.0, 4.0]])
    lone = np.array([[8.0, 4.0, 4.0]])
    return _structures([(5, 0), (3, 0)], rng, extra=[pair, lone] + _threshold_clusters(rng, 1))


def cloud_strict():
    """an 8 x 8 x 8 lattice of pitch 0.25 (axis pairs at exactly d2 == r2 in f32: excluded), and beside it p = (0, 0, -3) with q at
    exactly 0.5 (excluded) and r at nextafter(0.5, 0) (included)"""
    i = np.arange(512)
    lat = np.stack([i % 8, i // 8 % 8, i // 64], axis=1) * 0.25
    trio = np.array([[0.0, 0.0, -3.0], [-0.5, 0.0, -3.0], [float(np.nextafter(F(0.5), F(0))), 0.0, -3.0]])
    return np.ascontiguousarray(np.concatenate([lat, trio]).astype(F))


def _check(ctx, oracle, xyz, radius=0.5, want_oracle=True):
    """the assertions of every case; returns (counts, GPU eigenvalues, GPU curvature, oracle counts equal the brute force)"""
    lr, cr, nr = FR.pca_reference(xyz, radius)
    lg, cg, ng = ctx.pca_curvature(xyz, radius)
    lg, cg, ng = lg.cpu().numpy(), cg.cpu().numpy(), ng.cpu().numpy()
    np.testing.assert_array_equal(ng, nr)
    err = np.abs(lg.astype(np.float64) - lr)
    worst = float((err / np.maximum(lr[:, :1], 1e-300)).max()) if (nr >= 3).any() else 0.0
    print("n = %d, worst eigenvalue error / lambda1 = %.3g (bound %.3g)" % (xyz.shape[0], worst, 2.0 ** -22))
    assert (err <= 2.0 ** -22 * lr[:, :1]).all(), worst
    assert not lg[nr < 3].any() and not cg[nr < 3].any()
    np.testing.assert_array_equal(cg, FR.curvature_of(lg))
    agree = None
    if want_oracle:
        lo, co, no = oracle.pca(xyz, radius)
        agree = bool(np.array_equal(no, nr))
        if agree:
            bad = np.flatnonzero((lg != lo).any(axis=1))
            assert bad.size <= max(3, lo.shape[0] // 20000), bad.size
            np.testing.assert_allclose(lg, lo, rtol=3e-7, atol=0)
    return nr, lg, cg, agree


def test_lane_split(ctx, oracle):
    xyz = cloud_lane_split()
    g = FR.grid_regimes(xyz, 0.5)
    for v in LANE_NP:
        sel = (g.np == v) & ((g.g_first == 1) | (g.total % g.g_first != 0))
        assert sel.any(), v  # a cell of v query points whose block does not fill its last step of g lanes (the `mine` mask)
    assert sorted(set(g.g_first.tolist())) == [1, 2, 4, 8, 16, 32, 64]
    assert _check(ctx, oracle, xyz)[3]


def test_second_query_pass(ctx, oracle):
    xyz = cloud_second_pass()
    g = FR.grid_regimes(xyz, 0.5)
    for v, gl in ((65, 64), (128, 1), (129, 64)):
        assert ((g.np == v) & (g.g_first == 1) & (g.g_last == gl)).any(), v
    assert _check(ctx, oracle, xyz)[3]


def test_mask_words_and_tail(ctx, oracle):
    xyz = cloud_masks()
    g = FR.grid_regimes(xyz, 0.5)
    for per in (31, 32, 33, 64, 96, 128, 129, 150):
        assert (g.resident & (g.per_lane == per)).any(), per
    assert (g.resident & (g.np == 20) & (g.total == 300)).any() and (g.resident & (g.np == 40) & (g.total == 448)).any()
    n, _, _, agree = _check(ctx, oracle, xyz)
    assert agree and n.max() > 200  # hits in every mask word and in the tail
    assert xyz.shape[0] <= 6000


def test_resident_streamed_boundary(ctx, oracle):
    xyz = cloud_boundary()
    g = FR.grid_regimes(xyz, 0.5)
    for t in BOUNDARY_TOTAL:
        sel = (g.np == 30) & (g.total == t)
        assert sel.any() and (g.resident[sel] == (t <= 448)).all(), t
    col = (g.cx == 12) & (g.cy == 32)
    assert col.sum() == 3 and g.np[col].sum() == 1100 and g.total[col].max() == 1100  # ONE run of three chunks, the last one ragged
    assert _check(ctx, oracle, xyz)[3]
    assert xyz.shape[0] <= 6200


def test_too_few_neighbours(ctx, oracle):
    xyz = cloud_few()
    n, lg, cg, agree = _check(ctx, oracle, xyz)
    assert agree and (n == 1).sum() >= 2 and (n == 2).sum() == 2 and (n == 3).sum() == 3
    assert not lg[n < 3].any() and not cg[n < 3].any() and lg[n == 3, 0].all()


def test_strict_radius(ctx, oracle):
    xyz = cloud_strict()
    x = xyz.astype(np.float64)
    d2 = ((x[:, None] - x[None]) ** 2).sum(-1)  # exact in f64: every coordinate is a multiple of 2^-24 below 4
    on = d2 == 0.25
    assert on.sum() >= 2 * 3 * 6 * 64 and on[512, 513]  # pairs at exactly the radius
    assert 0.2499999 < d2[512, 514] < 0.25
    n, _, _, agree = _check(ctx, oracle, xyz)
    assert agree
    np.testing.assert_array_equal(n, (d2 < 0.25).sum(1))
    assert n[512] == 2 and n[513] == 1 and n[514] == 2


def test_grid_faces(ctx, oracle):
    rng = np.random.default_rng(107)
    plane = np.concatenate([rng.uniform(0, 6, (2000, 2)), np.zeros((2000, 1))], axis=1).astype(F)
    line = np.concatenate([rng.uniform(0, 20, (600, 1)), np.zeros((600, 2))], axis=1).astype(F)
    one = rng.uniform(0, 0.3, (50, 3)).astype(F)
    box = rng.uniform(0, 3, (3000, 3)).astype(F)
    g = FR.grid_regimes(plane, 0.5)
    assert g.dim[2] == 1 and g.dim[0] > 3 and g.dim[1] > 3
    g = FR.grid_regimes(line, 0.5)
    assert g.dim[1] == 1 and g.dim[2] == 1 and g.dim[0] > 30
    assert FR.grid_regimes(one, 0.5).dim.tolist() == [1, 1, 1]
    g = FR.grid_regimes(box, 0.5)
    for c, d in ((g.cx, 0), (g.cy, 1), (g.cz, 2)):
        assert g.dim[d] >= 3 and (c == 0).any() and (c == g.dim[d] - 1).any()
    for xyz in (plane, line, one, box):
        assert _check(ctx, oracle, np.ascontiguousarray(xyz))[3]


# ---------------------------------------------------------------- extent
WIDE_R = 0.3  # the radius of the widened-cell case


def _straddlers(mn, lo, hi, radius, step=4e-6):
    """Pairs (a, b) on the x axis, lo <= a < b <= hi, closer than the radius in f32, that the UNWIDENED table of a cloud whose corner is
    x = mn puts two cells apart: a is the last float of its cell, b the first float of the cell after the next.  Far from the corner
    v - mn is rounded to a float grid of pitch p, so a cell boundary moves by up to p / 2 and the cells of a and b can be one whole cell
    plus p apart where the points are not; the margin of 1e-4 cells is 0.12 p here.  (At a radius of 0.5 there is no such pair at any
    extent: 0.5 is a multiple of p, the cell is 0.2 p longer, and the nearest two-cell distance on the grid, less p, is the radius itself,
    which the strict test excludes.  Hence a radius of 0.3.)"""
    cell = F(radius) * F(1.0001)
    inv = F(F(1.0) / cell)
    v = np.arange(lo, hi, step).astype(F)
    c = np.floor(F(v - F(mn)) * inv).astype(np.int64)
    out = []
    for k in range(int(c[0]) + 2, int(c[-1])):
        ia, ib = np.searchsorted(c, k) - 1, np.searchsorted(c, k + 1)
        a, b = v[ia], v[ib]
        d = F(b - a)
        if c[ia] == k - 1 and c[ib] == k + 1 and F(d * d) < FR.r2_of(radius):
            out.append((float(a), float(b)))
    return out


def cloud_widened():
    """a line of clusters over 3 300 cells of x at a radius of 0.3, the table's corner at x = -1000, and at the far end (near x = 0, where
    floats are fine) pairs just inside the radius that straddle a whole cell of the unwidened table, each with a third point just outside"""
    rng = np.random.default_rng(108)
    mn, cell = -1000.0, float(F(WIDE_R) * F(1.0001))
    parts = [np.array([[mn, 0.0, 0.0]])]
    for t in range(33):
        parts.append(np.array([mn + (2 + 100 * t + 0.5) * cell, 0.0, 0.0]) + _offsets(9, rng) * [1, 0, 0])
    pairs = []
    for a, b in _straddlers(mn, 0.0, 16.0, WIDE_R):  # a few cells from one pair to the next: each point's neighbours are its own pair's
        if len(pairs) < 4 and (not pairs or a - pairs[-1][1] > 1.0):
            pairs.append((a, b))
    for a, b in pairs:
        far = F(b)
        while F(F(far - F(a)) * F(far - F(a))) < FR.r2_of(WIDE_R):
            far = np.nextafter(far, F(np.inf))
        parts.append(np.array([[a, 0, 0], [b, 0, 0], [float(far), 0, 0]]))
    return np.ascontiguousarray(np.concatenate(parts).astype(F)), pairs


def test_extent_widened_cell(ctx, oracle):
    xyz, pairs = cloud_widened()
    assert len(pairs) >= 2, "no straddling pair found"
    g0, g = FR.grid_regimes(xyz, WIDE_R, widen=False), FR.grid_regimes(xyz, WIDE_R)
    assert g.widened and g.coarsened == 0 and g.dim[0] > 3300 and g.dim[1] == 1 and g.dim[2] == 1 and g.ncell < 4000
    n3 = xyz.shape[0] - 3 * len(pairs)
    for t in range(len(pairs)):
        ia, ib = n3 + 3 * t, n3 + 3 * t + 1
        assert g0.coord[ib, 0] - g0.coord[ia, 0] == 2  # neighbours that the margin of 1e-4 alone loses ...
        assert g.coord[ib, 0] - g.coord[ia, 0] <= 1    # ... and the widened cell keeps
        assert g.coord[ia, 0] > 3300
    n, _, _, agree = _check(ctx, oracle, xyz, WIDE_R)
    for t in range(len(pairs)):
        assert n[n3 + 3 * t] == 2 and n[n3 + 3 * t + 1] >= 2  # a sees b; b sees a (and perhaps the point just outside a's radius)
    assert agree, "oracle.pca's counts differ from the brute force at 3 300 cells per axis"
    assert FR.grid_regimes(xyz, 0.5).widened and _check(ctx, oracle, xyz, 0.5)[3]  # and the same line at the default radius (2 000 cells)


def cloud_coarsened():
    """two groups 500 m apart on the diagonal (1 160 cells of 0.5 m per axis: 1.5e9 > 2^26), the far one near the origin with pairs just
    inside and just outside the radius across a boundary of the coarsened cell"""
    rng = np.random.default_rng(109)
    near = -290.0 + rng.uniform(0, 3, (400, 3))
    far = rng.uniform(0, 3, (400, 3))
    pre = np.concatenate([near, far]).astype(F)
    d = FR.grid_desc(pre, F(0.5) * F(1.0001))
    edge = (np.floor((0.0 - float(d.mn[0])) / float(d.cell)) + 1) * float(d.cell) + float(d.mn[0])  # the first cell boundary above x = 0
    a = F(edge - 0.25)
    trio = np.array([[a, 1.5, 1.5], [np.nextafter(F(a + F(0.5)), F(0)), 1.5, 1.5], [F(a - F(0.5)), 1.5, 1.5]], F)
    return np.ascontiguousarray(np.concatenate([pre, trio]))


def test_extent_coarsened_cell(ctx, oracle):
    xyz = cloud_coarsened()
    g = FR.grid_regimes(xyz, 0.5)
    assert g.widened and g.coarsened >= 1 and g.ncell <= (1 << 26) and float(g.cell) > 0.75
    assert ((xyz.max(0) - xyz.min(0)) / F(CELL)).prod() > (1 << 26)
    a, b, c = xyz.shape[0] - 3, xyz.shape[0] - 2, xyz.shape[0] - 1
    assert g.coord[b, 0] == g.coord[a, 0] + 1 and g.coord[a, 0] > 100  # the pair straddles a boundary of the far group's cells
    dab, dac = F(xyz[b, 0] - xyz[a, 0]), F(xyz[a, 0] - xyz[c, 0])
    assert F(dab * dab) < FR.r2_of(0.5) <= F(dac * dac)
    n, _, _, agree = _check(ctx, oracle, xyz)
    assert agree, "oracle.pca's counts differ from the brute force on a cloud of 1 160 cells per axis"
    nb = set(FR.neighbour_pairs(xyz, 0.5, [a])[1].tolist())
    assert b in nb and c not in nb


def test_run_deal(ctx, oracle):
    """more than 4 096 occupied cells (a second round of 512 runs, partly empty), their number no multiple of 8: cells of 1 to 2 points
    on a lattice of pitch 0.4 x the radius"""
    rng = np.random.default_rng(110)
    side = 17  # 4 125 of the 17^3 cells of a cube, one point in the middle part of each, a second one beside 1 500 of them
    i = np.arange(side ** 3)
    lat = np.stack([i % side, i // side % side, i // side ** 2], axis=1).astype(np.float64)
    cells = lat[rng.permutation(side ** 3)[:4125]]
    one = (cells + 0.5) * CELL + rng.uniform(-0.2, 0.2, (4125, 3))
    two = one[:1500] + rng.uniform(-0.03, 0.03, (1500, 3))
    xyz = np.ascontiguousarray(np.concatenate([np.zeros((1, 3)), one, two]).astype(F))
    g = FR.grid_regimes(xyz, 0.5)
    nc = g.keys.size
    nrun = (nc + 7) // 8
    assert nc > 4096 and nc % 8 != 0 and nrun > 512 and nrun % 512 != 0, (nc, nrun)
    assert g.np.max() <= 3 and (g.np == 1).any() and (g.np == 2).any()
    assert _check(ctx, oracle, xyz)[3]


# ---------------------------------------------------------------- the batched path
def test_batched_pca_on_the_crafted_clouds(ctx, api, oracle):
    """k_fb_pca_cells shares the cell body but has its own cloud lookup and run-crossing code: the crafted clouds in ONE batch, a cloud of
    3 occupied cells between two larger ones (a run of 8 cells crosses two cloud boundaries) and an empty cloud.  Every handle equals its
    recompute twin bit for bit, and its keypoints are oracle.nms(oracle.prune(...)) of the brute-force counts and the single-cloud
    eigenvalues; clusters of exactly min_neighbors points are rejected, of min_neighbors + 1 accepted."""
    cfg = api.pair_config(api.FEATURE_NONE, api.CORR_NN, dof=6, voxel=0.001, neighborhood_radius=0.5, radius_nonmax=0.6, max_iter=10)
    cfg.min_neighbors, cfg.ratio_max = MIN_N, 0.65
    rng = np.random.default_rng(111)
    three = np.ascontiguousarray(np.concatenate([_cluster((0, 0, 0), 6, rng), _cluster((4.4, 0, 0), 17, rng), _cluster((8.4, 0, 0), 18, rng)]).astype(F))
    empty = np.zeros((0, 3), F)
    first = cloud_lane_split()

    def ncells(raw):
        return FR.grid_regimes(raw[oracle.voxel_filter(raw, cfg.voxel)], 0.5).keys.size

    while ncells(first) % 8 not in (1, 2, 3, 4):  # the 3 cells of the next cloud then lie inside ONE run of 8 that begins in this cloud and ends in the one after
        first = np.ascontiguousarray(np.concatenate([first, np.array([[100.0 + 2.0 * (first.shape[0] % 50), 0.0, 0.0]], F)]))
    raws = [first, three, cloud_masks(), empty, cloud_second_pass(), cloud_boundary(), cloud_few(), cloud_strict()]
    single = [ctx.cloud_create(cfg, three) for _ in raws]
    batch = [ctx.cloud_create(cfg, three) for _ in raws]
    for c, r in zip(single, raws):
        c.recompute(r)
    ctx.clouds_recompute(batch, raws)
    nontrivial = 0
    for c, d, raw in zip(single, batch, raws):
        ia, ib = c.info(), d.info()
        assert (ia.n, ia.m, ia.k) == (ib.n, ib.m, ib.k)
        da, db = c.download(), d.download()
        for key in ("ds", "kp", "kp_xyz"):
            if da[key] is None or db[key] is None:
                assert da[key] is None and db[key] is None, key
            else:
                np.testing.assert_array_equal(da[key].cpu().numpy(), db[key].cpu().numpy(), err_msg=key)
        if raw.shape[0] == 0:
            assert ib.m == 0 and ib.k == 0
            continue
        keep = oracle.voxel_filter(raw, cfg.voxel)
        assert np.unique(keep).size >= raw.shape[0] - 1  # the filter keeps every crafted point (row 0 is its phantom copy of point 0)
        ds = np.ascontiguousarray(raw[keep])
        np.testing.assert_array_equal(db["ds"].cpu().numpy(), ds)
        g = FR.grid_regimes(ds, 0.5)
        if raw is three:
            assert g.keys.size == 3
        n = FR.radius_counts(ds, 0.5)
        lg, cg, ng = ctx.pca_curvature(ds, 0.5)
        np.testing.assert_array_equal(ng.cpu().numpy(), n)
        cand = oracle.prune(lg.cpu().numpy(), n, cfg.ratio_max, cfg.min_neighbors)
        kp = oracle.nms(ds, cg.cpu().numpy(), cand, cfg.reg.radius_nonmax)
        got = db["kp"].cpu().numpy() if db["kp"] is not None else np.zeros(0, np.int32)
        np.testing.assert_array_equal(got, kp)
        at, over = np.flatnonzero(n == MIN_N), np.flatnonzero(n == MIN_N + 1)
        assert not np.isin(kp, at).any()
        if raw is not three and raw is not raws[-1]:
            assert at.size >= 4 * MIN_N and over.size >= 8 * (MIN_N + 1)
            assert np.isin(kp, over).sum() >= 4  # accepted one neighbour above the threshold
            assert kp.size >= 10, kp.size
            nontrivial += 1
    assert nontrivial == 5
    for c in single + batch:
        c.close()
