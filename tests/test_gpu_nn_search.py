"""The spatial search under fine registration, on its own and on degenerate geometry: ghicp_nn_search (k_nn_fine / k_nn_coarse),
ghicp_cal_overlap (k_overlap) and the k-NN behind ghicp_knn_normals / ghicp_gicp_covariances, through the C ABI.

The reference of the 1-NN search and of the overlap count is a brute force over every target in numpy float32 that does not go through
oracle/: d2 = dx*dx; d2 += dy*dy; d2 += dz*dz, every step rounded to float32 (numpy does not fuse), ties to the lowest target index
(argmin takes the first minimum).  The search is specified as exact, so indices AND distance bits are compared with assert_array_equal;
nothing here has a tolerance.  Where it is cheap the CPU oracle's nn1 is held to the same brute force, which keeps the oracle pinned.

Targets (TARGETS): a line, a thin bar and a plane along / normal to every axis, all points identical, n = 1, 2, 3, two clusters 5000
apart, an exact lattice in shuffled order (queries on nodes, edge midpoints and cell centres: exact ties), a cloud smaller than the floor
of the cell size, clouds shifted by 1e3 .. 5e5, duplicated points, and clouds whose points lie exactly on the faces of the grid's cells.
The last are built on the 0.02 floor of the cell size: when the volume guess of build_index falls below the floor the cell is 0.02f (or
0.02f / 2^j after the occupancy halvings), so nodes at mn + k * 0.02f sit on cell faces.  A line along an axis is the same thing with one
cell across: every point has y = z = mn.

The k-NN consumers are compared with the CPU oracle at the equality / tolerance of test_gpu_icp.py (normals: 1e-6) and test_gpu_gicp.py
(covariances: bit-exact up to the N2 allowance of three rows).

On the host SIMT interpreter (GHICP_SIM=1) every case runs; the file takes a few minutes there."""
import numpy as np
import pytest

import gicp_restatement as G
from conftest import rot_err, trans_err
from test_gpu_gicp import _cov_parity

pytestmark = pytest.mark.gpu

F = np.float32
FLOOR = F(0.02)  # build_index: the cell size never starts below this


# ------------------------------------------------------------------------------------------------------------------------ reference
def brute_nn(q, t):
    """(index, d2) of the nearest target of every query: float32 brute force, ties to the lowest index"""
    q = np.ascontiguousarray(np.asarray(q)[:, :3], F)
    t = np.ascontiguousarray(np.asarray(t)[:, :3], F)
    nq, nt = len(q), len(t)
    idx = np.zeros(nq, np.int32)
    d2 = np.zeros(nq, F)
    step = max(1, (1 << 21) // nt)
    for s in range(0, nq, step):
        a = q[s:s + step]
        d = a[:, None, 0] - t[None, :, 0]
        d = d * d
        for c in (1, 2):
            e = a[:, None, c] - t[None, :, c]
            d += e * e
        assert d.dtype == F
        j = d.argmin(axis=1)
        idx[s:s + step] = j
        d2[s:s + step] = d[np.arange(len(a)), j]
    return idx, d2


def check_nn(ctx, q, t, labels=None, oracle=None):
    """ghicp_nn_search(q, t) == brute force, bit for bit; with `oracle`, oracle.nn1 too"""
    q, t = np.ascontiguousarray(q, F), np.ascontiguousarray(t, F)
    ib, db = brute_nn(q, t)
    ig, dg = ctx.nn_search(q, t)
    ig, dg = ig.cpu().numpy(), dg.cpu().numpy()
    bad = np.flatnonzero((ig != ib) | (dg.view(np.uint32) != db.view(np.uint32)))
    if bad.size:
        b = bad[0]
        what = labels[b] if labels is not None else "query"
        pytest.fail("%d of %d queries differ from the brute force; first: #%d (%s) %r -> index %d d2 %.9g, nearest is index %d d2 %.9g" % (
            bad.size, len(q), b, what, q[b, :3].tolist(), ig[b], dg[b], ib[b], db[b]))
    np.testing.assert_array_equal(ig, ib)
    np.testing.assert_array_equal(dg.view(np.uint32), db.view(np.uint32))
    if oracle is not None:
        io, do = oracle.nn1(q, t)
        np.testing.assert_array_equal(io, ib)
        np.testing.assert_array_equal(do.view(np.uint32), db.view(np.uint32))
    return ib, db


# ------------------------------------------------------------------------------------------------------------------------ targets
def _axes(v, a):
    """the (x, y, z) triple v with its first entry moved to axis a"""
    out = [v[1], v[2]]
    out.insert(a, v[0])
    return np.array(out)


def _line(a):
    return lambda rng: (rng.random((2000, 3)) * _axes([10.0, 0.0, 0.0], a)).astype(F)


def _bar(a):
    return lambda rng: (rng.random((2000, 3)) * _axes([10.0, 1e-3, 1e-3], a)).astype(F)


def _plane(a):
    return lambda rng: (rng.random((2500, 3)) * _axes([0.0, 8.0, 5.0], a) + _axes([1.5, -2.0, 0.5], a)).astype(F)


def _shifted(s):
    return lambda rng: (rng.random((2000, 3)) * [20.0, 15.0, 5.0] + np.array([s, -s, s])).astype(F)


def _lattice(rng):
    g = np.arange(12, dtype=np.float64) * 0.25 - 1.0  # every node, midpoint and centre is exact in float32
    t = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return t[rng.permutation(len(t))].astype(F)


def _clusters(rng):
    off = np.array([3000.0, -2500.0, 3122.0])  # |off| = 5000
    return np.vstack([rng.standard_normal((1000, 3)), rng.standard_normal((1000, 3)) + off]).astype(F)


def _cellface_plane(rng):
    """20 x 20 nodes at mn + k * 0.02f in a plane z = const: the volume guess is below the floor, one node per cell -> cell = 0.02f"""
    k = np.arange(20, dtype=F)
    x, y = F(0.5) + k * FLOOR, F(-0.3) + k * FLOOR
    t = np.stack(np.meshgrid(x, y, indexing="ij"), -1).reshape(-1, 2)
    t = np.hstack([t, np.full((len(t), 1), F(0.2))]).astype(F)
    return t[rng.permutation(len(t))]


def _cellface_block(rng):
    """6 x 6 x 6 nodes at mn + k * 0.02f, 5 points on each (1080 points: below the floor, 5 per occupied cell -> no halving)"""
    k = np.arange(6, dtype=F)
    x, y, z = F(-1.0) + k * FLOOR, F(2.0) + k * FLOOR, F(0.25) + k * FLOOR
    t = np.stack(np.meshgrid(x, y, z, indexing="ij"), -1).reshape(-1, 3)
    t = np.repeat(t, 5, axis=0).astype(F)
    return t[rng.permutation(len(t))]


def _cellface_halved(rng):
    """the same nodes with 12 points on each: the occupancy test halves the cell (0.02f / 2^j), the nodes stay on cell faces"""
    k = np.arange(5, dtype=F)
    x, y, z = F(0.0) + k * FLOOR, F(0.0) + k * FLOOR, F(0.0) + k * FLOOR
    t = np.stack(np.meshgrid(x, y, z, indexing="ij"), -1).reshape(-1, 3)
    t = np.repeat(t, 12, axis=0).astype(F)
    return t[rng.permutation(len(t))]


TARGETS = {
    "line_x": _line(0), "line_y": _line(1), "line_z": _line(2),
    "bar_x": _bar(0), "bar_y": _bar(1), "bar_z": _bar(2),
    "plane_x": _plane(0), "plane_y": _plane(1), "plane_z": _plane(2),
    "identical": lambda rng: np.tile(np.array([1.25, -3.5, 0.75], F), (500, 1)),
    "n1": lambda rng: rng.standard_normal((1, 3)).astype(F),
    "n2": lambda rng: rng.standard_normal((2, 3)).astype(F),
    "n3": lambda rng: rng.standard_normal((3, 3)).astype(F),
    "clusters": _clusters,
    "lattice": _lattice,
    "tiny": lambda rng: (rng.random((1500, 3)) * 1e-4 + [0.3, -0.2, 0.1]).astype(F),
    "shift_1e3": _shifted(1e3), "shift_1e5": _shifted(1e5), "shift_5e5": _shifted(5e5),
    "cellface_plane": _cellface_plane, "cellface_block": _cellface_block, "cellface_halved": _cellface_halved,
    "duplicates": lambda rng: (rng.random((700, 3)) * [6.0, 4.0, 2.0]).astype(F)[rng.integers(0, 700, 2000)],
    "generic": lambda rng: (rng.random((3000, 3)) * [20.0, 15.0, 5.0]).astype(F),
}


def _rng(name, salt=0):
    return np.random.default_rng([20261017, sorted(TARGETS).index(name), salt])


def query_sets(rng, t):
    """(label, queries) around target t: its own points, those shifted by 1e-3, Gaussians at 0.3 / 1 / 3 / 30 extents (the far ones are
    resolved on the coarse grid), Gaussians around the origin, points far outside the box, the faces and corners of the bounding box"""
    t64 = t.astype(np.float64)
    mn, mx = t64.min(0), t64.max(0)
    ext = float((mx - mn).max())
    s = ext if ext > 0 else 1.0
    c = 0.5 * (mn + mx)
    own = t64[rng.permutation(len(t))[:400]]
    yield "own points", own
    yield "own points + 1e-3", own + 1e-3
    yield "own points - 1e-3 in x", own - [1e-3, 0, 0]
    for f, n in ((0.3, 200), (1.0, 100), (3.0, 40), (30.0, 16)):  # few far ones: a far query walks many rings, slow on the interpreter
        yield "Gaussian at %g extents" % f, c + rng.standard_normal((n, 3)) * f * s
    yield "Gaussian around the origin, sigma 3", rng.standard_normal((300, 3)) * 3.0
    yield "far outside", np.array([[1e6, -1e6, 1e5], [-1e6, 0.0, 0.0], [0.0, 0.0, 1e6], [1e5, 1e5, 1e5]]) + c
    corners = np.array([[(mn, mx)[(b >> d) & 1][d] for d in range(3)] for b in range(8)])
    yield "bounding-box corners", corners
    yield "just outside the corners", corners + np.sign(corners - c) * 1e-3 * s
    for d in range(3):
        for side, v in (("min", mn[d]), ("max", mx[d])):
            p = mn + rng.random((30, 3)) * (mx - mn)
            p[:, d] = v
            yield "bounding-box face %s %s" % ("xyz"[d], side), p


def all_queries(rng, t):
    labels, qs = [], []
    for label, q in query_sets(rng, t):
        labels += [label] * len(q)
        qs.append(q)
    return labels, np.vstack(qs).astype(F)


# ------------------------------------------------------------------------------------------------------------------------ ghicp_nn_search
@pytest.mark.parametrize("name", list(TARGETS))
def test_nn_search_equals_brute_force(ctx, oracle, name):
    rng = _rng(name)
    t = TARGETS[name](rng)
    labels, q = all_queries(rng, t)
    check_nn(ctx, q, t, labels, oracle)


def test_nn_search_line_of_50_points(ctx, oracle):
    rng = np.random.default_rng(50)
    t = (rng.random((50, 3)) * [10.0, 0.0, 0.0]).astype(F)
    labels, q = all_queries(rng, t)
    check_nn(ctx, q, t, labels, oracle)


def test_nn_search_line_of_20000_cells(ctx):
    """2000 points on 400 m along x: the cell stays at the 0.02 floor, 20 000 cells on one axis.  The rounding of the cell coordinate
    grows with it (2.4e-7 cell per cell) and passes a flat 2e-3 cell there, so the pruning margin has to grow with the axis.  Queries
    stay near the line: one far from a grid this long walks thousands of rings."""
    rng = np.random.default_rng(20000)
    t = (rng.random((2000, 3)) * [400.0, 0.0, 0.0]).astype(F)
    own = t.astype(np.float64)
    q = np.vstack([own, own + [1e-5, 0, 0], own - [1e-5, 0, 0], own + [2e-4, 0, 0], own - [2e-4, 0, 0], own + rng.standard_normal((2000, 3)) * 0.03])
    labels = [l for l in ("own", "+1e-5", "-1e-5", "+2e-4", "-2e-4", "Gaussian 0.03") for _ in range(2000)]
    check_nn(ctx, q, t, labels)


def test_nn_search_lattice_ties(ctx, oracle):
    """Queries on the nodes, the edge midpoints and the cell centres of an exact lattice: 1, 2 and 8 targets at exactly the same distance,
    in cells on different sides of the query; the lowest index wins."""
    rng = _rng("lattice", 1)
    t = _lattice(rng)
    g = np.arange(12, dtype=np.float64) * 0.25 - 1.0
    nodes = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    sets = [("node", nodes)]
    for d in range(3):
        e = np.zeros(3)
        e[d] = 0.125
        sets.append(("midpoint of an edge along %s" % "xyz"[d], nodes + e))  # the last layer lies outside the box: one nearest node
    for d in range(3):
        e = np.full(3, 0.125)
        e[d] = 0.0
        sets.append(("centre of a face normal to %s" % "xyz"[d], nodes + e))
    sets.append(("cell centre", nodes + 0.125))
    sets.append(("cell centre, outside the low corner", nodes - 0.125))
    labels = [l for l, p in sets for _ in range(len(p))]
    q = np.vstack([p for _, p in sets]).astype(F)
    ib, db = check_nn(ctx, q, t, labels, oracle)
    inner = (q < g[-1]).all(axis=1) & np.array([l == "cell centre" for l in labels])  # the centres of the 11^3 cells of the lattice
    assert inner.sum() > 500 and (db[inner] == F(3 * 0.125 ** 2)).all()  # the ties are exact
    # the winner is the lowest index among the eight corners
    p = q[inner][:50]
    for k in range(len(p)):
        d = ((t.astype(np.float64) - p[k]) ** 2).sum(axis=1)
        tied = np.flatnonzero(d == d.min())
        assert tied.size == 8 and ib[np.flatnonzero(inner)[k]] == tied.min()


def test_nn_search_duplicated_targets_lower_index_wins(ctx):
    rng = _rng("duplicates", 1)
    b = (rng.random((900, 3)) * [6.0, 4.0, 2.0]).astype(F)
    t = np.vstack([b, b, b])
    ib, db = check_nn(ctx, b, t)
    np.testing.assert_array_equal(ib, np.arange(900))
    assert not db.any()
    perm = rng.permutation(len(t))
    ib, _ = check_nn(ctx, b, t[perm])
    first = np.full(900, len(t))
    np.minimum.at(first, perm % 900, np.arange(len(t)))
    np.testing.assert_array_equal(ib, first)


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025])
def test_nn_search_query_counts_around_a_workgroup(ctx, nq):
    """k_nn_fine runs one query per thread in workgroups of 256; a mix of near (fine grid) and far (pending) queries"""
    rng = np.random.default_rng(nq)
    t = (rng.random((1500, 3)) * [20.0, 15.0, 5.0]).astype(F)
    q = (rng.standard_normal((nq, 3)) * [30.0, 20.0, 10.0] + [10.0, 7.5, 2.5]).astype(F)
    if nq == 0:
        ig, dg = ctx.nn_search(q, t)
        assert ig.shape[0] == 0 and dg.shape[0] == 0
        return
    check_nn(ctx, q, t)


@pytest.mark.parametrize("nq", [16383, 16384, 16385, 16384 + 4133])
def test_nn_search_pending_queries_around_the_coarse_grid_launch(ctx, nq):
    """k_nn_coarse runs one wave per pending query on at most 4096 workgroups of 4 waves; beyond 16384 pending queries every wave takes
    several in a strided loop.  Every query here is pending: it lies outside the target's box on all three axes, 200 to 400 away on
    each, and the target (512 points in 16 x 8 x 4, a cell of 2 or 1 by build_index's volume guess) has at least 9 cells along x.  So
    the block of RCAP = 2 rings around the query's corner cell does not span x, its reach along x is at most |q_x - centre| + extent,
    and the nearest target is farther than that (asserted below on the test's own input): k_nn_fine cannot close the query.
    (Runs on the interpreter too.)"""
    rng = np.random.default_rng(nq)
    t = (rng.random((512, 3)) * [16.0, 8.0, 4.0]).astype(F)
    q = (rng.uniform(200.0, 400.0, (nq, 3)) * rng.choice([-1.0, 1.0], (nq, 3)) + [8.0, 4.0, 2.0]).astype(F)
    _, db = check_nn(ctx, q, t)
    assert (np.sqrt(db.astype(np.float64)) > np.abs(q[:, 0].astype(np.float64) - 8.0) + 16.0).all()


@pytest.mark.parametrize("sq,st", [(3, 3), (3, 4), (4, 3), (4, 4), (7, 5)])
def test_nn_search_strides(ctx, sq, st):
    """rows of 3, 4 and more floats on both arguments; the columns after z hold values that would win or lose every comparison"""
    rng = np.random.default_rng(100 * sq + st)
    t = (rng.random((1500, 3)) * [20.0, 15.0, 5.0]).astype(F)
    q = (rng.standard_normal((700, 3)) * [20.0, 15.0, 5.0] + [10.0, 7.5, 2.5]).astype(F)
    ib, db = brute_nn(q, t)
    qw = np.hstack([q, rng.choice(np.array([0.0, -1e9, 1e9], F), (len(q), sq - 3))]).astype(F)
    tw = np.hstack([t, rng.choice(np.array([0.0, -1e9, 1e9], F), (len(t), st - 3))]).astype(F)
    ig, dg = ctx.nn_search(qw, tw)
    np.testing.assert_array_equal(ig.cpu().numpy(), ib)
    np.testing.assert_array_equal(dg.cpu().numpy().view(np.uint32), db.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------ ghicp_cal_overlap
def overlap_ref(q, t, r):
    """calOverlap's float: (0.01 + #{queries with a target at d2 < r * r in float32}) / n1 (common_reg.cpp:313)"""
    _, d2 = brute_nn(q, t)
    r = F(r)
    count = int((d2 < r * r).sum())
    return F((0.01 + count) / float(len(q))), count


def ring_queries(rng, t, r, per=150):
    """Queries at r * (1 +- 2e-5) and r * (1 +- 1e-3) from a target point: in random directions, along the axes (the two points are then
    a whole cell apart) and around the extreme points of the cloud (the query falls into the one-cell pad of the grid)"""
    t64 = t.astype(np.float64)
    extreme = np.concatenate([t64.argmin(0), t64.argmax(0)])
    out = []
    for delta in (2e-5, -2e-5, 1e-3, -1e-3):
        j = np.concatenate([rng.integers(0, len(t), per), np.repeat(extreme, 7)])
        u = rng.standard_normal((len(j), 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        ax = np.vstack([np.eye(3), -np.eye(3)])
        u[:48] = ax[np.arange(48) % 6]
        u[per:] = np.tile(np.vstack([ax, [[0.6, 0.8, 0.0]]]), (6, 1))
        out.append(t64[j] + u * (float(F(r)) * (1.0 + delta)))
    return np.vstack(out).astype(F)


OVERLAP_CASES = {
    # name: (target, radius); extent / radius decides the branch of gh_grid_desc
    "extent 200 r": (lambda rng: rng.random((3000, 3)) * [20.0, 15.0, 5.0], 0.1),
    "extent 2000 r (widened cells)": (lambda rng: rng.random((3000, 3)) * [200.0, 10.0, 10.0], 0.1),
    "extent 2000 r, shifted": (lambda rng: rng.random((3000, 3)) * [60.0, 3.0, 3.0] + [1e3, -1e3, 1e3], 0.03),
    "shifted by 1e3": (lambda rng: rng.random((3000, 3)) * [20.0, 15.0, 5.0] + [1e3, -1e3, 1e3], 0.1),
    "line along x": (lambda rng: rng.random((2000, 3)) * [10.0, 0.0, 0.0], 0.05),
    "line along z": (lambda rng: rng.random((2000, 3)) * [0.0, 0.0, 10.0], 0.05),
    # the overlap grid's cell is the radius: nodes at a pitch of two radii lie on cell faces
    "on cell faces": (lambda rng: np.stack(np.meshgrid(*[np.arange(12) * 0.25] * 3, indexing="ij"), -1).reshape(-1, 3), 0.125),
    "identical": (lambda rng: np.tile([1.25, -3.5, 0.75], (300, 1)), 0.2),
}


@pytest.mark.parametrize("name", list(OVERLAP_CASES))
def test_cal_overlap_equals_brute_force(ctx, oracle, name):
    make, r = OVERLAP_CASES[name]
    rng = np.random.default_rng([7, list(OVERLAP_CASES).index(name)])
    t = np.asarray(make(rng)).astype(F)
    q = ring_queries(rng, t, r)
    want, count = overlap_ref(q, t, r)
    print("%s: %d of %d ring queries have a target inside r" % (name, count, len(q)))
    assert 0.1 * len(q) < count < 0.9 * len(q)  # of the test's own input: the ring queries fall on both sides of r
    assert F(ctx.cal_overlap(q, t, r)) == want
    assert F(oracle.cal_overlap(q, t, r)) == want
    # the cloud against itself and against a near copy; rows of 4 floats on both arguments
    mix = np.vstack([q[::3], t[:500], t[:500] + F(0.7 * r), t[:300] + F(40.0 * r)]).astype(F)
    want, _ = overlap_ref(mix, t, r)
    assert F(ctx.cal_overlap(mix, t, r)) == want
    pad = lambda a: np.hstack([a, np.full((len(a), 1), F(-1e9))]).astype(F)
    assert F(ctx.cal_overlap(pad(mix), pad(t), r)) == want
    # a query set entirely outside the padded grid: no neighbour at all
    ext = float((t.max(0) - t.min(0)).max()) + 1.0
    outside = np.vstack([t[:257] + F(3.0 * ext), t[:100] - F(2.0 * ext), [[1e6, -1e6, 1e5]]]).astype(F)
    assert F(ctx.cal_overlap(outside, t, r)) == F(0.01 / len(outside))
    # ... and just outside / just inside the pad of one cell
    lo = t.min(0).astype(np.float64)
    edge = np.vstack([lo - [0.999 * r, 0, 0], lo - [1.001 * r, 0, 0], lo - [2.5 * r, 0, 0], lo - 0.57 * r, lo - 0.58 * r]).astype(F)
    want, _ = overlap_ref(edge, t, r)
    assert F(ctx.cal_overlap(edge, t, r)) == want


# ------------------------------------------------------------------------------------------------------------------------ k-NN consumers
FALLBACK = np.full(3, 0.577, F)  # CheckNormals (pca.h:258-271): the normal of a point with fewer than 3 neighbours


@pytest.mark.parametrize("k", [5, 20])
@pytest.mark.parametrize("name", list(TARGETS))
def test_knn_normals_and_covariances_on_degenerate_clouds(ctx, oracle, name, k):
    rng = _rng(name, 2)
    t = TARGETS[name](rng)
    t = t[np.sort(rng.permutation(len(t))[:1200])]  # a random subset in the cloud's order: the geometry of every part of it is kept
    no = oracle.knn_normals(t, k)
    ng = ctx.knn_normals(t, k).cpu().numpy()
    assert np.isfinite(ng).all()
    assert np.abs(ng - no).max() <= 1e-6
    if len(t) < 3:  # k >= n and fewer than 3 neighbours: the documented fallback
        np.testing.assert_array_equal(ng, np.tile(FALLBACK, (len(t), 1)))
    else:
        unit = np.abs(np.linalg.norm(ng.astype(np.float64), axis=1) - 1.0) <= 1e-6
        assert (unit | (ng == FALLBACK).all(axis=1)).all()
    if name.startswith("plane_"):
        a = "xyz".index(name[-1])
        e = np.zeros(3)
        e[a] = 1.0
        assert (np.abs(np.abs(ng @ e) - 1.0) <= 1e-6).all()  # +-(plane normal)
        assert (np.sign(ng[:, a]) == -np.sign(t[:, a])).all()  # flipped towards the viewpoint at the origin
    cg = _cov_parity(ctx, oracle, t, k, name)
    assert np.isfinite(cg).all()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 19, 20, 21])
def test_knn_with_k_at_least_n(ctx, oracle, n):
    """k = 5 and k = 20 on clouds of up to 21 points: every point's list is the whole cloud, or all but the farthest"""
    rng = np.random.default_rng(n)
    t = rng.standard_normal((n, 3)).astype(F)
    for k in (5, 20):
        no = oracle.knn_normals(t, k)
        ng = ctx.knn_normals(t, k).cpu().numpy()
        assert np.isfinite(ng).all() and np.abs(ng - no).max() <= 1e-6
        if n < 3:
            np.testing.assert_array_equal(ng, np.tile(FALLBACK, (n, 1)))
        cg = _cov_parity(ctx, oracle, t, k, "n = %d" % n)
        assert np.isfinite(cg).all()


# ------------------------------------------------------------------------------------------------------------------------ end to end
def _bar_pair(axis, n=3000):
    """A thin bar (10 x 1e-3 x 1e-3) as target; the source is a rigidly displaced, sub-sampled, noisy copy lying off the bar's axis"""
    rng = np.random.default_rng(90 + axis)
    tgt = (rng.random((n, 3)) * _axes([10.0, 1e-3, 1e-3], axis)).astype(F)
    a = np.deg2rad(0.4)
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    if axis == 2:
        R = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    src = (tgt.astype(np.float64) - [0.3, -0.2, 0.25]) @ R  # a dozen cells off the axis: no run of the first searches is the query's own
    src = src[rng.permutation(len(src))[:int(0.8 * n)]]
    return (src + rng.normal(0.0, 1e-3, src.shape)).astype(F), tgt


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_icp_on_a_thin_bar(ctx, api, oracle, axis):
    """icp_reg, point to point, untrimmed: every iteration is one 1-NN search of off-axis queries in a thin target.  A wrong neighbour on
    such a target is a near-tie along the bar and moves T by far less than the bounds, so the correspondences of the first iteration
    (the search of the untransformed source) are compared index by index as well."""
    src, tgt = _bar_pair(axis)
    ro = oracle.icp(src, tgt, oracle.icp_params(25, False, False, 0, 0.5, 0.1))
    rg = ctx.icp(src, tgt, api.icp_params(25, False, False, 0, 0.5, 0.1))
    Tg, To = rg["T"].astype(np.float64), ro["T"].astype(np.float64)
    print("icp bar %d: iterations %d / %d correspondences %d / %d rot %.3g trans %.3g" % (
        axis, rg["iterations"], ro["iterations"], rg["correspondences"], ro["correspondences"], rot_err(Tg, To), trans_err(Tg, To)))
    assert rg["done"] == ro["done"] == 1 and rg["overlap"] == ro["overlap"]
    assert rg["iterations"] == ro["iterations"] and rg["reason"] == ro["reason"]
    assert rg["correspondences"] == ro["correspondences"] == len(src)
    assert rg["mse"] == pytest.approx(ro["mse"], rel=1e-9)  # the same correspondences: the same sum of squared distances
    assert rot_err(Tg, To) <= 1e-4 and trans_err(Tg, To) <= 1e-3
    # the first iteration's correspondences, the oracle's and the GPU's, are the brute force's
    ib, _ = check_nn(ctx, src, tgt)
    np.testing.assert_array_equal(ro["corr0"], ib)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_gicp_on_a_thin_bar(ctx, api, oracle, axis):
    src, tgt = _bar_pair(axis, 1500)  # small: the inner solver is slow on the interpreter
    ro = G.gicp(oracle, src, tgt, G.params(10, False, False, 0.5, 0.1, 20))
    rg = ctx.gicp(src, tgt, api.gicp_params(10, False, False, 0.5, 0.1, 20))
    Tg, To = rg["T"].astype(np.float64), ro["T"].astype(np.float64)
    print("gicp bar %d: iterations %d / %d correspondences %d / %d rot %.3g trans %.3g" % (
        axis, rg["iterations"], ro["iterations"], rg["correspondences"], ro["correspondences"], rot_err(Tg, To), trans_err(Tg, To)))
    assert rg["done"] == ro["done"] == 1 and rg["overlap"] == ro["overlap"]
    assert rg["iterations"] == ro["iterations"] and rg["reason"] == ro["reason"]
    assert rg["correspondences"] == ro["correspondences"]
    assert rot_err(Tg, To) <= 1e-4 and trans_err(Tg, To) <= 1e-3
    check_nn(ctx, src, tgt)  # the search of the first outer iteration
