"""Greedy non-maximum suppression at the edges of its regimes, exact: same keypoint ids in the same order, no tolerances.

Part A drives the one-workgroup sweep (gh_nms_greedy_cloud of nms_dev.h, through ghicp_nms) with hand-built candidates whose rank is known:
counts around a wave and a chunk, a suppressor in the same wave / the next wave / the next chunk, the crossing from the LDS list to the
global grid at NMS_SEL_CAP selected keypoints, the column cap NMS_COL_CAP, the widening and coarsening branches of gh_grid_desc, a
distance exactly at R, plateaus of equal curvature and odd keys.  Part B drives the batched decision rounds (k_fb_nmsr_* of batch_nms.hip,
through ghicp_clouds_recompute) with lattice "ribbons" whose PCA curvature forms long chains of decisions or long plateaus.

Two CPU references must agree with each other before the GPU is asked: the oracle (oracle.nms / oracle.keypoints) and the plain greedy
sweep below, which has no grid at all -- the oracle's Grid and the kernel's GridDesc are both cell tables of side R * 1.0001 and could
share a mistake.  gh_grid_desc is restated here in f32 only to ASSERT that a fixture lands in the regime it was built for."""
import os
import re
from collections import defaultdict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
R = 1.5
# what the fixtures were built for; test_the_caps_are_what_the_fixtures_were_built_for compares them with the sources
NMS_T, NMS_SEL_CAP, NMS_COL_CAP, FB_NMS_ROUNDS, RANK_TILE = 256, 3072, 16384, 16, 1024


# ---------------------------------------------------------------------------------------------------------------- references
def ref_nms(xyz, curv, cand, radius):
    """Plain greedy NMS: stable argsort by curvature descending, keep a candidate iff no kept one is closer than R.  The distance as
    the numerics contract spells it (f32, d2 = dx*dx; d2 += dy*dy; d2 += dz*dz, every operation rounded on its own), strict d2 < r2."""
    xyz = np.asarray(xyz, F)
    cand = np.asarray(cand, np.int64)
    r2 = F(np.float64(F(radius)) * np.float64(F(radius)))
    order = np.argsort(-np.asarray(curv, np.float64)[cand], kind="stable")
    P = np.ascontiguousarray(xyz[cand[order], :3])
    kept = np.empty((max(1, len(cand)), 3), F)
    n, out = 0, []
    for r in range(len(order)):
        if n:
            d = kept[:n] - P[r]
            d2 = d[:, 0] * d[:, 0]
            d2 += d[:, 1] * d[:, 1]
            d2 += d[:, 2] * d[:, 2]
            if (d2 < r2).any():
                continue
        kept[n] = P[r]
        n += 1
        out.append(cand[order[r]])
    return np.array(out, np.int32)


def grid_desc(pts, radius):
    """gh_grid_desc (grid.h) over the box of pts for the cell radius * 1.0001f, in f32 as the host computes it."""
    pts = np.asarray(pts, F)[:, :3]
    mn, mx = pts.min(axis=0), pts.max(axis=0)
    cell = F(radius) * F(1.0001)
    ext = F(max(mx[d] - mn[d] for d in range(3)))
    dims = ext / cell
    widened = bool(dims > F(256.0))
    if widened:
        cell = cell * (F(1.0) + F(4e-7) * dims)
    coarsened = 0
    while True:
        inv = F(1.0) / cell
        dim = [max(1, int(np.floor((mx[d] - mn[d]) * inv)) + 1) for d in range(3)]
        ncell = dim[0] * dim[1] * dim[2]
        if ncell <= 1 << 26:
            break
        cell = cell * F(1.5)
        coarsened += 1
    return dict(dim=dim, ncell=ncell, ncol=dim[0] * dim[1], widened=widened, coarsened=coarsened, inv=inv, mn=mn)


def test_the_caps_are_what_the_fixtures_were_built_for():
    """The regime asserts below use the constants of this file: a changed cap must fail here, loudly, not move a fixture into another regime."""
    src = os.path.join(ROOT, "gh-icp_amd", "csrc")
    dev, batch = open(os.path.join(src, "nms_dev.h")).read(), open(os.path.join(src, "batch_dev.h")).read() + open(os.path.join(src, "batch_nms.hip")).read()
    for text, name, want in ((dev, "NMS_T", NMS_T), (dev, "NMS_SEL_CAP", NMS_SEL_CAP), (dev, "NMS_COL_CAP", NMS_COL_CAP), (batch, "FB_NMS_ROUNDS", FB_NMS_ROUNDS)):
        m = re.search(r"constexpr int %s = (\d+);" % name, text)
        assert m and int(m.group(1)) == want, name
    assert "s_key[%d]" % RANK_TILE in batch and "q0 += %d" % RANK_TILE in batch  # the rank pass's tile


# ---------------------------------------------------------------------------------------------------------------- Part A helpers
def _pack(P, rng, stride, curv_of_rank=None):
    """Rank-ordered points P -> (xyz, curvature, cand, index of rank r).  stride 3: cand is the identity over a shuffled store; stride 4:
    cand is a shuffled subset of a larger cloud whose other rows sit exactly on candidates and carry the largest curvature."""
    P = np.asarray(P, F).reshape(-1, 3)
    n = len(P)
    if curv_of_rank is None:
        curv_of_rank = 1.0 - np.arange(n, dtype=np.float64) / (n + 1)  # strictly decreasing in the rank
    if stride == 3:
        idx = rng.permutation(n)
        xyz = np.empty((n, 3), F)
        curv = np.empty(n, np.float64)
        xyz[idx], curv[idx] = P, curv_of_rank
        return xyz, curv, np.arange(n, dtype=np.int32), idx
    m = n + n // 2 + 3
    idx = rng.permutation(m)[:n]
    xyz = np.zeros((m, 4), F)
    if n:
        xyz[:, :3] = P[rng.integers(0, n, m)]
    xyz[:, 3] = F(7e8)
    curv = np.full(m, 9.0)
    xyz[idx, :3], curv[idx] = P, curv_of_rank
    return xyz, curv, idx[rng.permutation(n)].astype(np.int32), idx


def _check(ctx, oracle, xyz, curv, cand, radius=R, expect=None, twice=False):
    want = ref_nms(xyz, curv, cand, radius)
    np.testing.assert_array_equal(oracle.nms(xyz, curv, cand, radius), want, err_msg="the two CPU references disagree: the fixture is at fault")
    if expect is not None:
        np.testing.assert_array_equal(want, np.asarray(expect, np.int32), err_msg="the fixture does not have the answer it was built for")
    got = ctx.nms(xyz, curv, cand, radius).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    if twice:  # A7: the same context, the same buffers, bit-identical
        again = ctx.nms(xyz, curv, cand, radius).cpu().numpy()
        assert again.dtype == got.dtype and again.tobytes() == got.tobytes()
    return want


def _lattice2(n, step, nx=None):
    nx = nx or int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    return np.stack([(i % nx) * step, (i // nx) * step, np.zeros(n)], axis=1).astype(F)


def _lattice3(n, step):
    s = 1
    while s * s * s < n:
        s += 1
    i = np.arange(n)
    return np.stack([(i % s) * step, ((i // s) % s) * step, (i // (s * s)) * step], axis=1).astype(F)


def _cand_box(xyz, cand):
    return np.asarray(xyz, F)[np.asarray(cand, np.int64), :3]


# ---------------------------------------------------------------------------------------------------------------- A1
@pytest.mark.parametrize("layout", ["far", "ball", "alternating"])
def test_counts_around_a_wave_and_a_chunk(ctx, oracle, layout):
    rng = np.random.default_rng(11)
    for c in (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025):
        for stride in (3, 4):
            if layout == "far":  # all farther apart than R: all selected
                P = _lattice2(c, 1.25 * R)[rng.permutation(c)]
                sel = np.arange(c)
            elif layout == "ball":  # all inside one ball of radius R / 2: one selected
                v = rng.normal(size=(c, 3))
                P = (v / np.linalg.norm(v, axis=1, keepdims=True) * (rng.random((c, 1)) * 0.49 * R) + 5.0).astype(F)
                sel = np.arange(1)
            else:  # rank 2k at a site of its own, rank 2k + 1 within R of it
                sites = _lattice2((c + 1) // 2, 2.5 * R)[rng.permutation((c + 1) // 2)]
                P = np.repeat(sites, 2, axis=0)[:c]
                P[1::2] += np.array([0.3 * R, -0.2 * R, 0.1 * R], F)
                sel = np.arange(0, c, 2)
            xyz, curv, cand, idx = _pack(P, rng, stride)
            _check(ctx, oracle, xyz, curv, cand, expect=idx[sel])


# ---------------------------------------------------------------------------------------------------------------- A2
def test_where_the_suppressor_sits(ctx, oracle):
    """b within R of a, everything else far away, at ranks r and r + d: the same wave, the next wave of the chunk, the next chunk, a chunk
    far later.  1331 sites of a cube lattice: 41 x 41 columns, the per-column LDS lists."""
    rng = np.random.default_rng(12)
    n = 1331
    base = _lattice3(n, 4.0 * R)
    assert grid_desc(base, R)["ncol"] <= NMS_COL_CAP
    k = 0
    for r in (0, 63, 200):
        for d in (1, 63, 64, 65, 255, 256, 257, 1000):
            P = base[rng.permutation(n)]
            P[r + d] = P[r] + np.array([0.5 * R, 0.0, 0.0], F)[[k % 3, (k + 1) % 3, (k + 2) % 3]] * F(1 if k % 2 else -1)
            xyz, curv, cand, idx = _pack(P, rng, 3 + k % 2)
            _check(ctx, oracle, xyz, curv, cand, expect=np.delete(idx, r + d), twice=True)
            k += 1


@pytest.mark.parametrize("wide", [False, True])
def test_a_suppressed_candidate_suppresses_nobody(ctx, oracle, wide):
    """a -> b -> c with b within R of a, c within R of b but not of a: c is selected.  The three in one wave, across two waves, across two
    chunks; with the column lists and with the sweep of the LDS list (more than NMS_COL_CAP columns)."""
    rng = np.random.default_rng(13)
    n = 1331
    base = _lattice2(n, 4.0 * R) if wide else _lattice3(n, 4.0 * R)
    assert (grid_desc(base, R)["ncol"] > NMS_COL_CAP) == wide and not grid_desc(base, R)["widened"]
    for k, (ra, rb, rc) in enumerate([(10, 11, 12), (0, 1, 63), (60, 64, 70), (10, 70, 130), (100, 191, 192), (250, 256, 300), (255, 256, 257), (100, 300, 600), (3, 700, 1330)]):
        P = base[rng.permutation(n)]
        axis = np.eye(3, dtype=F)[k % 2]  # x or y
        P[rb] = P[ra] + F(0.8 * R) * axis
        P[rc] = P[ra] + F(1.6 * R) * axis
        xyz, curv, cand, idx = _pack(P, rng, 3 + k % 2)
        _check(ctx, oracle, xyz, curv, cand, expect=np.delete(idx, rb), twice=True)


# ---------------------------------------------------------------------------------------------------------------- A3
_OFF = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], np.float64) * 0.3 * R  # 0.52 R from the leader, > R from every other site


def _followers(K):
    """(p, q): a candidate within R of the keypoint at final position p, ranked right behind the keypoint at position q >= p."""
    spec = [(0, 3500), (5, 3400), (1000, 3300), (3000, 3200), (3070, 3100), (2047, 6999), (17, 3071),  # early keypoints, tested after the crossing
            (3071, 3071), (3072, 3072), (3073, 3073), (3071, 3080), (3072, 3090), (3073, 6999),  # the keypoints at the cap
            (5000, 5000), (5000, 6999), (6999, 6999), (6500, 6900),  # far beyond
            (3070, 3072), (100, 3072), (3072, 3073),  # in the very wave that crosses
            (0, K - 1), (3071, K - 1), (3072, K - 1), (K - 1, K - 1), (K // 2, K - 1), (K // 2, K // 2)]
    return sorted({(p, q) for p, q in spec if 0 <= p <= q < K})


def _crossing_fixture(K, wide, with_followers, rng):
    sites = (_lattice2(K, 3.0 * R, nx=85) if wide else _lattice3(K, 1.25 * R))[rng.permutation(K)]  # sites[p]: the keypoint at final position p
    behind = defaultdict(list)
    if with_followers:
        for j, (p, q) in enumerate(_followers(K)):
            behind[q].append(sites[p].astype(np.float64) + _OFF[j % 8])
    P, sel = [], []
    for q in range(K):
        P.append(sites[q])
        sel.append(len(P) - 1)
        P.extend(behind[q])
    P = np.asarray(P, F)
    g = grid_desc(P, R)
    assert (g["ncol"] > NMS_COL_CAP) == wide and not g["widened"] and not g["coarsened"], g
    return P, np.asarray(sel)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("with_followers", [False, True])
def test_the_crossing_into_the_global_grid(ctx, oracle, wide, with_followers):
    """A lattice in which every site is selected, K sites around NMS_SEL_CAP: from position 3072 on a keypoint exists only in the per-cell
    lists in global memory, which must hold the earlier keypoints too.  Followers: lower-ranked candidates within R of one keypoint each."""
    rng = np.random.default_rng(14 + 2 * wide + with_followers)
    for k, K in enumerate((3071, 3072, 3073, 3072 + 64, 3072 + 257, 7000)):
        P, sel = _crossing_fixture(K, wide, with_followers, rng)
        assert len(P) <= 20_000
        if with_followers and K > NMS_SEL_CAP:  # a follower shares the wave in which the list crosses the cap
            wave = sel[NMS_SEL_CAP] // 64
            assert any(r // 64 == wave for r in np.setdiff1d(np.arange(len(P)), sel))
        xyz, curv, cand, idx = _pack(P, rng, 3 + k % 2)
        _check(ctx, oracle, xyz, curv, cand, expect=idx[sel], twice=True)


# ---------------------------------------------------------------------------------------------------------------- A4
def _scatter_with_pairs(ext_x, ext_y, rng, nx=41, ny=41):
    """nx x ny sites that span the box exactly (its corners are sites), two z layers, a partner within ~R of every third site; ranks are random."""
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    S = np.stack([gx.ravel() * (np.float64(ext_x) / (nx - 1)), gy.ravel() * (np.float64(ext_y) / (ny - 1)), (gx.ravel() % 2) * 0.4 * R], axis=1)
    lead = S[2::3]
    v = rng.normal(size=lead.shape)
    v[:, 2] *= 0.2
    near = lead + v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.2 * R, 1.2 * R, (len(lead), 1))
    near[:, 0] = np.clip(near[:, 0], 0, ext_x)
    near[:, 1] = np.clip(near[:, 1], 0, ext_y)
    P = np.concatenate([S, near]).astype(F)
    P[:, 0] = np.minimum(P[:, 0], F(ext_x))
    P[:, 1] = np.minimum(P[:, 1], F(ext_y))
    return P[rng.permutation(len(P))]


@pytest.mark.parametrize("rows", [128, 129])
def test_the_column_cap(ctx, oracle, rows):
    """128 x 128 = NMS_COL_CAP columns (the per-column lists, every head in use) and 128 x 129 (the sweep of the LDS list)."""
    rng = np.random.default_rng(15)
    cell = F(R) * F(1.0001)
    P = _scatter_with_pairs(F(127.5) * cell, F(rows - 0.5) * cell, rng)
    xyz, curv, cand, _ = _pack(P, rng, 3 + rows % 2)
    g = grid_desc(_cand_box(xyz, cand), R)
    assert g["dim"][:2] == [128, rows] and g["ncol"] == 128 * rows and (g["ncol"] <= NMS_COL_CAP) == (rows == 128), g
    want = _check(ctx, oracle, xyz, curv, cand, twice=True)
    assert 1681 < len(want) < len(P)  # pairs on both sides of R


def test_widened_cells_beyond_256_per_axis(ctx, oracle):
    """Candidates strung along 600 m: 400 cells along x, so gh_grid_desc widens the cell.  Close pairs at the far end, where the rounding of
    (v - mn) * inv is largest, at distances just inside, at and just outside R."""
    rng = np.random.default_rng(16)
    x = np.concatenate([np.arange(240) * 2.0, 482.0 + np.arange(30) * 4.0, [600.0]])  # 2 m apart, then 4 m apart at the far end
    line = np.stack([x, rng.uniform(-0.2, 0.2, len(x)), rng.uniform(-0.2, 0.2, len(x))], axis=1)
    far = line[240:270]
    d = np.resize(np.array([0.9999, 0.99999, 1.0, 1.00001, 1.0001, 0.75]), len(far))[:, None] * R
    mate = far + np.concatenate([d, np.zeros((len(far), 2))], axis=1)  # along x
    P = np.concatenate([line, mate]).astype(F)
    P = P[rng.permutation(len(P))]
    xyz, curv, cand, _ = _pack(P, rng, 4)
    g = grid_desc(_cand_box(xyz, cand), R)
    assert g["widened"] and not g["coarsened"] and g["dim"][0] > 256, g
    want = _check(ctx, oracle, xyz, curv, cand)
    assert len(line) <= len(want) < len(P)  # some partners inside R, some not


def test_coarsened_cells_beyond_2_26(ctx, oracle):
    """The corners of a 700 m cube and a cluster: 467^3 cells of side R are more than 2^26, so the cell grows by 1.5."""
    rng = np.random.default_rng(17)
    corners = np.array([[x, y, z] for x in (0.0, 700.0) for y in (0.0, 700.0) for z in (0.0, 700.0)])
    cluster = 350.0 + rng.uniform(-4.0, 4.0, (400, 3))
    P = np.concatenate([corners, cluster, corners[1:] * 0.999]).astype(F)
    P = P[rng.permutation(len(P))]
    xyz, curv, cand, _ = _pack(P, rng, 3)
    g = grid_desc(_cand_box(xyz, cand), R)
    assert g["widened"] and g["coarsened"] == 1 and g["ncell"] <= 1 << 26, g
    want = _check(ctx, oracle, xyz, curv, cand)
    assert 16 < len(want) < len(P)


def test_negative_coordinates_and_a_box_far_from_the_origin(ctx, oracle):
    rng = np.random.default_rng(18)
    P = _scatter_with_pairs(60.0, 45.0, rng, nx=21, ny=16).astype(np.float64)
    for shift in ([-30.0, -22.5, -0.3], [-250.3, 1234.7, -77.1], [4096.0, -8192.0, 512.0]):
        Q = (P + np.array(shift)).astype(F)
        xyz, curv, cand, _ = _pack(Q, rng, 3)
        want = _check(ctx, oracle, xyz, curv, cand)
        assert 250 < len(want) < len(Q)


# ---------------------------------------------------------------------------------------------------------------- A5
def _sum_unfused(d):
    d = d.astype(F)
    s = d[..., 0] * d[..., 0]
    s = s + d[..., 1] * d[..., 1]
    return s + d[..., 2] * d[..., 2]


def _sum_fused(d):
    """what fma(dz, dz, fma(dy, dy, dx * dx)) gives: a product of two f32 is exact in f64 and the sums below stay within 53 bits of the result's exponent"""
    d = d.astype(F).astype(np.float64)
    s = (d[..., 0] * d[..., 0]).astype(F).astype(np.float64)
    s = (s + d[..., 1] * d[..., 1]).astype(F).astype(np.float64)
    return (s + d[..., 2] * d[..., 2]).astype(F)


def _boundary_pairs(rng, sites):
    """Per site a partner: exactly at R (axis-aligned, d2 == r2), one ulp inside, and off-axis partners for which the contract's unfused sum
    and a fused one fall on different sides of r2 (seeded search over the PLACED coordinates: d = partner - site in f32, as the kernel forms it)."""
    r2 = F(np.float64(F(R)) ** 2)
    pairs, kinds = [], []
    it = iter(sites)
    for axis in range(3):
        for sign in (1.0, -1.0):
            a = next(it)
            b = a.copy()
            b[axis] = a[axis] + F(sign * R)
            assert _sum_unfused(b - a) == r2
            pairs.append((a, b)); kinds.append("at")
            a = next(it)
            b = a.copy()
            b[axis] = np.nextafter(a[axis] + F(sign * R), a[axis])
            assert _sum_unfused(b - a) < r2
            pairs.append((a, b)); kinds.append("inside")
    want = {"in_unfused_only": 6, "in_fused_only": 6}
    while any(want.values()):
        a = next(it)
        v = rng.normal(size=3)
        v = v / np.linalg.norm(v) * R
        b0 = (a.astype(np.float64) + v).astype(F)
        ax = int(np.argmax(np.abs(v)))
        for steps in range(-40, 41):  # walk the partner's largest component through its neighbouring floats
            b = b0.copy()
            b[ax] = (b0[ax:ax + 1].view(np.int32) + np.int32(steps)).view(F)[0]  # |b| > 0: the next floats are the next integers
            d = b - a
            u, f = _sum_unfused(d) < r2, _sum_fused(d) < r2
            kind = "in_unfused_only" if (u and not f) else ("in_fused_only" if (f and not u) else None)
            if kind and want[kind]:
                want[kind] -= 1
                pairs.append((a, b)); kinds.append(kind)
                break
    return pairs, kinds


def test_a_distance_exactly_at_R(ctx, oracle):
    rng = np.random.default_rng(19)
    # sites 5 R apart at odd offsets (partners fall on either side of cell boundaries), some on the negative side
    sites = iter((_lattice3(4000, 5.0 * R) + np.array([-37.0, 0.37, -11.1], F))[rng.permutation(4000)])
    pairs, kinds = _boundary_pairs(rng, sites)
    assert kinds.count("at") == 6 and kinds.count("inside") == 6 and kinds.count("in_unfused_only") == 6 and kinds.count("in_fused_only") == 6
    P, sel = [], []
    for j, (a, b) in enumerate(pairs):
        lo, hi = (a, b) if j % 2 else (b, a)
        P += [lo, hi]
    P = np.asarray(P, F)
    order = rng.permutation(len(pairs))  # pairs in random rank order, the first of a pair right before the second
    P = P.reshape(-1, 2, 3)[order].reshape(-1, 3)
    kinds = [kinds[j] for j in order]
    r2 = F(np.float64(F(R)) ** 2)
    expect_sel = []
    for j, kind in enumerate(kinds):
        expect_sel.append(2 * j)
        if kind in ("at", "in_fused_only"):
            expect_sel.append(2 * j + 1)  # d2 >= r2 under the contract: not suppressed
    g = grid_desc(P, R)
    cell = lambda p: tuple(int(np.floor((p[d] - g["mn"][d]) * g["inv"])) for d in range(3))
    crossing = {kind for j, kind in enumerate(kinds) if cell(P[2 * j]) != cell(P[2 * j + 1])}
    together = {kind for j, kind in enumerate(kinds) if cell(P[2 * j]) == cell(P[2 * j + 1])}
    assert crossing == {"at", "inside", "in_unfused_only", "in_fused_only"}, crossing  # every kind has a pair across a cell boundary
    print("kinds with a pair inside one cell:", sorted(together))
    for stride in (3, 4):
        xyz, curv, cand, idx = _pack(P, rng, stride)
        _check(ctx, oracle, xyz, curv, cand, expect=idx[np.asarray(expect_sel)])


# ---------------------------------------------------------------------------------------------------------------- A6
def test_ties_and_odd_keys(ctx, oracle):
    """Plateaus of bit-identical curvature longer than a wave and longer than a chunk with close pairs inside: the lower CANDIDATE position
    wins.  Denormal and negative curvatures; +0.0 next to -0.0, which compare equal (the oracle's comparator is >), so candidate order decides."""
    rng = np.random.default_rng(20)
    levels = [(2.0, 100), (1.0, 300), (5e-324, 70), (0.0, 40), (-0.0, 40), (-5e-324, 70), (-1.0, 80), (-1.7e308, 30)]
    n = sum(k for _, k in levels)
    sites = _lattice3((n + 1) // 2, 3.0 * R)
    P0 = np.repeat(sites, 2, axis=0)[:n].astype(np.float64)
    P0[1::2] += np.array([0.4 * R, 0.3 * R, -0.2 * R])  # every site has a partner within R ...
    perm = rng.permutation(n)  # ... at a random place of the level sequence, on the same plateau or on another
    P = P0[perm].astype(F)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    partner = inv[perm ^ 1]  # i -> the i of the other member of its pair (n is even)
    assert n % 2 == 0 and (partner[partner] == np.arange(n)).all()
    m = n + 200
    store = rng.permutation(m)[:n]
    xyz = np.zeros((m, 3), F)
    xyz[:] = P[rng.integers(0, n, m)]
    xyz[store] = P
    lev = np.concatenate([np.full(k, v) for v, k in levels])
    lev[470:550] = np.where(rng.integers(0, 2, 80) == 1, 0.0, -0.0)  # the two zero levels: the signs interleaved
    for i in range(470, 550, 5):  # and sixteen pairs of one zero of each sign
        lev[partner[i]] = -lev[i]
    curv = np.full(m, 9.0)
    curv[store] = lev
    cand = store[rng.permutation(n)].astype(np.int32)
    want = _check(ctx, oracle, xyz, curv, cand, twice=True)
    # the fixture decides ties: pairs on one plateau, and pairs of zeros of different sign in which the NEGATIVE zero comes first in candidate order
    pos = {int(c): i for i, c in enumerate(cand)}
    sel = set(want.tolist())
    same = [(i, int(partner[i])) for i in range(n) if i < partner[i] and lev[i] == lev[partner[i]]]
    assert len(same) >= 20 and any(lev[i] == 1.0 for i, _ in same) and any(lev[i] == 2.0 for i, _ in same)
    neg_first = 0
    for i, j in same:
        first, second = (i, j) if pos[int(store[i])] < pos[int(store[j])] else (j, i)
        assert int(store[first]) in sel and int(store[second]) not in sel  # nothing else is within R of either
        neg_first += int(lev[i] == 0 and np.signbit(lev[first]) and not np.signbit(lev[second]))
    assert neg_first >= 1, "no +0.0 / -0.0 pair in which the candidate order and the sign bit disagree: reseed"
    # all equal, longer than two chunks, identity candidates: the sweep in storage order
    xyz2, _, cand2, _ = _pack(P[:600], rng, 3)
    _check(ctx, oracle, xyz2, np.full(600, 0.25), cand2, twice=True)
    assert ctx.nms(xyz2, np.zeros(600), np.zeros(0, np.int32), R).shape[0] == 0


# ---------------------------------------------------------------------------------------------------------------- Part B helpers
VOXEL, R_PCA = 0.2, 1.0


def _ribbon(L, W=4, T=2, grow=0.0, x0=0.0, mirror=False, s=0.25):
    """L x W x T lattice points, s apart (more than the voxel: the voxel filter keeps every point; multiples of a power of two: the f64
    scatter sums of the PCA are exact, so translation along x gives bit-identical curvature).  Narrower than the PCA ball, so the
    eigenvalue ratios pass prune.  grow > 0: the z spacing grows by `grow` per column, curvature rises strictly along x."""
    i, j, k = np.meshgrid(np.arange(L), np.arange(W), np.arange(T), indexing="ij")
    x = i * s
    if mirror:
        x = (L - 1) * s - x
    return np.stack([x + x0, j * s, k * (s + i * grow)], axis=-1).reshape(-1, 3).astype(F)


def _cfg(api, radius_nonmax=R):
    return api.pair_config(api.FEATURE_NONE, api.CORR_NN, dof=6, voxel=VOXEL, neighborhood_radius=R_PCA, radius_nonmax=radius_nonmax, max_iter=10)


_REF = {}


def _reference(oracle, raw, radius_nonmax=R):
    """(down-sampled cloud, curvature, candidates, keypoints) of a raw cloud from the CPU: computed once per cloud, the two references compared."""
    key = (raw.shape, raw.tobytes(), float(radius_nonmax))
    if key not in _REF:
        ds = raw[oracle.voxel_filter(raw, VOXEL)] if len(raw) else raw
        kp, _ = oracle.keypoints(ds, R_PCA, radius_nonmax, 0.65, 20)
        lam, curv, cnt = oracle.pca(ds, R_PCA)
        cand = oracle.prune(lam, cnt, 0.65, 20)
        np.testing.assert_array_equal(ref_nms(ds, curv, cand, radius_nonmax), kp, err_msg="the two CPU references disagree: the fixture is at fault")
        for a in (ds, curv, cand, kp):
            a.setflags(write=False)
        _REF[key] = (ds, curv, cand, kp)
    return _REF[key]


def sync_depth(ds, curv, cand, radius):
    """Rounds the fixed-point rule of batch_nms.hip needs when every round sees only the decisions of the rounds before it:
    suppressed(i) <=> a neighbour of higher rank is selected, selected(i) <=> every neighbour of higher rank is suppressed."""
    from scipy.spatial import cKDTree

    order = np.argsort(-curv[cand], kind="stable")
    P = ds[cand[order]].astype(F)
    pairs = cKDTree(P.astype(np.float64)).query_pairs(float(radius) * 1.001, output_type="ndarray")
    d = P[pairs[:, 0]] - P[pairs[:, 1]]
    d2 = d[:, 0] * d[:, 0]
    d2 += d[:, 1] * d[:, 1]
    d2 += d[:, 2] * d[:, 2]
    pairs = pairs[d2 < F(np.float64(F(radius)) ** 2)]
    hi, lo = pairs.min(axis=1), pairs.max(axis=1)  # rank order = index order: hi outranks lo
    n = len(P)
    state = np.zeros(n, np.int8)
    rounds = 0
    while (state == 0).any():
        n_sel = np.bincount(lo, weights=state[hi] == 1, minlength=n)
        n_open = np.bincount(lo, weights=state[hi] != 2, minlength=n)
        new = np.where(n_sel > 0, 2, np.where(n_open == 0, 1, 0)).astype(np.int8)
        state = np.where(state == 0, new, state)
        rounds += 1
    return rounds


def _same_keypoints(ctx, api, oracle, cfg, raws, handles=None, singles=None):
    """Every cloud of the batch against the oracle and against a handle filled by recompute (the one-workgroup path)."""
    seed = _ribbon(30)
    radius = cfg.reg.radius_nonmax
    refs = [_reference(oracle, raw, radius) for raw in raws]  # before the GPU is asked
    own = []  # handles made here are closed here; a caller that passes its own keeps them
    if handles is None:
        handles = [ctx.cloud_create(cfg, seed) for _ in raws]
        own += handles
    if singles is None:
        singles = [ctx.cloud_create(cfg, seed) for _ in raws]
        own += singles
    try:
        ctx.clouds_recompute(handles, raws)
        for h, s, raw, (ds, _, cand, kp) in zip(handles, singles, raws, refs):
            s.recompute(raw)
            for c in (h, s):
                i = c.info()
                assert (i.m, i.k) == (len(ds), len(kp))
                if len(ds):
                    d = c.download()
                    np.testing.assert_array_equal(d["ds"].cpu().numpy(), ds)
                    np.testing.assert_array_equal(d["kp"].cpu().numpy(), kp)
    finally:
        for c in own:
            c.close()
    return refs


def _timed_batch(ctx, cfg, raws):
    """timed launches of the NMS rounds of ONE batch: a launch sequence of FB_NMS_ROUNDS rounds counts once, the rank pass once"""
    handles = [ctx.cloud_create(cfg, _ribbon(30)) for _ in raws]
    ctx.kernel_timing(True)
    try:
        ctx.clouds_recompute(handles, raws)
        _, launches = ctx.kernel_time("nms_round")
    finally:
        ctx.kernel_timing(False)
        for h in handles:
            h.close()
    return launches


# ---------------------------------------------------------------------------------------------------------------- B1
def test_batch_long_chains_in_both_directions(ctx, api, oracle):
    """A ribbon whose curvature rises strictly along x: every keypoint waits for its neighbour further up, one chain from the highest
    cell index to the lowest (slots are ordered by cell, x-major: the early workgroups wait for the late ones), and its mirror image.
    The descending chain must take more than one launch sequence of the rounds: the only evidence that the second sequence ran."""
    L = 1000
    cfg = _cfg(api)
    for mirror in (False, True):
        raw = _ribbon(L, grow=2.0 ** -14, mirror=mirror)
        ds, curv, cand, kp = _reference(oracle, raw)
        depth = sync_depth(ds, curv, cand, R)
        assert depth >= 4 * FB_NMS_ROUNDS, depth
        steps = np.diff(ds[kp, 0])  # the chain's direction (the keypoint at the other end of the ribbon is the one exception)
        assert ((steps > 0) if mirror else (steps < 0)).sum() >= len(kp) - 3 and len(kp) >= 32
        launches = _timed_batch(ctx, cfg, [raw])
        print("chain of depth %d, %s: %d timed launches of the rounds" % (depth, "ascending" if mirror else "descending", launches))
        if not mirror:
            assert launches > 2, launches  # at least two sequences of rounds and the rank pass
        _same_keypoints(ctx, api, oracle, cfg, [raw])
    _same_keypoints(ctx, api, oracle, cfg, [_ribbon(L, grow=2.0 ** -14), _ribbon(L // 2, grow=2.0 ** -14, mirror=True), _ribbon(L // 3, grow=2.0 ** -14)])
    # and no further sequence once the last round leaves nobody undecided: a short chain (it runs against the slot order, so its first round
    # leaves candidates waiting) settles within one sequence: one timed launch for the rounds, one for the rank pass
    short = _ribbon(20, grow=2.0 ** -14)
    ds, curv, cand, kp = _reference(oracle, short)
    assert len(kp) >= 3 and 4 <= sync_depth(ds, curv, cand, R) <= FB_NMS_ROUNDS
    assert _timed_batch(ctx, cfg, [short]) == 2


# ---------------------------------------------------------------------------------------------------------------- B2
def test_batch_plateaus(ctx, api, oracle):
    """The tie ribbon: a handful of curvature values, plateaus of hundreds of bit-identical keys that resolve by point index, so the
    decisions still form one chain: the equal-key branches of k_fb_nmsr_sort, the `below` cut of the walk and k_fb_nmsr_rank.  The ribbon
    is one cell thick in y and z: dim = 1 there, the clamps of the list heads and of the cell table apply."""
    L = 1000
    cfg = _cfg(api)
    raws = [_ribbon(L), _ribbon(L - 7, mirror=True, x0=-33.0)]
    for raw in raws:
        ds, curv, cand, kp = _reference(oracle, raw)
        _, counts = np.unique(curv[cand], return_counts=True)
        assert counts.max() > NMS_T and len(counts) <= 32, counts  # plateaus longer than a workgroup
        assert sync_depth(ds, curv, cand, R) >= 4 * FB_NMS_ROUNDS
        assert grid_desc(ds, R)["dim"][1:] == [1, 1]
    _same_keypoints(ctx, api, oracle, cfg, raws)


# ---------------------------------------------------------------------------------------------------------------- B3
@pytest.mark.parametrize("radius,shapes", [(0.3, [(341, 3, 1023), (344, 4, 1024), (683, 3, 2049)]), (0.4, [(683, 3, 1025), (1400, 3, 2099)])])
def test_batch_rank_tiles(ctx, api, oracle, radius, shapes):
    """Keypoint counts of one cloud on either side of the rank pass's LDS tile (1024) and beyond two tiles; the lengths were found with
    the oracle and are frozen here, the counts are asserted before the GPU is asked."""
    cfg = _cfg(api, radius)
    raws = [_ribbon(L, W=W) for L, W, _ in shapes]
    for raw, (_, _, K) in zip(raws, shapes):
        assert len(_reference(oracle, raw, radius)[3]) == K
    _same_keypoints(ctx, api, oracle, cfg, raws)


# ---------------------------------------------------------------------------------------------------------------- B4
def test_batch_offsets_and_buffer_reuse(ctx, api, oracle, synth):
    """empty, ribbon, one point, a scan, the mirrored ribbon, a blob with one keypoint: with the total candidate count just below and
    just above a multiple of 256 (the ribbon is padded to move it), then the same handles in another order."""
    cfg = _cfg(api)
    scan = np.ascontiguousarray(synth.tls_pair(20_000, pair_id=31).source, F)
    blob = _ribbon(5) + np.array([3.0, -2.0, 1.0], F)
    ds, _, cand, kp = _reference(oracle, blob)
    assert len(cand) > 1 and len(kp) == 1  # all candidates but one are suppressed by one
    one = _ribbon(1, W=1, T=1) + np.array([-7.5, 2.25, 0.5], F)
    assert one.shape == (1, 3) and len(_reference(oracle, one)[0]) == 1  # m = 1: a box of zero extent, dim = 1 on every axis, a one-point PCA
    def clouds(L):
        return [np.zeros((0, 3), F), _ribbon(L, grow=2.0 ** -14), one, scan, _ribbon(90, grow=2.0 ** -14, mirror=True), blob]
    def ctot(L):
        return sum(len(_reference(oracle, raw)[2]) for raw in clouds(L))
    L = 100
    while ctot(L + 1) // 256 == ctot(L) // 256:  # a column adds eight candidates
        L += 1
    assert ctot(L + 1) - ctot(L) == 8 and ctot(L) % 256 >= 248 and ctot(L + 1) % 256 < 8
    seed = _ribbon(30)
    handles, singles = [ctx.cloud_create(cfg, seed) for _ in range(6)], [ctx.cloud_create(cfg, seed) for _ in range(6)]
    try:
        _same_keypoints(ctx, api, oracle, cfg, clouds(L), handles, singles)
        _same_keypoints(ctx, api, oracle, cfg, clouds(L + 1), handles, singles)
        order = [3, 5, 1, 0, 4, 2]  # other sizes into the same handles
        _same_keypoints(ctx, api, oracle, cfg, [clouds(L)[i] for i in order], handles, singles)
    finally:
        for h in handles + singles:
            h.close()


# ---------------------------------------------------------------------------------------------------------------- B5
def test_batch_more_than_256_cells_along_x(ctx, api, oracle, synth):
    """A ribbon at x = 400 m with a scan far away in the same cloud: the NMS grid of the batch (over the box of the down-sampled cloud)
    has more than 256 cells along x and takes the widened cell."""
    cfg = _cfg(api)
    scan = np.ascontiguousarray(synth.tls_pair(20_000, pair_id=32).source, F)
    raw = np.concatenate([scan, _ribbon(120, grow=2.0 ** -14, x0=400.0)])
    ds, _, cand, kp = _reference(oracle, raw)
    g = grid_desc(ds, R)
    assert g["dim"][0] > 256 and g["widened"] and (ds[kp, 0] > 399.0).sum() >= 10 and (ds[kp, 0] < 399.0).sum() >= 10, g
    _same_keypoints(ctx, api, oracle, cfg, [raw, _ribbon(60, x0=-420.0)])
