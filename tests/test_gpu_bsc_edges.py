"""k_bsc / gh_bsc_keypoint (csrc/bsc_dev.h) at its regime edges, against oracle.bsc bit for bit (strings and LCS).  The oracle scans all
7 x 7 cells per plane for every point and does not chunk, so it is independent of the packed path's chunks of 512, of the BSC_CAP = 2048
threshold to the global sweeps, of the 3 x 3 window and its ring, and of the 64-bit depth word with its carry.  Its radius search is
pinned by tests/frontend_restatement.py (the sphere sizes below are asserted with the brute force)."""
import numpy as np
import pytest

import frontend_restatement as FR

pytestmark = pytest.mark.gpu

F = np.float32
R = 1.5
R_SEARCH = np.sqrt(3.0) * np.float64(F(R))  # bfe:641, as oracle.bsc and gh_bsc_make_const take it
SIZES_SMALL = [1, 2, 3, 255, 256, 257, 511, 512, 513, 1025]
SIZES_BIG = [2047, 2048]


def _ball(rng, k, radius):
    v = rng.normal(size=(k, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * radius * rng.random((k, 1)) ** (1 / 3)


def _spheres(sizes, seed):
    """one keypoint per size, 8 m apart (more than twice the search radius): the keypoint and size - 1 points in a flattened ball around it"""
    rng = np.random.default_rng(seed)
    parts, kp, n = [], [], 0
    for s, size in enumerate(sizes):
        c = np.array([8.0 * (s % 4), 8.0 * (s // 4), 0.0])
        parts.append(np.concatenate([c[None], c + _ball(rng, size - 1, 2.0) * [1.0, 0.7, 0.4]]))
        kp.append(n)
        n += size
    return np.ascontiguousarray(np.concatenate(parts).astype(F)), np.array(kp, np.int32)


def _compare(ctx, oracle, synth, xyz, kp, dofs=(6, 0)):
    pat = synth.bsc_pattern_glibc()
    out = None
    for dof in dofs:
        fo, lo, _ = oracle.bsc(xyz, kp, R, dof, pat)
        fg, lg = ctx.bsc_encode(xyz, kp, R, dof, pat)
        fg, lg = fg.cpu().numpy(), lg.cpu().numpy()
        np.testing.assert_array_equal(lg, lo)
        np.testing.assert_array_equal(fg, fo)
        out = out or (fg, lg)
    return out


def _sizes(xyz, kp):
    return FR.radius_counts(xyz, R_SEARCH, kp).tolist()


def test_sphere_sizes_small(ctx, oracle, synth):
    xyz, kp = _spheres(SIZES_SMALL, 201)
    assert _sizes(xyz, kp) == SIZES_SMALL  # mm of each keypoint: below 3, around every chunk of 512, two and three chunks
    fg, _ = _compare(ctx, oracle, synth, xyz, kp)
    assert fg[0, 3:].any(axis=1).all()


def test_sphere_sizes_at_the_packed_limit(ctx, oracle, synth):
    """2 047 and 2 048 points (the last packed size), then the same cloud plus one point in the second sphere: 2 049, the first unpacked"""
    xyz, kp = _spheres(SIZES_BIG, 202)
    assert _sizes(xyz, kp) == SIZES_BIG
    _compare(ctx, oracle, synth, xyz, kp)
    more = np.ascontiguousarray(np.concatenate([xyz, xyz[kp[1]:kp[1] + 1] + F([0.25, 0.125, 0.0625])]))
    assert _sizes(more, kp) == [2047, 2049]
    _compare(ctx, oracle, synth, more, kp)
    assert more.shape[0] <= 5000


def _loc(xyz, origin, lcs):
    """the points in a keypoint's LCS as gh_bsc_keypoint takes them (bfe:178-180), in float"""
    d = (xyz - origin).astype(F)
    X, Y, Z = lcs[0:3], lcs[3:6], lcs[6:9]
    return np.stack([F(F(X[0] * d[:, 0] + X[1] * d[:, 1]) + X[2] * d[:, 2]), F(F(Y[0] * d[:, 0] + Y[1] * d[:, 1]) + Y[2] * d[:, 2]),
                     F(F(Z[0] * d[:, 0] + Z[1] * d[:, 1]) + Z[2] * d[:, 2])], axis=1)


def test_ring_path(ctx, oracle, synth):
    """an axis-aligned lattice of pitch u / 2 around a keypoint at the origin, 13 x 9 x 5 points: the weighted covariance is diagonal with
    distinct entries, the axes are exact unit vectors, and every second lattice plane projects exactly onto cell edges -- the points for
    which the 3 x 3 window needs its ring"""
    u = F(2) * F(R) / F(7)
    h = F(u * F(0.5))
    i = np.arange(13 * 9 * 5)
    ijk = np.stack([i % 13 - 6, i // 13 % 9 - 4, i // 117 - 2], axis=1)
    order = np.argsort(np.abs(ijk).sum(1), kind="stable")  # the keypoint (0, 0, 0) first
    xyz = np.ascontiguousarray((ijk[order].astype(F) * h).astype(F))
    kp = np.array([0], np.int32)
    assert _sizes(xyz, kp) == [585]
    _, lg = _compare(ctx, oracle, synth, xyz, kp)
    assert sorted(np.abs(lg[0, :9]).tolist()) == [0.0] * 6 + [1.0] * 3 and abs(lg[0, 0]) == 1.0 and abs(lg[0, 8]) == 1.0
    loc = _loc(xyz, xyz[0], lg[0])
    inv_u = F(1.0) / u
    near = 0
    for a, b in ((0, 1), (0, 2), (1, 2)):
        ta, tb = F(loc[:, a] + F(R)) * inv_u, F(loc[:, b] + F(R)) * inv_u
        fa, fb = ta - np.floor(ta), tb - np.floor(tb)
        near += int(((fa < F(1e-4)) | (fa > F(0.9999)) | (fb < F(1e-4)) | (fb > F(0.9999))).sum())
    assert near >= 0.05 * 3 * 585, near  # (point, plane) items that enter the ring block


def test_depth_carry_word(ctx, oracle, synth):
    """1 500 points within a few millimetres of the centre of cell (3, 3) of the y-z plane at depth ~ 2 R along the principal axis: the cell's
    64-bit depth word wraps, and its exact sum needs the carry word"""
    rng = np.random.default_rng(203)
    base = rng.normal(size=(80, 3)) * [0.6, 0.3, 0.1]
    base[0] = 0.0
    blob = np.array([1.45, 0.0, 0.0]) + rng.uniform(-0.004, 0.004, (1500, 3))
    xyz = np.ascontiguousarray(np.concatenate([base, blob]).astype(F))
    kp = np.array([0], np.int32)
    assert _sizes(xyz, kp) == [1580]
    _, lg = _compare(ctx, oracle, synth, xyz, kp)
    loc = _loc(xyz, xyz[0], lg[0])
    u = F(2) * F(R) / F(7)
    delta = F(u * F(0.5))
    den = F(F(2) * delta * delta)
    centre = F((3 + 0.5) * np.float64(u) - np.float64(F(R)))
    da, db = loc[:, 1] - centre, loc[:, 2] - centre
    dd = da * da
    dd += db * db
    r2c = F((1.5 * np.float64(u)) ** 2)
    hit = np.flatnonzero(dd < r2c)
    ew = oracle.bsc_expf(-dd[hit] / den)
    depth = (loc[hit, 0] + F(R)).astype(np.float64)
    total = sum((int(d * 2.0 ** 24) + (1 << 27)) * int(np.float64(w) * 2.0 ** 30) for d, w in zip(depth, ew))  # gh_bsc_depth_add's terms (R / 2 = 0.75 2^0)
    assert total >= 1 << 65, total.bit_length()


def test_boundary_keypoints(ctx, oracle, synth):
    """keypoints in the first and the last cell of every axis of the search grid, and a planar cloud"""
    rng = np.random.default_rng(204)
    box = np.ascontiguousarray(rng.uniform(0, 12, (3000, 3)).astype(F))
    corners = np.array([[x, y, z] for x in (0, 12) for y in (0, 12) for z in (0, 12)] + [[6, 6, 6]], np.float64)
    kp = np.array([int(np.argmin(((box - c) ** 2).sum(1))) for c in corners], np.int32)
    g = FR.grid_desc(box, F(R_SEARCH) * F(1.0001))
    for d in range(3):
        assert g.dim[d] >= 3 and (g.coord[kp, d] == 0).any() and (g.coord[kp, d] == g.dim[d] - 1).any()
    _compare(ctx, oracle, synth, box, kp)
    plane = np.ascontiguousarray(np.concatenate([rng.uniform(0, 10, (1500, 2)), np.zeros((1500, 1))], axis=1).astype(F))
    g = FR.grid_desc(plane, F(R_SEARCH) * F(1.0001))
    assert g.dim[2] == 1
    kp = np.array([int(np.argmin(((plane - c) ** 2).sum(1))) for c in ([0, 0, 0], [10, 10, 0], [5, 5, 0], [0, 10, 0])], np.int32)
    _compare(ctx, oracle, synth, plane, kp)
