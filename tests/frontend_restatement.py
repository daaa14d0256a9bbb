"""TEST INFRASTRUCTURE: a grid-free restatement of the keypoint front end's radius search and PCA (pca.h:133-165, 202-250) in plain numpy.
No spatial index, nothing imported from the library or the oracle: every pair of points is tested.

radius_counts / neighbour_pairs : the exact neighbour sets of pcl's radiusSearch under the numerics contract -- float L2 in the order
                                  d = dx*dx; d += dy*dy; d += dz*dz, strict d < r2 with r2 = float32(float64(radius)**2), query included.
                                  numpy's float32 operations round once each and never contract, so this IS the set, not an approximation.
pca_reference                   : centroid and de-meaned scatter of that set in np.longdouble, eigenvalues by numpy.linalg.eigvalsh (f64).
grid_regimes                    : gh_grid_desc (csrc/grid.h) and the lane layout of gh_pca_cell_body (csrc/pca_dev.h) transcribed, ONLY so
                                  that a test can assert that its cloud reaches the regime it is named after.  Never an expected value.
"""
import types

import numpy as np

F = np.float32


def r2_of(radius):
    return F(np.float64(radius) ** 2)  # pcl radiusSearch: static_cast<float>(radius * radius)


def _hits(xq, x, r2):
    """(len(xq), len(x)) bool: x[j] within the radius of xq[i]"""
    dx = xq[:, None, 0] - x[None, :, 0]
    d = dx * dx
    dy = xq[:, None, 1] - x[None, :, 1]
    d += dy * dy
    dz = xq[:, None, 2] - x[None, :, 2]
    d += dz * dz
    assert d.dtype == np.float32
    return d < r2


def neighbour_pairs(xyz, radius, queries=None, block=512):
    """(qi, j): every pair with x[j] inside the radius of query qi (rows of `queries`, default all points), sorted by (qi, j)."""
    x = np.ascontiguousarray(xyz, F)[:, :3]
    q = np.arange(x.shape[0]) if queries is None else np.asarray(queries)
    r2 = r2_of(radius)
    I, J = [], []
    for b in range(0, q.size, block):
        i, j = np.nonzero(_hits(x[q[b:b + block]], x, r2))
        I.append(i + b)
        J.append(j)
    if not I:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(I), np.concatenate(J)


def radius_counts(xyz, radius, queries=None):
    x = np.ascontiguousarray(xyz, F)
    nq = x.shape[0] if queries is None else len(queries)
    i, _ = neighbour_pairs(x, radius, queries)
    return np.bincount(i, minlength=nq).astype(np.int32)


def curvature_of(lam):
    """pca.h:240-247 from (f32-valued) eigenvalues taken as doubles"""
    l = np.asarray(lam).astype(np.float64)
    s = (l[:, 0] + l[:, 1]) + l[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(s == 0.0, 0.0, l[:, 2] / np.where(s == 0.0, 1.0, s))


def pca_reference(xyz, radius):
    """(lambda (n, 3) f64 descending, curvature (n,) f64, count (n,) i32); points with fewer than 3 neighbours give zeros (pca.h:209).
    The sums run in np.longdouble over coordinates taken relative to the query point (the difference of two floats is exact in it, and
    the de-meaned scatter does not depend on the origin)."""
    x = np.ascontiguousarray(xyz, F)[:, :3]
    n = x.shape[0]
    i, j = neighbour_pairs(x, radius)
    cnt = np.bincount(i, minlength=n)
    lam = np.zeros((n, 3))
    if i.size:
        xl = x.astype(np.longdouble)
        d = xl[j] - xl[i]
        first = np.concatenate([[0], np.cumsum(cnt)[:-1]])  # every point is its own neighbour: no empty segment
        mean = np.add.reduceat(d, first, axis=0) / cnt[:, None].astype(np.longdouble)
        e = d - mean[i]
        S = np.zeros((n, 3, 3))
        for a in range(3):
            for b in range(a, 3):
                S[:, a, b] = S[:, b, a] = np.add.reduceat(e[:, a] * e[:, b], first).astype(np.float64)
        lam = np.linalg.eigvalsh(S)[:, ::-1].copy()
        lam[cnt < 3] = 0.0
    curv = curvature_of(lam)
    return lam, curv, cnt.astype(np.int32)


# ---------------------------------------------------------------- regimes (assertions about the INPUT only)
def grid_desc(xyz, cell, widen=True):
    """gh_grid_desc in float32, step by step.  widen=False leaves the `dims > 256` margin out (what the table would be without it)."""
    x = np.ascontiguousarray(xyz, F)[:, :3]
    mn, mx = x.min(axis=0), x.max(axis=0)
    cell = F(cell)
    ext = F((mx - mn).max())
    dims = F(ext / cell)
    widened = bool(dims > F(256.0))
    if widened and widen:
        cell = F(cell * F(F(1.0) + F(F(4e-7) * dims)))
    steps = 0
    while True:
        inv = F(F(1.0) / cell)
        dim = np.maximum(np.floor((mx - mn) * inv).astype(np.int64) + 1, 1)
        if int(dim[0]) * int(dim[1]) * int(dim[2]) <= (1 << 26):
            break
        cell = F(cell * F(1.5))
        steps += 1
    coord = np.clip(np.floor((x - mn) * inv).astype(np.int64), 0, dim - 1)  # gh_cell_coord
    return types.SimpleNamespace(cell=cell, inv=inv, mn=mn, dim=dim, ncell=int(dim.prod()), widened=widened, coarsened=steps, coord=coord)


def lane_split(np_):
    """g of gh_pca_cell_body: the largest power of two with np * g <= 64, per pass of at most 64 query points"""
    g = 1
    while g * 2 * np_ <= 64:
        g *= 2
    return g


def grid_regimes(xyz, radius, widen=True):
    """The PCA cell table of a cloud: per occupied cell (ascending key, z fastest) its coordinates, its query count np and the number of
    candidates in its 27-cell block; plus what gh_pca_cell_body derives from them for the cell's LAST pass of query points."""
    g = grid_desc(xyz, F(radius) * F(1.0001), widen)
    c = g.coord
    key = (c[:, 0] * g.dim[1] + c[:, 1]) * g.dim[2] + c[:, 2]
    keys, npq = np.unique(key, return_counts=True)
    cz, cy, cx = keys % g.dim[2], (keys // g.dim[2]) % g.dim[1], keys // (g.dim[2] * g.dim[1])
    total = np.zeros(keys.size, np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                x, y, z = cx + dx, cy + dy, cz + dz
                ok = (x >= 0) & (x < g.dim[0]) & (y >= 0) & (y < g.dim[1]) & (z >= 0) & (z < g.dim[2])
                k = (x * g.dim[1] + y) * g.dim[2] + z
                pos = np.searchsorted(keys, k)
                pos[pos >= keys.size] = 0
                ok &= keys[pos] == k
                total += np.where(ok, npq[pos], 0)
    g.keys, g.np, g.total, g.cx, g.cy, g.cz, g.key_of_point = keys, npq, total, cx, cy, cz, key
    first = np.minimum(npq, 64)
    last = np.where(npq % 64 == 0, 64, npq % 64)
    g.g_first = np.array([lane_split(int(v)) for v in first], np.int64)
    g.g_last = np.array([lane_split(int(v)) for v in last], np.int64)
    g.per_lane = -(-total // g.g_first)  # candidates the lanes of the first pass test at most
    g.resident = total + 64 <= 512       # PCA_PAD, PCA_CHUNK
    return g
