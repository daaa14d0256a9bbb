"""Named clouds for FPFH (gh-icp_amd/csrc/fpfh.hip) at the edges of its kernels, shared by tests/test_fpfh_restatement_cpu.py (no GPU) and
tests/test_gpu_fpfh_edges.py (MI355X, or the host SIMT interpreter).  Every cloud is seeded, float32, (m, 3) and has at most 3 000 points;
`rows4` gives the same cloud as rows of 4 floats.  No GPU import.

What each group is for:
  small       m = 0, 1, 2, 3, 19, 20, 21: nk < 20 (rows of the neighbour lists only partly filled), incr = 100 / (nk - 1) with nk = 1
  block       m = 127 .. 257: the last partial block of the 128-thread (k_knn, k_spfh, k_fpfh) and 256-thread (k_normals) launches
  dup         exact duplicates: the d == 0 and f4 == 0 skips, neighbour lists that do not hold the query itself, all-zero rows (s == 0)
  lattice     12^3 points of pitch 0.25: exact ties at the k-th distance (the 20th neighbour is one of eight at distance sqrt(3) pitch),
              isotropic scatters (normal = an axis: neighbours along it give vn == 0), features of exactly 1 and pi: the clamps of the
              bin indices
  plane       40 x 40 lattices normal to an axis: the closed-form row (100 in bins 5, 16, 27), features exactly on the middle bin's value
  line, bar   rank-1 scatters, and nearly so: normals that only the tie rule of the eigenvalues defines
  shift       a random box 1e3, 1e4, 1e5 away from the origin: coordinates with 2^-14 .. 2^-7 of resolution, ties and duplicates by rounding
  clusters    two clusters 5 000 apart: more than 1 000 empty shells, and more than 256 cells on an axis (the widened cell of grid.h; the
              coarsening above 2^26 cells is out of reach of gh_fpfh_cell, which sizes the cell for m / 8 cells)
  tiny        extent 0.01: everything in one cell under the 0.05 floor of the cell size
  faces       coordinates exactly on the faces mn + j * cell of the k-NN grid
  natural     a voxel-filtered synthetic scan, the well-behaved control"""
import numpy as np

F = np.float32
SMALL_M = (0, 1, 2, 3, 19, 20, 21)
BLOCK_M = (127, 128, 129, 255, 256, 257)
AXES = "xyz"


def rows4(xyz):
    """the same cloud as rows of 4 floats, a value in the fourth column that would wreck any result it leaked into"""
    out = np.full((xyz.shape[0], 4), F(-1e9), F)
    out[:, :3] = xyz
    return out


def fpfh_cell(xyz):
    """gh_fpfh_cell (fpfh.hip): the cell of the k-NN grid before any coarsening, from the float32 bounding box"""
    m = xyz.shape[0]
    mn, mx = xyz.min(0), xyz.max(0)  # float32
    ext = [float(F(mx[d] - mn[d])) + 1e-3 for d in range(3)]
    vol = max(1e-9, ext[0] * ext[1] * ext[2])
    cell = F(np.cbrt(vol / float(max(m, 1)) * 8.0))
    return F(0.05) if cell < F(0.05) else cell


def grid_dims(xyz, cell=None):
    """gh_grid_desc (grid.h) for the k-NN grid: (cell in use, dims) after the widening above 256 cells per axis and the coarsening above 2^26 cells"""
    cell = fpfh_cell(xyz) if cell is None else F(cell)
    mn, mx = xyz.min(0), xyz.max(0)
    ext = F(max(F(mx[d] - mn[d]) for d in range(3)))
    dims = F(ext / cell)
    if dims > F(256.0):
        cell = F(cell * F(F(1.0) + F(F(4e-7) * dims)))
    while True:
        inv = F(F(1.0) / cell)
        dim = [max(1, int(np.floor(F(F(mx[d] - mn[d]) * inv))) + 1) for d in range(3)]
        if dim[0] * dim[1] * dim[2] <= 1 << 26:
            return F(F(1.0) / inv), dim
        cell = F(cell * F(1.5))


def _rng(tag):
    return np.random.default_rng(0xF9F4 + tag)


def _box(rng, m, lo, hi):
    return np.ascontiguousarray(rng.uniform(lo, hi, (m, 3)).astype(F))


def small(m):
    return _box(_rng(m), m, -1.0, 1.0) + F(3.0)


def block(m):
    return _box(_rng(1000 + m), m, -2.0, 2.0) + np.array([4.0, -3.0, 2.0], F)


def dup_twice():
    rng = _rng(2001)
    p = _box(rng, 600, -2.0, 2.0) + F(5.0)
    return np.ascontiguousarray(np.repeat(p, 2, axis=0)[rng.permutation(1200)])


def dup_thrice():
    rng = _rng(2002)
    p = _box(rng, 400, -2.0, 2.0) + F(5.0)
    return np.ascontiguousarray(np.repeat(p, 3, axis=0)[rng.permutation(1200)])


def dup_25():
    """one point 25 times + 200 others: the 25 have twenty neighbours at distance 0 (an all-zero row), and the five of highest index do not
    find themselves in their own list"""
    rng = _rng(2003)
    p = np.concatenate([np.tile(np.array([[4.5, 5.25, 5.0]], F), (25, 1)), _box(rng, 200, -1.5, 1.5) + F(5.0)])
    return np.ascontiguousarray(p[rng.permutation(225)])


def identical():
    return np.tile(np.array([[1.25, -2.5, 0.75]], F), (30, 1))


def lattice():
    rng = _rng(2004)
    g = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing="ij"), -1).reshape(-1, 3)
    p = (g * 0.25 + np.array([1.0, 2.0, -4.0])).astype(F)  # every coordinate a multiple of 0.25: exact
    return np.ascontiguousarray(p[rng.permutation(p.shape[0])])


def plane(axis):
    """40 x 40 points of pitch 0.25 in the plane (coordinate `axis`) = 2.0, shuffled"""
    rng = _rng(2010 + axis)
    u, v = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
    p = np.zeros((1600, 3))
    a, b = [d for d in range(3) if d != axis]
    p[:, axis] = 2.0
    p[:, a] = u.reshape(-1) * 0.25 - 4.0
    p[:, b] = v.reshape(-1) * 0.25 + 1.0
    return np.ascontiguousarray(p.astype(F)[rng.permutation(1600)])


def line(axis):
    rng = _rng(2020 + axis)
    p = np.tile(np.array([[1.5, -2.0, 2.5]], F), (500, 1))
    p[:, axis] = rng.uniform(-10.0, 10.0, 500).astype(F)
    return np.ascontiguousarray(p)


def bar(axis):
    """a 1e-3 thin bar of 1 000 points along the axis"""
    rng = _rng(2030 + axis)
    p = (np.array([1.5, -2.0, 2.5]) + rng.uniform(-5e-4, 5e-4, (1000, 3))).astype(F)
    p[:, axis] = rng.uniform(-10.0, 10.0, 1000).astype(F)
    return np.ascontiguousarray(p)


def shifted(shift):
    rng = _rng(2040 + int(np.log10(shift)))
    p = rng.uniform(-2.0, 2.0, (1500, 3)) + np.array([shift, -shift, 0.5 * shift])
    return np.ascontiguousarray(p.astype(F))


def clusters():
    rng = _rng(2050)
    a = rng.uniform(-1.0, 1.0, (1000, 3)) + np.array([2.0, 3.0, 1.0])
    b = rng.uniform(-1.0, 1.0, (1000, 3)) + np.array([5002.0, 3.0, 1.0])
    p = np.concatenate([a, b]).astype(F)
    return np.ascontiguousarray(p[rng.permutation(2000)])


def tiny():
    rng = _rng(2060)
    return np.ascontiguousarray((rng.uniform(0.0, 0.01, (800, 3)) + np.array([0.5, 0.25, -0.75])).astype(F))


FACE_DIMS = (8, 6, 4)


def faces():
    """2 000 points in a box of 8 x 6 x 4 cells of the k-NN grid, mn + j * cell in one (1 400 points), two (400) or all three (200 distinct
    lattice nodes) of their coordinates, computed in float32 as the grid computes them.  The box is small enough for the cell to sit on its
    floor of 0.05 (asserted: the cell that gh_fpfh_cell gives for the finished cloud is the one the points were placed with)."""
    rng = _rng(2070)
    cell = F(0.05)
    mn = np.array([1.5, -2.25, 0.75], F)
    D = np.array(FACE_DIMS)
    m = 2000
    p = (mn + rng.uniform(0.0, 1.0, (m, 3)) * D * float(cell)).astype(F)
    nodes = rng.permutation(int(np.prod(D + 1)))[:200]
    jn = np.stack(np.unravel_index(nodes, tuple(D + 1)), -1)
    for i in range(m):
        if i < 1400:
            ax = [rng.integers(3)]
        elif i < 1800:
            ax = rng.permutation(3)[:2]
        else:
            ax = [0, 1, 2]
        for d in ax:
            j = jn[i - 1800, d] if i >= 1800 else rng.integers(0, D[d] + 1)
            p[i, d] = F(mn[d] + F(F(j) * cell))
    p[0] = mn  # the corners of the box are in the cloud
    p[1] = np.array([F(mn[d] + F(F(D[d]) * cell)) for d in range(3)], F)
    p = np.ascontiguousarray(p[rng.permutation(m)])
    assert fpfh_cell(p) == cell, (fpfh_cell(p), cell)
    return p


def natural(synth, voxel_filter):
    """the first 3 000 points of a synthetic terrestrial scan voxel-filtered at 0.2"""
    t = synth.tls_pair(30_000, pair_id=31).target
    return np.ascontiguousarray(t[voxel_filter(t, 0.2)][:3000, :3].astype(F))


CASES = {}
for _m in SMALL_M:
    CASES["small_%d" % _m] = (lambda m=_m: small(m))
for _m in BLOCK_M:
    CASES["block_%d" % _m] = (lambda m=_m: block(m))
CASES.update(dup_twice=dup_twice, dup_thrice=dup_thrice, dup_25=dup_25, identical=identical, lattice=lattice)
for _a in range(3):
    CASES["plane_" + AXES[_a]] = (lambda a=_a: plane(a))
for _a in range(3):
    CASES["line_" + AXES[_a]] = (lambda a=_a: line(a))
    CASES["bar_" + AXES[_a]] = (lambda a=_a: bar(a))
for _s in (1e3, 1e4, 1e5):
    CASES["shift_1e%d" % int(np.log10(_s))] = (lambda s=_s: shifted(s))
CASES.update(clusters=clusters, tiny=tiny, faces=faces)
NAMES = list(CASES) + ["natural"]
PLANES = ["plane_x", "plane_y", "plane_z"]

# the f64 normal check does not apply where no normal is defined: rank <= 1 scatters (lines, bars, fewer than 4 points), and the clouds
# that consist of duplicates
NORMAL_EXEMPT = {"small_0", "small_1", "small_2", "small_3", "dup_twice", "dup_thrice", "identical"} | {"line_" + a for a in AXES} | {"bar_" + a for a in AXES}

# the share of rows that the f64 normal check of the GPU test must keep.  Two clouds hold rows without a normal by construction: the 25
# copies of one point in dup_25 (zero scatter; 200 of 225 rows are left), and the 10^3 interior points of the lattice (the 19 nearest are
# the point, its 6 face and 12 edge neighbours -- isotropic -- and the 20th is one corner neighbour: the two smallest eigenvalues are equal;
# 728 of 1728 rows are left).  There the 90 % are asked of the rows that are left.
KEEP_FLOOR = {"dup_25": 0.9 * 200 / 225, "lattice": 0.9 * 728 / 1728}


def build(name, synth=None, voxel_filter=None):
    if name == "natural":
        return natural(synth, voxel_filter)
    p = CASES[name]()
    assert p.dtype == F and p.ndim == 2 and p.shape[1] == 3 and p.shape[0] <= 3000
    return p


def plane_row():
    """the closed-form FPFH row of a plane: f1 = f2 = f3 = 0 -> the middle bin of each block"""
    r = np.zeros(33, F)
    r[[5, 16, 27]] = 100.0
    return r


# ---------------------------------------------------------------- rows for the feature distance (fd.hip: k_fd_fpfh)
FD_SHAPES = [(1, 1), (1, 65), (63, 64), (64, 63), (65, 129), (129, 65)]  # around the 64 x 64 tile


def fd_rows(k, seed, offset=0):
    """k histogram rows (k, 33) f32: a constant row, an all-zero row, the plane's one-hot row twice (identical rows: r = 1), two rows that
    differ in one bin by one ulp, then random histograms (sparse, each block scaled to 100 as FPFH rows are); `offset` rotates the list, so
    that a single row is not always the constant one.  A constant and a zero row have no variance: their distances are 0 / 0."""
    rng = np.random.default_rng(0xFD00 + seed)
    rnd = rng.random((k + 8, 3, 11)) * (rng.random((k + 8, 3, 11)) < 0.6)
    rnd[:, :, 0] += 1e-3
    rnd = (rnd * (100.0 / rnd.sum(2, keepdims=True))).reshape(-1, 33).astype(F)
    ulp = rnd[0].copy()
    ulp[7] = np.nextafter(ulp[7], F(np.inf))
    special = np.stack([np.full(33, 3.0303030303, F), np.zeros(33, F), plane_row(), plane_row(), rnd[0], ulp])
    pool = np.concatenate([special, rnd[1:]])
    return np.ascontiguousarray(pool[(offset + np.arange(k)) % pool.shape[0]])


def fd_case(ks, kt):
    return fd_rows(ks, 100 * ks + kt, 0), fd_rows(kt, 100 * kt + ks + 7, 2)
