"""A brute-force float32 restatement of the FPFH front end (gh-icp_amd/csrc/fpfh.hip: k_knn, k_spfh, k_fpfh; fd.hip: k_fd_fpfh), numpy only.

It goes through neither oracle/'s grid nor its FPFH code: the neighbours come from the full m x m distance matrix, and SPFH and the weighting
are written from SURVEY.md §8c (pcl::computePairFeatures, computePointSPFHSignature, weightPointSPFHSignature) in float32, one rounding per
operation in the kernels' order -- the library is compiled with -ffp-contract=off, so equality is bit for bit.  The single thing taken from
the oracle is the numerics contract's atan2f (`oracle.atan2f`), whose own accuracy tests/test_oracle_cpu.py checks.  Shared by
tests/test_fpfh_restatement_cpu.py (no GPU: restatement == oracle on every edge case) and tests/test_gpu_fpfh_edges.py (kernels == restatement).

Every loop over points is a numpy vector operation; the loops that remain are the 20 neighbours and the 11 bins, in the kernels' order, so
that each accumulator sees its addends in the same sequence."""
import numpy as np

F = np.float32
K = 20
NB = 11


def _f32(a):
    return np.ascontiguousarray(a, dtype=F)


def knn_brute(xyz, k=K, rows=None):
    """(nn (m, nk) int64, nd (m, nk) f32, nk): the nk = min(k, m) points nearest to each point, the point itself included, by
    (d2, index) with d2 = dx*dx; d2 += dy*dy; d2 += dz*dz in float32.  `rows`: the lists of these points only, in this order."""
    p = _f32(xyz)[:, :3]
    m = p.shape[0]
    nk = min(k, m)
    if m == 0:
        return np.zeros((0, 0), np.int64), np.zeros((0, 0), F), 0
    q = p if rows is None else p[rows]
    dx = q[:, None, 0] - p[None, :, 0]
    d2 = dx * dx
    dx = q[:, None, 1] - p[None, :, 1]
    d2 += dx * dx
    dx = q[:, None, 2] - p[None, :, 2]
    d2 += dx * dx
    assert d2.dtype == F
    order = np.argsort(d2, axis=1, kind="stable")[:, :nk]  # stable: equal distances stay in index order
    return order.astype(np.int64), np.take_along_axis(d2, order, axis=1), nk


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def spfh(xyz, normals, nn, nk, atan2f=None, stats=None, rows=None):
    """(m, 33) f32: the three 11-bin histograms of the Darboux-frame features of each point against its nk neighbours (list order).
    `rows`: nn holds the lists of these points only, and so does the result.
    `stats`, when a dict, receives how many pairs took each skip and the role switch, and how many bin indices the clamp to 0..10 changed."""
    if atan2f is None:
        from oracle import oracle as O

        atan2f = O.atan2f
    p = _f32(xyz)[:, :3]
    n = _f32(normals)
    ids = np.arange(p.shape[0]) if rows is None else np.asarray(rows, np.int64)
    m = ids.shape[0]
    H = np.zeros((m, 33), F)
    if m == 0:
        return H
    rows = np.arange(m)
    with np.errstate(divide="ignore", invalid="ignore"):
        incr = F(100.0) / F(nk - 1)  # nk = 1: infinite, and never added (the only neighbour is the point itself)
        cnt = dict(self=0, f4=0, vn=0, switch=0, pairs=0, clamp=0)
        for t in range(nk):
            j = nn[:, t]
            p1, p2 = [p[ids, d] for d in range(3)], [p[j, d] for d in range(3)]
            n1, n2 = [n[ids, d] for d in range(3)], [n[j, d] for d in range(3)]
            dp = [p2[d] - p1[d] for d in range(3)]
            f4 = np.sqrt(_dot3(dp, dp))
            angle1, angle2 = _dot3(n1, dp) / f4, _dot3(n2, dp) / f4
            sw = np.abs(angle1) < np.abs(angle2)  # the frame sits at the point whose normal is closer to the connecting line
            a1 = [np.where(sw, n2[d], n1[d]) for d in range(3)]
            a2 = [np.where(sw, n1[d], n2[d]) for d in range(3)]
            dp = [np.where(sw, -dp[d], dp[d]) for d in range(3)]
            f3 = np.where(sw, -angle2, angle1)
            vv = _cross(dp, a1)
            vn = np.sqrt(_dot3(vv, vv))
            iv = F(1.0) / vn
            vv = [vv[d] * iv for d in range(3)]
            ww = _cross(a1, vv)
            f2 = _dot3(vv, a2)
            not_self = j != ids
            ok = not_self & (f4 != 0) & (vn != 0)
            y, x = _dot3(ww, a2), _dot3(a1, a2)
            f1 = np.zeros(m, F)
            f1[ok] = atan2f(_f32(y[ok]), _f32(x[ok]))
            for a in (f1, f2, f3, f4, vn):
                assert a.dtype == F
            assert np.isfinite(f1[ok]).all() and np.isfinite(f2[ok]).all() and np.isfinite(f3[ok]).all()
            h1 = np.floor(11 * ((f1[ok].astype(np.float64) + np.pi) * (1.0 / (2.0 * np.pi))))
            h2 = np.floor(11 * ((f2[ok].astype(np.float64) + 1.0) * 0.5))
            h3 = np.floor(11 * ((f3[ok].astype(np.float64) + 1.0) * 0.5))
            r = rows[ok]
            for blk, h in enumerate((h1, h2, h3)):
                cnt["clamp"] += int(((h < 0) | (h > NB - 1)).sum())
                H[r, blk * NB + np.clip(h, 0, NB - 1).astype(np.int64)] += incr  # one addend per row and block: no repeated index
            cnt["self"] += int((~not_self).sum())
            cnt["f4"] += int((not_self & (f4 == 0)).sum())
            cnt["vn"] += int((not_self & (f4 != 0) & (vn == 0)).sum())
            cnt["switch"] += int((ok & sw).sum())
            cnt["pairs"] += int(ok.sum())
    if stats is not None:
        stats.update(cnt)
    return H


def fpfh(nn, nd, nk, S):
    """(m, 33) f32: sum over the neighbours with nd != 0 of SPFH(neighbour) / nd, each 11-bin block rescaled to 100 (k_fpfh's order:
    per neighbour the bins 0..10, the three blocks interleaved per bin; a block's sum sees the same addends as its bins)."""
    S = _f32(S)
    m = nn.shape[0]
    Fh = np.zeros((m, 33), F)
    s = np.zeros((m, 3), F)
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(nk):
            d = nd[:, t]
            ok = d != 0
            w = F(1.0) / d
            Hn = S[nn[:, t]]
            for b in range(NB):
                for blk in range(3):
                    v = Hn[:, blk * NB + b] * w
                    s[ok, blk] += v[ok]
                    Fh[ok, blk * NB + b] += v[ok]
        scale = np.where(s != 0, F(100.0) / s, s)
    assert scale.dtype == F
    return (Fh.reshape(m, 3, NB) * scale[:, :, None]).reshape(m, 33)


def fpfh_brute(xyz, normals, k=K, atan2f=None, stats=None):
    """the three steps in one: brute-force neighbours, SPFH with the given normals, the weighting"""
    nn, nd, nk = knn_brute(xyz, k)
    return fpfh(nn, nd, nk, spfh(xyz, normals, nn, nk, atan2f, stats))


def fpfh_brute_rows(xyz, normals, rows, k=K, atan2f=None):
    """rows `rows` of fpfh_brute without the m x m matrix: the lists of these points, then the SPFH of the points in those lists only"""
    rows = np.asarray(rows, np.int64)
    nn, nd, nk = knn_brute(xyz, k, rows)
    need = np.unique(nn)
    nn2, _, _ = knn_brute(xyz, k, need)
    S = np.zeros((np.asarray(xyz).shape[0], 33), F)
    S[need] = spfh(xyz, normals, nn2, nk, atan2f, rows=need)
    return fpfh(nn, nd, nk, S), nn, nd


def normals_f64(xyz, nn, nk):
    """A tolerance reference, no restatement: (normals (m, 3) f64, eigenvalues (m, 3) ascending) of the f64 scatter of each point's nk
    neighbours through numpy.linalg.eigh, the normal flipped towards the origin."""
    p = np.asarray(xyz, np.float64)[:, :3]
    m = p.shape[0]
    if m == 0:
        return np.zeros((0, 3)), np.zeros((0, 3))
    q = p[nn[:, :nk]]  # (m, nk, 3)
    d = q - q.mean(1, keepdims=True)
    lam, vec = np.linalg.eigh(np.einsum("mki,mkj->mij", d, d) / nk)
    nrm = vec[:, :, 0]
    flip = (-(p * nrm).sum(1)) < 0
    nrm[flip] = -nrm[flip]
    return nrm, lam


def normal_filter(xyz, nrm64, lam):
    """rows on which the f64 normal is well defined: the two smallest eigenvalues apart, (l1 - l0) / l2 > 1e-3, and the line of sight
    not in the tangent plane, |p . n| / |p| > 1e-3 (there the flip may go either way)"""
    p = np.asarray(xyz, np.float64)[:, :3]
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
        side = np.abs((p * nrm64).sum(1)) / np.sqrt((p * p).sum(1))
    return (gap > 1e-3) & (side > 1e-3)


def fd_fpfh_ref(hS, hT):
    """(ks, kt) f32: FPFHfeature::compute_fpfh_distance (reference include/fpfh.hpp:135-165), |Pearson r| in sequential float32: the
    means first (sum, then / 33), then up, d1, d2 over the 33 bins in order, then |up / sqrt(d1 * d2)|."""
    hS, hT = _f32(hS), _f32(hT)
    ks, kt = hS.shape[0], hT.shape[0]
    m1, m2 = np.zeros(ks, F), np.zeros(kt, F)
    for q in range(33):
        m1 += hS[:, q]
        m2 += hT[:, q]
    m1 /= F(33)
    m2 /= F(33)
    up, d1, d2 = np.zeros((ks, kt), F), np.zeros((ks, 1), F), np.zeros((1, kt), F)
    for q in range(33):
        a, b = (hS[:, q] - m1)[:, None], (hT[:, q] - m2)[None, :]
        up += a * b
        d1 += a * a
        d2 += b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.abs(up / np.sqrt(d1 * d2))
    assert out.dtype == F
    return out
