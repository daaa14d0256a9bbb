"""Cases and an independent reference for the iteration loop (loop.hip, loop_dev.h, pair_loop.hip) at its tile edges, on exact ties and on
degenerate matches: shared by tests/test_loop_edges_cpu.py (no GPU: the cases hit the regimes they name, the oracle agrees with the
restatement below) and tests/test_gpu_loop_edges.py (MI355X, or the host SIMT interpreter).  No GPU import, nothing from oracle/.

The reference is a plain numpy f64 restatement of ONE iteration's matching, written from ghicp_reg.cpp: calED (114-139), calCD_NF /
calCD_BSC (216-293), findcorrespondenceNN / NNR (605-769: start (9e20, 0), strict '<', ascending index -- the FIRST index wins a tie)
and an f64 Umeyama through numpy.linalg.svd with the diag(1, 1, det) correction.  `tie="last"` is the wrong rule ("<="): the CPU
test shows for every tie case that it moves the iteration's 4x4 by more than 1e-3, i.e. that a kernel taking the wrong partner cannot hide
inside the comparison tolerance (1e-6).

Ties.  Target keypoints are points of the integer lattice, source keypoints sit at the centre of 2, 4 or 8 of them (offsets (+-8, 0, 0),
(+-8, +-8, 0), (+-8, +-8, +-8)): every coordinate is a small integer, so the tied squared distances are the same integer and their square
roots and products with the scale the same bits.  Every tie group lives at a site of its own, >= 64 apart from every other site, so no row
has an unplanned tie for its minimum.  Under FEATURE_BSC the first iteration's weights are wfd = exp(0) = 1, wed = 0 (ghicp_reg.cpp:247):
CD is the u16 feature distance alone there, a full CD tie is a tie of the feature distances (tied targets carry the same string), and the
"break" variant gives the geometric tie different feature distances with the LAST partner the closest.

Which partner carries the lowest index: every boundary is straddled by two groups, once with the partner at -8 in the lower column and once
with the partner at +8 there (`flip`), so that a rule that prefers a place in space instead of an index is caught as well."""
import numpy as np

ROWS = 256  # loop_dev.h: rows of a sweep block
CHUNK_MIN, CHUNK_MAX = 32, 512  # loop.hip:pick_chunks, loop_dev.h
SCAN = 1024  # the widest block of the compaction rounds (dev_solve, dev_km_scan_desc)
NONE, BSC = "none", "bsc"
NN, NNR, KM = 0, 1, 2


def cdiv(a, b):
    return -(-a // b)


def chunks(ka, kb, batch):
    """loop.hip:pick_chunks -- (chunk, nchunk) of a sweep with ka rows over kb columns in a batch of `batch` pairs.  ghicp_register_clouds
    hands all its pairs to run_loops as ONE batch (cloud.hip: no split before layout_batch), NN / NNR batches get chunk_batch = nb; a
    ghicp_register call is a batch of one."""
    rowblocks = cdiv(ka if ka > 0 else 1, ROWS) * (batch if batch > 0 else 1)
    want = cdiv(2048, rowblocks)
    ch = cdiv(kb if kb > 0 else 1, want)
    ch = min(max(ch, CHUNK_MIN), CHUNK_MAX)
    return ch, (cdiv(kb, ch) if kb > 0 else 1)


def regimes(ks, kt, batch):
    """what the code's tiles make of a pair: row sweep (chunk_b over the targets), column sweep of NNR (chunk_a over the sources), row blocks"""
    cb, nb = chunks(ks, kt, batch)
    ca, na = chunks(kt, ks, batch)
    return dict(chunk_b=cb, nchunk_b=nb, chunk_a=ca, nchunk_a=na, rowblocks=cdiv(max(ks, 1), ROWS), colblocks=cdiv(max(kt, 1), ROWS),
                scan_rounds=cdiv(max(ks, kt, 1), SCAN))


# ------------------------------------------------------------------------------------------------ the independent reference
def scale_of(bbx):
    """ghicp_reg.h:40: 0.005 * bbx_magnitude (a float) stored to a float"""
    return float(np.float32(0.005 * float(np.float32(bbx))))


def hamming(fS, fT):
    """feature distance of BSC strings (ghicp_reg.cpp:143-186): Hamming distance, the minimum over the source's variants.  fS (V, ks, 56),
    fT (kt, 56) u8 -> (ks, kt) f64"""
    bS = np.unpackbits(np.asarray(fS, np.uint8), axis=-1).astype(np.int16)
    bT = np.unpackbits(np.asarray(fT, np.uint8), axis=-1).astype(np.int16)
    out = None
    for v in range(bS.shape[0]):
        d = bS[v].sum(-1)[:, None] + bT.sum(-1)[None, :] - 2 * (bS[v] @ bT.T)
        out = d if out is None else np.minimum(out, d)
    return out.astype(np.float64)


def cd_matrix(kpS, kpT, FD, feature, bbx, it=0, weight_changing_rate=6):
    d = np.asarray(kpS, np.float64)[:, None, :] - np.asarray(kpT, np.float64)[None, :, :]
    ed = scale_of(bbx) * np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2 + d[..., 2] ** 2)
    if feature == NONE:
        return ed
    wfd = float(np.exp(-1.0 * it / weight_changing_rate))
    wed = 1.0 - wfd
    return wed * ed + wfd * np.asarray(FD, np.float64)


def _argmin(M, tie):
    """row arg-min of ghicp_reg.cpp:715-724: (9e20, 0), strict '<' ("first"); "last": '<=' -- the wrong rule.  A row without an entry below
    9e20 (NaN) keeps index 0."""
    n, m = M.shape
    idx = np.zeros(n, np.int64)
    best = np.full(n, 9e20)
    for i in range(n):
        row = M[i]
        ok = row < 9e20
        if not ok.any():
            continue
        v = row[ok].min()
        hit = np.flatnonzero(ok & (row == v))
        idx[i] = hit[0] if tie == "first" else hit[-1]
        best[i] = v
    return idx, best


def match_once(kpS, kpT, FD, feature, corr, bbx, it=0, penalty_initial=2.0, tie="first", override=None):
    """One iteration's matching (it <= 1: the penalty comes from this iteration's CD).  override: {row: column} forces single rows of the
    row arg-min (the per-row detectability check).  Returns CD, SV, TV, cdmean, cdstd, penalty, SP, TP, cor, matchrow."""
    assert it <= 1 and corr in (NN, NNR)
    CD = cd_matrix(kpS, kpT, FD, feature, bbx, it)
    ks, kt = CD.shape
    cdmean = CD.sum() / kt / ks
    cdstd = float(np.sqrt(((CD - cdmean) ** 2).sum() / kt / ks))
    if feature == NONE:
        penalty, cdstd = max(cdmean, 1.0), 0.0  # ghicp_reg.cpp:239 overrides 230-237
    else:
        penalty = max(cdmean - penalty_initial * cdstd, 5.0)
    SV, best = _argmin(CD, tie)
    for r, c in (override or {}).items():
        SV[r] = c
    TV = None
    if corr == NN:
        keep = best < penalty
    else:
        TV, _ = _argmin(CD.T, tie)
        keep = TV[SV] == np.arange(ks)
    SP = np.flatnonzero(keep)
    TP = SV[SP]
    row = np.full(ks, -1, np.int32)
    row[SP] = TP
    return dict(CD=CD, SV=SV, TV=TV, cdmean=float(cdmean), cdstd=cdstd, penalty=float(penalty), SP=SP, TP=TP, cor=int(SP.size), matchrow=row)


def umeyama(src, tgt):
    """f64 least-squares rigid transform src -> tgt (Umeyama 1991 without scale): SVD of the cross-covariance, diag(1, 1, det(U V^T))."""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    ms, mt = src.mean(0), tgt.mean(0)
    H = (tgt - mt).T @ (src - ms) / src.shape[0]
    U, s, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U @ Vt) >= 0 else -1.0])
    R = U @ D @ Vt
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = mt - R @ ms
    return M, s, float(np.linalg.det(H))


def first_Rt(case, corr, tie="first", override=None):
    m = match_once(case["kpS"], case["kpT"], case.get("FD"), case["feature"], corr, case["bbx"], tie=tie, override=override)
    return umeyama(case["kpS"][m["SP"]], case["kpT"][m["TP"]])[0], m


# ------------------------------------------------------------------------------------------------ tie cases
_OFFS = {2: [(-8, 0, 0), (8, 0, 0)],
         4: [(-8, -8, 0), (8, 8, 0), (-8, 8, 0), (8, -8, 0)],
         8: [(-8, -8, -8), (8, 8, 8), (-8, 8, 8), (8, -8, -8), (8, -8, 8), (-8, 8, -8), (8, 8, -8), (-8, -8, 8)]}
_PLAIN = [(0, 0, 4), (3, 0, 0), (0, -5, 0), (2, 2, 1), (-1, 4, 2), (0, 3, -4)]


def _flip_bits(rng, s, k, avoid=()):
    """a copy of the 56-byte string s with k of its first 441 bits flipped (none of `avoid`); returns (string, flipped bit numbers)"""
    free = np.setdiff1d(np.arange(441), np.asarray(avoid, np.int64))
    bits = rng.choice(free, size=k, replace=False)
    out = s.copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(0x80 >> (b & 7))
    return out, bits


def tie_case(name, ks, kt, row_ties, col_ties, feature, seed, fd_mode="tie", bbx=123.0):
    """row_ties: [(row, cols, flip)] -- source `row` at the centre of len(cols) in (2, 4, 8) targets that stand in columns `cols` (ascending);
    flip: the order in which the partners' places in space go to the columns is reversed.  col_ties: [(col, (row_lo, row_hi), flip)] -- target
    `col` half-way between two sources.  Every other source row gets a site and a partner column of its own, every other target column a
    site without a source.  fd_mode (BSC): "tie" -- tied partners carry the same string (a full CD tie at iteration 0); "break" -- the
    geometric tie is broken by the feature distance alone, the partner in the HIGHEST column is the closest."""
    rng = np.random.default_rng(seed)
    used_rows, used_cols = set(), set()
    for r, cols, _ in row_ties:
        assert r not in used_rows and not used_cols & set(cols) and list(cols) == sorted(cols) and len(cols) in _OFFS
        used_rows.add(r)
        used_cols |= set(cols)
    for c, rows, _ in col_ties:
        assert c not in used_cols and not used_rows & set(rows) and rows[0] < rows[1]
        used_cols.add(c)
        used_rows |= set(rows)
    assert max(used_rows, default=0) < ks and max(used_cols, default=0) < kt
    plain_rows = [r for r in range(ks) if r not in used_rows]
    free_cols = [c for c in range(kt) if c not in used_cols]
    assert len(plain_rows) <= len(free_cols), "every source row needs a partner column of its own"
    partner = dict(zip(plain_rows, free_cols))  # ascending rows to ascending columns
    filler = free_cols[len(plain_rows):]
    n_sites = len(row_ties) + len(col_ties) + len(plain_rows) + len(filler)
    side = int(np.ceil((2.5 * n_sites) ** (1 / 3))) + 1
    cells = rng.choice(side ** 3, size=n_sites, replace=False)
    sites = iter(64 * np.stack([cells // (side * side), (cells // side) % side, cells % side], axis=1).astype(np.int64))
    kpS, kpT = np.zeros((ks, 3), np.int64), np.zeros((kt, 3), np.int64)
    fT = rng.integers(0, 256, size=(kt, 56), dtype=np.uint8)
    fT[:, 55] &= 0x80  # bits 441 .. 447 stay clear
    fS = np.zeros((ks, 56), np.uint8)
    for r, cols, flip in row_ties:
        C = next(sites)
        offs = _OFFS[len(cols)][::-1] if flip else _OFFS[len(cols)]
        kpS[r] = C
        for c, o in zip(cols, offs):
            kpT[c] = C + o
            fT[c] = fT[cols[0]]
        fS[r], flipped = _flip_bits(rng, fT[cols[0]], 8 + int(rng.integers(0, 8)))
        if fd_mode == "break":  # every partner but the last moves 12 more bits away from the source's string
            for c in cols[:-1]:
                fT[c], _ = _flip_bits(rng, fT[c], 12, avoid=flipped)
    for c, rows, flip in col_ties:
        C = next(sites)
        kpT[c] = C
        sgn = -1 if flip else 1
        kpS[rows[0]] = C + np.array([-8 * sgn, 0, 0])
        kpS[rows[1]] = C + np.array([8 * sgn, 0, 0])
        k = 8 + int(rng.integers(0, 8))
        fS[rows[0]], f0 = _flip_bits(rng, fT[c], k)
        fS[rows[1]], _ = _flip_bits(rng, fT[c], k if fd_mode == "tie" else k - 5, avoid=f0)  # "break": the HIGHER row is the closer one
    for i, r in enumerate(plain_rows):
        C = next(sites)
        kpS[r] = C
        kpT[partner[r]] = C + np.array(_PLAIN[i % len(_PLAIN)])
        fS[r], _ = _flip_bits(rng, fT[partner[r]], 6 + int(rng.integers(0, 20)))
    for c in filler:
        kpT[c] = next(sites) + np.array([0, 0, 16])
    case = dict(name=name, kpS=kpS.astype(np.float64), kpT=kpT.astype(np.float64), feature=feature, bbx=float(bbx), row_ties=list(row_ties),
                col_ties=list(col_ties), fd_mode=fd_mode, ks=ks, kt=kt)
    if feature == BSC:
        case["fS"] = np.repeat(fS[None], 4, axis=0).copy()  # the four variants of a 6-DoF source carry the same string
        case["fT"] = fT
        case["FD"] = hamming(case["fS"], fT)
    return case


def straddle(bounds_b, bounds_a, ks, kt, rows_at=(), inside=(2, 4, 8)):
    """Tie groups for the chunk boundaries `bounds_b` of the row sweep (a column boundary B is straddled by the columns B-1 | B) and
    `bounds_a` of NNR's column sweep (rows B-1 | B), two groups per boundary, plus groups inside the first chunk (`inside`: how many partners
    each has); the first tie rows are `rows_at` (the row-block boundary).  The second group of a boundary cannot use the same two columns: it
    takes the columns next to them, B-2 | B+1 -- still one partner on each side of the boundary -- with the partners' places in space
    exchanged (flip).  Returns (row_ties, col_ties)."""
    col_groups, c0 = [], 2  # (columns, flip); the inside groups start at column 2 (the smallest chunk has 32 columns)
    for k, n in enumerate(inside):
        assert c0 + n <= min(kt, CHUNK_MIN) and not any(c0 < b < c0 + n for b in bounds_b)
        col_groups.append((tuple(range(c0, c0 + n)), k % 2))
        c0 += n
    for B in bounds_b:
        assert c0 + 2 <= B - 2 and B + 1 < kt + 1 and 0 < B < kt
        col_groups.append(((B - 1, B), 0))
        if B + 1 < kt:
            col_groups.append(((B - 2, B + 1), 1))
    row_groups = []
    for B in bounds_a:
        assert 2 <= B and B < ks
        row_groups.append(((B - 1, B), 0))
        if B + 1 < ks:
            row_groups.append(((B - 2, B + 1), 1))
    rows_used = {r for rows, _ in row_groups for r in rows}
    cols_used = {c for cols, _ in col_groups for c in cols}
    assert len(rows_used) == 2 * len(row_groups) and len(cols_used) == sum(len(c) for c, _ in col_groups), "boundaries too close to each other"
    free_rows = [r for r in rows_at if r not in rows_used] + [r for r in range(ks) if r not in rows_used and r not in rows_at]
    free_cols = [c for c in range(kt) if c not in cols_used][::-1]  # the column ties' targets: from the far end, the last chunk
    row_ties = [(free_rows[i], cols, f) for i, (cols, f) in enumerate(col_groups)]
    col_ties = [(free_cols[i], rows, f) for i, (rows, f) in enumerate(row_groups)]
    return row_ties, col_ties


def single_call_tie_cases():
    """ghicp_register (a batch of one: chunk = 32 on both sweeps).  ks = 300, kt = 600: two row blocks, three column blocks, 19 column
    chunks; ties inside chunk 0, across 31 | 32, across 511 | 512 (a boundary of the 32-chunks as well as of CHUNK_MAX), tie rows 253 and 258
    (both row blocks; 254 .. 257 belong to the column ties); for NNR a target between the source rows 255 | 256 (row block and chunk_a boundary at once) and 31 | 32."""
    ks, kt = 300, 600
    rt, ct = straddle([32, 512], [32, 256], ks, kt, rows_at=(253, 258))
    out = []
    for feature in (NONE, BSC):
        out.append(tie_case("single-%s-tie" % feature, ks, kt, rt, ct, feature, seed=11))
    out.append(tie_case("single-bsc-break", ks, kt, rt, ct, BSC, seed=12, fd_mode="break"))
    return out


BATCHES = {
    # name: (pairs in the batch, [(ks, kt, column boundaries, row boundaries of NNR, rows_at)]): the shapes of its tie pairs; the batch is
    # filled up to its size by repeating them (the same handles serve many pairs).
    # chunk 32: four pairs -- 8 row blocks, chunk = max(32, ceil(600 / 256))
    "chunk32": (4, [(300, 600, [32, 512], [32, 256], (253, 258))]),
    # intermediate: 256 pairs.  (12, 300): chunk_b = ceil(300 / 8) = 38, boundaries 38, 76, ...; (200, 300): chunk_b = 38 and chunk_a = ceil(200 / 4) = 50
    "intermediate": (256, [(12, 300, [38, 76], [], ()), (200, 300, [38, 266], [50, 150], ())]),
    # CHUNK_MAX: 2048 pairs.  (4, 513): chunk_b = 512 and a last chunk of the single column 512; (513, 540): chunk_a = 512 as well, rows 511 | 512
    "chunkmax": (2048, [(4, 513, [512], [], ()), (513, 540, [512], [512, 256], (253, 258))]),
}
BATCH_EXPECT = {"chunk32": [dict(chunk_b=32, chunk_a=32)],
                "intermediate": [dict(chunk_b=38, nchunk_b=8, chunk_a=32, nchunk_a=1), dict(chunk_b=38, nchunk_b=8, chunk_a=50, nchunk_a=4)],
                "chunkmax": [dict(chunk_b=512, nchunk_b=2, chunk_a=32, nchunk_a=1), dict(chunk_b=512, nchunk_b=2, chunk_a=512, nchunk_a=2)]}


def batch_tie_cases(batch, feature):
    """the distinct tie pairs of a batch regime, [case]; case["batch"] = the number of pairs of the whole batch"""
    n, shapes = BATCHES[batch]
    out = []
    for k, (ks, kt, bb, ba, rows_at) in enumerate(shapes):
        rt, ct = straddle(bb, ba, ks, kt, rows_at=rows_at, inside=(2, 4, 8) if ks > 8 else (2,))
        for mode in (("tie",) if feature == NONE else ("tie", "break")):
            c = tie_case("%s-%s-%dx%d-%s" % (batch, feature, ks, kt, mode), ks, kt, rt, ct, feature, seed=100 + 7 * k + len(out), fd_mode=mode)
            c["batch"] = n
            out.append(c)
    return out


def tied_columns(case):
    """[(row, cols)] of the row ties whose CD values must be bit-equal, [(col, rows)] of the column ties"""
    rows = [(r, cols) for r, cols, _ in case["row_ties"]] if not (case["feature"] == BSC and case["fd_mode"] == "break") else []
    cols = [(c, rows_) for c, rows_, _ in case["col_ties"]] if not (case["feature"] == BSC and case["fd_mode"] == "break") else []
    return rows, cols


# ------------------------------------------------------------------------------------------------ shape cases
SHAPES = [(1, 1), (1, 40), (40, 1), (3, 5), (255, 257), (256, 256), (257, 255), (300, 513), (513, 300), (1025, 31), (31, 1025)]
KM_SHAPES = [s for s in SHAPES if max(s) <= 513]
KM_MAX_ITER = 8


def shape_pair(synth, bbx_of):
    """the rotated-and-jittered set of tests/test_gpu_loop_fused.py's `pair` fixture (keypoint i <-> keypoint i, 12 degrees and 1.7 m apart),
    with enough keypoints for the 1025 shapes"""
    p = synth.gauss_pair(n_kp=1100)
    S = p.source[p.kp_source].astype(np.float64)
    a = np.deg2rad(12.0)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    T = S @ R.T + np.array([1.5, -0.8, 0.3]) + 0.02 * np.random.default_rng(1).standard_normal(S.shape)
    return S, T, float(bbx_of(p.source))


def fake_bsc_fd(rng, ks, kt):
    """u16 feature distances as tests/test_gpu_loop_fused.py makes them: 60 .. 200, half of the true partners 5 .. 40, 1 % false friends"""
    FD = rng.integers(60, 200, size=(ks, kt)).astype(np.float64)
    low = rng.random((ks, kt)) < 0.01
    FD[low] = rng.integers(5, 45, size=int(low.sum()))
    idx = np.arange(min(ks, kt))
    idx = idx[rng.random(idx.size) < 0.5]
    FD[idx, idx] = rng.integers(5, 40, size=idx.size)
    return FD


# ------------------------------------------------------------------------------------------------ degenerate matches (FEATURE_NONE, NN)
def _rotz(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])


def _accept_n(n_acc, n_rej=12, kt=14, seed=3):
    """n_acc source rows 0.05 .. 0.2 from a target of a 10 m cluster, n_rej rows 300 m away from every target: CDmean lies between, the
    first are accepted (best < penalty), the others are not"""
    rng = np.random.default_rng(seed)
    T = rng.uniform(-5, 5, size=(kt, 3))
    S = np.concatenate([T[:n_acc] + rng.uniform(0.03, 0.1, size=(n_acc, 3)), np.array([300.0, 40.0, -20.0]) + rng.uniform(-3, 3, size=(n_rej, 3))])
    order = rng.permutation(S.shape[0])
    return S[order], T


def degenerate_cases():
    """name -> dict(kpS, kpT, bbx, expect): expect holds what the CPU test proves about the case through the restatement"""
    rng = np.random.default_rng(20261020)
    out = {}
    xy = rng.uniform(-20, 20, size=(60, 2))
    S = np.column_stack([xy, np.full(60, 2.5)])
    out["coplanar"] = dict(kpS=S, kpT=S @ _rotz(3.0).T + np.array([0.4, -0.2, 0.0]), bbx=60.0, expect=dict(rank=2))
    u = rng.uniform(-30, 30, size=40)
    S = np.outer(u, [2.0, 1.0, 0.5]) + np.array([1.0, 2.0, 3.0])
    out["collinear"] = dict(kpS=S, kpT=S + np.array([0.25, 0.5, -0.125]), bbx=60.0, expect=dict(rank=1))
    T = np.array([[9, 0, 0], [40, 3, 1], [0, 50, 2], [-30, -30, 7], [12, 44, -9], [-9, 0, 0], [60, -8, 5]], float) + np.array([5.0, -3.0, 2.0])
    out["identical-sources"] = dict(kpS=np.tile(np.array([5.0, -3.0, 2.0]), (20, 1)), kpT=T, bbx=200.0, expect=dict(rank=0, all_take=0, tied=(0, 5)))
    xy = 4.0 * np.stack(np.meshgrid(np.arange(7.0), np.arange(6.0)), -1).reshape(-1, 2) + rng.uniform(-0.5, 0.5, size=(42, 2))
    S = np.column_stack([xy, rng.uniform(-0.3, 0.3, size=42)])
    out["mirrored"] = dict(kpS=S, kpT=S * np.array([1.0, 1.0, -1.0]), bbx=60.0, expect=dict(rank=3, det_negative=True, identity_match=True))
    for n in (9, 10, 1):
        S, T = _accept_n(n)
        out["cor-%d" % n] = dict(kpS=S, kpT=T, bbx=200.0, expect=dict(cor=n))
    # no correspondence: three sources at the centre of six targets 9 m away, scale = 1: every CD is 9, CDmean is 9 exactly (sums of small
    # integers), and 9 < 9 is false for every row
    T = np.array([[9, 0, 0], [-9, 0, 0], [0, 9, 0], [0, -9, 0], [0, 0, 9], [0, 0, -9]], float) + np.array([2.0, 1.0, -4.0])
    out["cor-0"] = dict(kpS=np.tile(np.array([2.0, 1.0, -4.0]), (3, 1)), kpT=T, bbx=200.0, expect=dict(cor=0))
    return out


def fpfh_nan_case(fd_fpfh):
    """FPFH similarity matrix with the NaN row a constant source histogram gets (fd_fpfh: the caller's implementation of calFD_FPFH)"""
    rng = np.random.default_rng(11)
    ks, kt, row = 70, 90, 13
    hS = (rng.random((ks, 33)) * 100).astype(np.float32)
    hT = (rng.random((kt, 33)) * 100).astype(np.float32)
    hS[row] = 7.0
    nanrow = np.asarray(fd_fpfh(hS, hT), np.float64)[row]
    FD = (0.2 + 0.6 * rng.random((ks, kt))).astype(np.float32)
    FD[np.arange(ks), np.arange(ks)] = 0.97
    FD[row] = nanrow.astype(np.float32)
    return dict(ks=ks, kt=kt, row=row, FD=FD)


# ------------------------------------------------------------------------------------------------ the rigid solve
# Tolerances of check 3 (tests/test_loop_edges_cpu.py's docstring has the measurement): 4 x the largest value oracle.rigid_svd shows against the
# f64 SVD over rigid_cases(), relative to max |p| where the quantity is a length.
RIGID_SEEN = dict(angle=5.8e-6, dt=4.6e-6, rmse=3.3e-8)  # the largest values measured (rounded up in the second digit)
RIGID_ANGLE_TOL = 4 * RIGID_SEEN["angle"]  # rad, cases with a unique rotation
RIGID_DT_TOL = 4 * RIGID_SEEN["dt"]        # |dt| / max|p|, the same cases
RIGID_RMSE_TOL = 4 * RIGID_SEEN["rmse"]    # (RMSE under the returned 4x4 - RMSE of the f64 optimum) / max|p|, all cases
# check 2: every entry of R is an f32 rounding of an entry of an f64-orthonormal matrix, |E_ij| <= 2^-25.  R^T R - I = E^T R + R^T E + E^T E:
# an entry is bounded by 2^-25 (|R col i|_1 + |R col j|_1) <= 2^-25 2 sqrt(3), a row sum of three by 6 sqrt(3) 2^-25; det(R + E) - 1 =
# sum cof_ij E_ij + O(E^2) with cof = R, so |det - 1| <= 2^-25 sum |R_ij| <= 3 sqrt(3) 2^-25.  (+ 1e-12 for the f64 orthonormality and E^2)
RIGID_ORTHO_TOL = 6 * np.sqrt(3.0) * 2.0 ** -25 + 1e-12
RIGID_DET_TOL = 3 * np.sqrt(3.0) * 2.0 ** -25 + 1e-12


def rigid_cases():
    """[(name, src, tgt, unique)] -- unique: the least-squares rotation is unique (the cross-covariance has rank >= 2 and, where its determinant
    is negative, distinct smallest singular values)"""
    rng = np.random.default_rng(8)
    R0 = _rotz(25.0) @ np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])
    t0 = np.array([1.0, -2.0, 0.5])
    move = lambda P: P @ R0.T + t0  # noqa: E731
    out = []
    for c in (1, 2, 3):
        P = rng.normal(size=(c, 3)) * [10, 5, 2]
        out.append(("c=%d" % c, P, move(P), c == 3))
    P = np.column_stack([rng.uniform(-20, 20, size=(50, 2)), np.full(50, 2.5)])
    out.append(("coplanar", P, move(P), True))
    P = np.column_stack([rng.uniform(-20, 20, size=(50, 2)), np.zeros(50)])
    out.append(("coplanar-z0-inplane", P, P @ _rotz(40.0).T + np.array([3.0, 1.0, 0.0]), True))  # the third row and column of the covariance are exactly 0
    P = np.outer(rng.uniform(-30, 30, size=40), [2.0, 1.0, 0.5]) + np.array([1.0, 2.0, 3.0])
    out.append(("collinear", P, move(P), False))
    P = np.column_stack([np.arange(-8.0, 9.0), np.zeros(17), np.zeros(17)])
    out.append(("collinear-x-axis", P, P + np.array([0.5, 0.25, -1.0]), False))  # covariance = one entry: u2 = A v2 is exactly 0 (n1 <= 1e-300, n0 > 0)
    P = rng.normal(size=(200, 3)) * [10, 5, 2]
    out.append(("mirrored", P, P * np.array([1.0, 1.0, -1.0]), True))  # det of the cross-covariance < 0
    P = rng.normal(size=(200, 3)) * [10, 5, 2]
    out.append(("mirrored-moved", P, move(P * np.array([1.0, 1.0, -1.0])), True))
    # isotropic in x and y: +-a on both axes, another spread on z; turned by exactly 90 degrees about z the cross-covariance is
    # [[0, -s, 0], [s, 0, 0], [0, 0, q]] and A^T A = diag(s^2, s^2, q^2): two exactly equal eigenvalues, no Jacobi rotation, the stable order decides
    P = np.array([[4, 0, 0], [-4, 0, 0], [0, 4, 0], [0, -4, 0], [0, 0, 2], [0, 0, -2]], float)
    out.append(("isotropic-xy", P, P @ _rotz(90.0).round().T + np.array([1.0, 2.0, 3.0]), True))
    P = np.array([[4, 0, 0], [-4, 0, 0], [0, 4, 0], [0, -4, 0], [0, 0, 8], [0, 0, -8]], float)  # the tied pair is the SMALLER one
    out.append(("isotropic-xy-small", P, P @ _rotz(90.0).round().T + np.array([1.0, 2.0, 3.0]), True))
    for c in (1023, 1024, 1025):
        P = rng.normal(size=(c, 3)) * [10, 5, 2]
        out.append(("c=%d" % c, P, move(P) + 0.01 * rng.normal(size=(c, 3)), True))
    P = rng.normal(size=(300, 3)) * [10, 5, 2] + np.array([1.0e4, -1.0e4, 0.9e4])
    out.append(("far-1e4", P, move(P) + 0.01 * rng.normal(size=(300, 3)), True))
    return out


def cross_covariance_f32(src, tgt):
    """the cross-covariance the float Umeyama hands to its Kabsch step (inputs and means cast to f32, sums in f64, rounded onto the f32 grid
    of its largest entry): what decides which branch of gh_kabsch a case reaches"""
    s = np.asarray(src, np.float64).astype(np.float32).astype(np.float64)
    t = np.asarray(tgt, np.float64).astype(np.float32).astype(np.float64)
    ms = (s.sum(0) / s.shape[0]).astype(np.float32).astype(np.float64)
    mt = (t.sum(0) / t.shape[0]).astype(np.float32).astype(np.float64)
    A = (t - mt).T @ (s - ms) / s.shape[0]
    mx = np.abs(A).max()
    if mx > 0:
        q = 2.0 ** (np.frexp(mx)[1] - 1 - 23)
        A = np.rint(A / q) * q
    return A


def kabsch_branches(src, tgt, jacobi3):
    """Which branches of gh_kabsch (devmath.h) the case reaches, from its text: jacobi3(3 x 3) -> (eigenvalues, eigenvectors in columns) is
    the contract's Jacobi (N3).  n0_zero: u1 = A v1 is exactly 0; n1_zero: u2 = A v2 - (.) u1 is exactly 0; reflect: det V < 0 after the
    ordering; ev_tie: two eigenvalues exactly equal, the stable order decides."""
    A = cross_covariance_f32(src, tgt)
    ata = A.T @ A
    ev, V = jacobi3(ata)
    order = [0, 1, 2]
    for i in range(1, 3):
        j = i
        while j > 0 and ev[order[j]] > ev[order[j - 1]]:
            order[j], order[j - 1] = order[j - 1], order[j]
            j -= 1
    v = np.asarray(V, np.float64).reshape(3, 3)[:, order]
    u0 = A @ v[:, 0]
    n0 = np.sqrt((u0 * u0).sum())
    u0 = u0 / n0 if n0 > 0 else np.array([1.0, 0, 0])
    u1 = A @ v[:, 1]
    u1 = u1 - (u1 @ u0) * u0
    n1 = np.sqrt((u1 * u1).sum())
    evs = sorted(ev)
    return dict(n0_zero=not n0 > 0, n1_zero=not n1 > 1e-300, reflect=bool(np.linalg.det(v) < 0), ev_tie=bool(evs[0] == evs[1] or evs[1] == evs[2]),
                order=tuple(order))


def rigid_quality(M, src, tgt):
    """(|| R^T R - I ||_inf, |det R - 1|, correspondence RMSE under M)"""
    R = M[:3, :3]
    d = np.asarray(src, np.float64) @ R.T + M[:3, 3] - np.asarray(tgt, np.float64)
    return float(np.abs(R.T @ R - np.eye(3)).sum(axis=1).max()), float(abs(np.linalg.det(R) - 1.0)), float(np.sqrt((d * d).sum() / d.shape[0]))


def rigid_against_f64(M, src, tgt):
    """(rotation angle between M and the f64 optimum, |dt| / max|p|, RMSE excess / max|p|)"""
    O, _, _ = umeyama(src, tgt)
    scale = float(np.sqrt((np.concatenate([src, tgt]) ** 2).sum(axis=1)).max())
    cosang = (np.trace(M[:3, :3] @ O[:3, :3].T) - 1.0) / 2.0
    # the angle through the sine as well: arccos alone cannot resolve 1e-7 rad
    skew = M[:3, :3] @ O[:3, :3].T
    sin = 0.5 * np.sqrt((skew[2, 1] - skew[1, 2]) ** 2 + (skew[0, 2] - skew[2, 0]) ** 2 + (skew[1, 0] - skew[0, 1]) ** 2)
    ang = float(np.arctan2(sin, cosang))
    dt = float(np.linalg.norm(M[:3, 3] - O[:3, 3])) / scale
    ex = (rigid_quality(M, src, tgt)[2] - rigid_quality(O, src, tgt)[2]) / scale
    return ang, dt, ex
