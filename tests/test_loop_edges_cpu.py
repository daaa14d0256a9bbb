"""The cases of tests/loop_edge_cases.py, without a GPU: every case is in the regime it names (through the mirror of pick_chunks and ROWS), every
tie case holds bit-equal CD values at the named columns and the wrong tie rule ("last index wins", or the other partner in a single row)
moves the iteration's 4x4 by more than 1e-3, the oracle's first iteration equals the independent numpy restatement (index work exactly,
scalars within rel 1e-12), the degenerate cases are what they claim, and the rigid solve of the oracle against an f64 SVD Umeyama.

The rigid solve, measured here with oracle.rigid_svd (the reference of the GPU solve) against numpy's f64 SVD over rigid_cases():
    largest rotation angle between the two R (cases with a unique rotation)    5.72e-6 rad       (far-1e4: coordinates near 1e4 m, spread ~10 m)
    largest |dt| / max|p| (the same cases)                                     4.53e-6           (far-1e4)
    largest (RMSE under the returned 4x4 - RMSE of the f64 optimum) / max|p|   3.20e-8           (c=1: the f32 rounding of t)
    everywhere else: angle <= 2.7e-7 rad, |dt| / max|p| <= 4.6e-8, RMSE excess / max|p| <= 2.9e-8
    || R^T R - I ||_inf <= 9.7e-8 (bound 3.10e-7), |det R - 1| <= 2.5e-8 (bound 1.55e-7; loop_edge_cases.py derives both)
recorded (rounded up) as loop_edge_cases.RIGID_SEEN; the tolerances the GPU test imports are 4 x these: RIGID_ANGLE_TOL = 2.32e-5 rad,
RIGID_DT_TOL = 1.84e-5, RIGID_RMSE_TOL = 1.32e-7.  The margin covers the rounding of the covariance onto the f32 grid (N2) and the f32 rounding of
R and t, which scale with the coordinates."""
import numpy as np
import pytest

import loop_edge_cases as L


def _oracle_feature(oracle, case):
    return oracle.BSC if case["feature"] == L.BSC else oracle.NONE


def _all_tie_cases():
    out = list(L.single_call_tie_cases())
    for b in L.BATCHES:
        for f in (L.NONE, L.BSC):
            out += L.batch_tie_cases(b, f)
    return out


TIE_CASES = _all_tie_cases()


def test_pick_chunks_mirror_and_batch_regimes():
    """the mirror on hand-computed values of loop.hip:pick_chunks, and the regimes the batches name"""
    assert L.chunks(2000, 2000, 1) == (32, 63) and L.chunks(1, 1, 1) == (32, 1) and L.chunks(0, 0, 1) == (32, 1)
    assert L.chunks(12, 300, 256) == (38, 8)  # 256 row blocks, 8 chunks wanted, ceil(300 / 8)
    assert L.chunks(300, 12, 256) == (32, 1) and L.chunks(300, 200, 256) == (50, 4)
    assert L.chunks(4, 513, 2048) == (512, 2) and L.chunks(540, 513, 2048) == (512, 2)
    assert L.chunks(600, 600, 1 << 20) == (512, 2)  # the persistent pair loop: the largest chunks
    for name, (n, shapes) in L.BATCHES.items():
        for (ks, kt, bb, ba, _), want in zip(shapes, L.BATCH_EXPECT[name]):
            got = L.regimes(ks, kt, n)
            assert {k: got[k] for k in want} == want, (name, ks, kt, got)
            assert all(b % got["chunk_b"] == 0 for b in bb) and all(b % got["chunk_a"] == 0 or b % L.ROWS == 0 for b in ba), (name, ks, kt)
    r = L.regimes(12, 300, 256)
    assert 32 < r["chunk_b"] < 512 and r["chunk_b"] % 32 != 0
    r = L.regimes(200, 300, 256)
    assert 32 < r["chunk_a"] < 512 and r["chunk_a"] % 32 != 0
    r = L.regimes(4, 513, 2048)
    assert r["chunk_b"] == L.CHUNK_MAX and 513 - r["chunk_b"] * (r["nchunk_b"] - 1) == 1  # a last chunk of one column
    for ks, kt in L.SHAPES:  # a single call is a batch of one: chunk 32 everywhere
        r = L.regimes(ks, kt, 1)
        assert r["chunk_b"] == r["chunk_a"] == 32
    assert L.regimes(1025, 31, 1)["scan_rounds"] == 2 and L.regimes(31, 1025, 1)["scan_rounds"] == 2 and L.regimes(31, 1025, 1)["nchunk_a"] == 1
    assert [L.regimes(ks, kt, 1)["rowblocks"] for ks, kt in ((255, 257), (256, 256), (257, 255))] == [1, 1, 2]


@pytest.mark.parametrize("case", TIE_CASES, ids=[c["name"] for c in TIE_CASES])
def test_tie_case_is_what_it_names(case):
    n = case.get("batch", 1)
    reg = L.regimes(case["ks"], case["kt"], n)
    CD = L.cd_matrix(case["kpS"], case["kpT"], case.get("FD"), case["feature"], case["bbx"])
    geo = L.cd_matrix(case["kpS"], case["kpT"], None, L.NONE, case["bbx"])
    brk = case["feature"] == L.BSC and case["fd_mode"] == "break"
    inside, block_rows = 0, set()
    for r, cols, _ in case["row_ties"]:
        assert len(set(geo[r, list(cols)].tolist())) == 1, "the geometric tie is bit-exact"
        assert geo[r, cols[0]] == geo[r].min() and (geo[r] == geo[r].min()).sum() == len(cols)
        if brk:
            assert CD[r, cols[-1]] == CD[r].min() and (CD[r] == CD[r].min()).sum() == 1  # the feature distance alone decides: the LAST partner
        else:
            assert len(set(CD[r, list(cols)].tolist())) == 1 and CD[r, cols[0]] == CD[r].min() and (CD[r] == CD[r].min()).sum() == len(cols)
        ch = {c // reg["chunk_b"] for c in cols}
        inside += len(ch) == 1
        block_rows.add(r)
    for c, rows, _ in case["col_ties"]:
        assert geo[rows[0], c] == geo[rows[1], c] == geo[:, c].min() and (geo[:, c] == geo[:, c].min()).sum() == 2
        if brk:
            assert CD[rows[1], c] == CD[:, c].min() and (CD[:, c] == CD[:, c].min()).sum() == 1  # the HIGHER row is the closer one
        else:
            assert CD[rows[0], c] == CD[rows[1], c] == CD[:, c].min() and (CD[:, c] == CD[:, c].min()).sum() == 2
        assert rows[0] // reg["chunk_a"] != rows[1] // reg["chunk_a"] or rows[0] // L.ROWS != rows[1] // L.ROWS, "the tied rows straddle a boundary"
    assert inside >= 1
    # the boundaries the case was built for, as the mirror sees them
    shape = next(s for s in (L.BATCHES[case["name"].split("-")[0]][1] if "batch" in case else [(300, 600, [32, 512], [32, 256], (253, 258))])
                 if s[0] == case["ks"] and s[1] == case["kt"])
    for B in shape[2]:
        assert B % reg["chunk_b"] == 0 and any(B - 1 in cols and B in cols for _, cols, _ in case["row_ties"]), B
        if B + 1 < case["kt"]:
            assert any(B - 2 in cols and B + 1 in cols for _, cols, _ in case["row_ties"]), B
    for B in shape[3]:
        assert (B % reg["chunk_a"] == 0 or B % L.ROWS == 0) and any(rows == (B - 1, B) for _, rows, _ in case["col_ties"]), B
    if shape[4]:
        assert set(shape[4]) <= block_rows and len({r // L.ROWS for r in shape[4]}) == 2  # tie rows in both row blocks


@pytest.mark.parametrize("corr", [L.NN, L.NNR])
@pytest.mark.parametrize("case", TIE_CASES, ids=[c["name"] for c in TIE_CASES])
def test_wrong_tie_rule_moves_the_transform(case, corr):
    """a tie case that cannot show the wrong partner in the 4x4 is not a test"""
    good, m = L.first_Rt(case, corr)
    brk = case["feature"] == L.BSC and case["fd_mode"] == "break"
    if not brk:
        bad, _ = L.first_Rt(case, corr, tie="last")
        assert np.abs(good - bad).max() > 1e-3
    for r, cols, _ in case["row_ties"]:  # ... and row by row: the other end of the tie in this row alone
        right, wrong = (cols[-1], cols[0]) if brk else (cols[0], cols[-1])
        assert m["SV"][r] == right and m["matchrow"][r] == right
        bad, _ = L.first_Rt(case, corr, override={r: wrong})
        assert np.abs(good - bad).max() > 1e-3, (r, cols)
    if corr == L.NNR:
        for c, rows, _ in case["col_ties"]:  # the column tie: the correspondence of column c goes to the lower row (to the closer one: "break")
            right, wrong = (rows[1], rows[0]) if brk else (rows[0], rows[1])
            assert m["TV"][c] == right and m["matchrow"][right] == c and m["matchrow"][wrong] == -1
            SP = np.where(m["SP"] == right, wrong, m["SP"])
            bad = L.umeyama(case["kpS"][SP], case["kpT"][m["TP"]])[0]
            assert np.abs(good - bad).max() > 1e-3, (c, rows)


def _first_iteration_equals(oracle, feature, corr, kpS, kpT, FD, bbx, est_iou):
    po = oracle.default_params(feature, corr, 6, est_iou, 1.5, bbx, max_iter=1)
    ro = oracle.register(po, kpS, kpT, FD, want_matchlist=True)
    m = L.match_once(kpS, kpT, FD, L.BSC if feature == oracle.BSC else L.NONE, corr, bbx)
    r = ro["trace"][0]
    np.testing.assert_array_equal(ro["matchlist"][0], m["matchrow"])
    assert r["cor"] == m["cor"]
    assert r["cdmean"] == pytest.approx(m["cdmean"], rel=1e-12) and r["penalty"] == pytest.approx(m["penalty"], rel=1e-12)
    return ro, m


@pytest.mark.parametrize("corr", [L.NN, L.NNR])
@pytest.mark.parametrize("case", TIE_CASES, ids=[c["name"] for c in TIE_CASES])
def test_oracle_equals_restatement_on_ties(oracle, case, corr):
    if case["feature"] == L.BSC:
        np.testing.assert_array_equal(oracle.fd_bsc(case["fS"], case["fT"]), case["FD"])
    ro, m = _first_iteration_equals(oracle, _oracle_feature(oracle, case), corr, case["kpS"], case["kpT"], case.get("FD"), case["bbx"], 0.6)
    # the float Umeyama of the oracle against the f64 one on the same correspondences: far inside the 1e-3 a wrong partner costs
    np.testing.assert_allclose(ro["trace"][0]["Rt"], L.first_Rt(case, corr)[0], rtol=0, atol=1e-4)


@pytest.fixture(scope="module")
def shape_pair(synth, oracle):
    return L.shape_pair(synth, oracle.bbx_magnitude)


@pytest.mark.parametrize("feature", [L.NONE, L.BSC])
@pytest.mark.parametrize("corr", [L.NN, L.NNR])
@pytest.mark.parametrize("ks,kt", L.SHAPES)
def test_oracle_equals_restatement_on_shapes(oracle, shape_pair, ks, kt, corr, feature):
    S, T, bbx = shape_pair
    FD = None if feature == L.NONE else L.fake_bsc_fd(np.random.default_rng(100 + ks * 7 + kt), ks, kt)
    _first_iteration_equals(oracle, oracle.BSC if feature == L.BSC else oracle.NONE, corr, S[:ks], T[:kt], FD, bbx, 0.9 if feature == L.NONE else 0.6)


def test_degenerate_cases_are_what_they_claim(oracle):
    for name, c in L.degenerate_cases().items():
        ro, m = _first_iteration_equals(oracle, oracle.NONE, L.NN, c["kpS"], c["kpT"], None, c["bbx"], 0.9)
        e = c["expect"]
        if "cor" in e:
            assert m["cor"] == e["cor"], name
            assert ro["trace"][0]["converged"] == (1 if e["cor"] < 10 else ro["trace"][0]["converged"]), name  # ghicp_reg.cpp:796, min_cor = 10
            if e["cor"] == 10:
                full = oracle.register(oracle.default_params(oracle.NONE, L.NN, 6, 0.9, 1.5, c["bbx"], max_iter=6), c["kpS"], c["kpT"])
                assert full["iters"] >= 2 and full["trace"][0]["cor"] == 10 and full["trace"][0]["converged"] == 0, name
            if e["cor"] == 0:
                assert (m["CD"] >= m["penalty"]).all() and np.isnan(ro["trace"][0]["rmse"]) and np.isnan(ro["trace"][0]["Rt"][:3]).all()
            continue
        _, s, det = L.umeyama(c["kpS"][m["SP"]], c["kpT"][m["TP"]])
        assert int((s > 1e-9 * max(s[0], 1e-300)).sum()) == e["rank"], (name, s)
        if e.get("det_negative"):
            assert det < 0 and (m["matchrow"] == np.arange(c["kpS"].shape[0])).all(), name
        if "all_take" in e:
            assert (m["SV"] == e["all_take"]).all() and m["CD"][0, e["tied"][0]] == m["CD"][0, e["tied"][1]] == m["CD"][0].min(), name
    z = L.degenerate_cases()
    assert np.ptp(z["coplanar"]["kpS"][:, 2]) == 0 and np.ptp(z["coplanar"]["kpT"][:, 2]) == 0


def test_fpfh_nan_row(oracle):
    c = L.fpfh_nan_case(oracle.fd_fpfh)
    assert np.isnan(c["FD"][c["row"]]).all() and np.isnan(c["FD"]).sum() == c["kt"]


def test_rigid_solve_of_the_oracle_against_f64_svd(oracle):
    """section 5's measurement: every value within what RIGID_SEEN records, the branches of gh_kabsch all reached"""
    seen = dict(angle=0.0, dt=0.0, rmse=0.0)
    reached = dict(n0_zero=[], n1_zero_only=[], reflect=[], ev_tie_full_rank=[])
    for name, src, tgt, unique in L.rigid_cases():
        M = oracle.rigid_svd(src, tgt)
        ortho, det, _ = L.rigid_quality(M, src, tgt)
        assert ortho <= L.RIGID_ORTHO_TOL and det <= L.RIGID_DET_TOL, (name, ortho, det)
        ang, dt, ex = L.rigid_against_f64(M, src, tgt)
        _, s, dH = L.umeyama(src, tgt)
        assert unique == bool(s[1] > 1e-3 * s[0] and (dH >= 0 or s[1] - s[2] > 1e-3 * s[0])), (name, s)
        if unique:
            seen["angle"], seen["dt"] = max(seen["angle"], ang), max(seen["dt"], dt)
        seen["rmse"] = max(seen["rmse"], ex)
        b = L.kabsch_branches(src, tgt, oracle.jacobi3)
        if b["n0_zero"]:
            reached["n0_zero"].append(name)
        if b["n1_zero"] and not b["n0_zero"]:
            reached["n1_zero_only"].append(name)
        if b["reflect"]:
            reached["reflect"].append(name)
        if b["ev_tie"] and s[2] > 1e-3 * s[0]:
            reached["ev_tie_full_rank"].append((name, b["order"]))
    print("rigid solve, oracle vs f64 SVD:", seen, reached)
    for k in seen:
        assert seen[k] <= L.RIGID_SEEN[k], (k, seen[k])
        assert seen[k] >= 0.5 * L.RIGID_SEEN[k], "the record is stale: measure again"
    assert reached["n0_zero"] == ["c=1"] and "collinear-x-axis" in reached["n1_zero_only"] and reached["reflect"], reached
    # the tie among the two LARGEST eigenvalues keeps its order, the tie among the two smallest comes after the largest
    assert dict(reached["ev_tie_full_rank"]) == {"isotropic-xy": (0, 1, 2), "isotropic-xy-small": (2, 0, 1)}
    assert L.RIGID_ANGLE_TOL == 4 * L.RIGID_SEEN["angle"] and L.RIGID_DT_TOL == 4 * L.RIGID_SEEN["dt"] and L.RIGID_RMSE_TOL == 4 * L.RIGID_SEEN["rmse"]


def test_rigid_host_solve_equals_the_oracle(api, oracle):
    """ghicp_rigid_svd_host needs no GPU: the same bits as the oracle on every case"""
    for name, src, tgt, _ in L.rigid_cases():
        np.testing.assert_array_equal(api.rigid_svd_host(src, tgt), oracle.rigid_svd(src, tgt), err_msg=name)
