"""The iteration loop (loop.hip, loop_dev.h, pair_loop.hip) at its tile edges, on exact ties and on degenerate matches, against the CPU oracle and
against the independent restatement of tests/loop_edge_cases.py (tests/test_loop_edges_cpu.py proves, without a GPU, that every case is in the
regime it names and that a wrong tie partner moves the 4x4 by more than 1e-3 -- the comparisons here hold it to 1e-6):
  * ties (bit-equal combined distances) inside a column chunk, across the 32-column chunk, across an intermediate chunk of a batch and across
    CHUNK_MAX, for the row arg-min and for NNR's column arg-min (rows 255 | 256 and the chunk_a boundaries), FEATURE_NONE and FEATURE_BSC;
  * the per-stage NN / NNR kernels and the fused Kuhn-Munkres loop against the ORACLE at shapes around the 256-row block, the 512-column
    chunk and the second 1024-round of the compaction;
  * ghicp_register_clouds batches whose size gives chunk 32, an intermediate chunk (38 / 50) and CHUNK_MAX with a last chunk of one column;
  * coplanar, collinear, identical, mirrored keypoints; min_cor - 1, min_cor, one and no correspondence; an FPFH matrix with a NaN row;
  * ghicp_rigid_svd and ghicp_rigid_svd_host on rank-deficient, mirrored, isotropic, 1023 .. 1025-point and far-from-the-origin sets."""
import os

import numpy as np
import pytest

import loop_edge_cases as L
from test_gpu_loop import _compare_traces

pytestmark = pytest.mark.gpu

SIM = os.environ.get("GHICP_SIM") == "1"


def _params(api, oracle, feature, corr, bbx, max_iter, est_iou=None):
    ft_g, ft_o = {L.NONE: (api.FEATURE_NONE, oracle.NONE), L.BSC: (api.FEATURE_BSC, oracle.BSC), "fpfh": (api.FEATURE_FPFH, oracle.FPFH)}[feature]
    iou = est_iou if est_iou is not None else (0.9 if feature == L.NONE else 0.6)
    return api.default_params(ft_g, corr, 6, iou, 1.5, bbx, max_iter=max_iter), oracle.default_params(ft_o, corr, 6, iou, 1.5, bbx, max_iter=max_iter)


def _register_both(ctx, api, oracle, feature, corr, kpS, kpT, FD, bbx, max_iter, rel=1e-9):
    """single-call ctx.register against oracle.register: iteration count, every record, the match lists bit for bit"""
    import torch

    pg, po = _params(api, oracle, feature, corr, bbx, max_iter)
    ro = oracle.register(po, kpS, kpT, None if FD is None else FD.astype(np.float64), want_matchlist=True)
    FDg = None
    if FD is not None:
        FDg = torch.from_numpy(FD.astype(np.float32) if feature == "fpfh" else FD.astype(np.uint16).view(np.int16)).to(ctx.dev)
    rg = ctx.register(pg, kpS, kpT, FDg, want_matchlist=True)
    assert rg["iters"] == ro["iters"]
    np.testing.assert_array_equal(rg["matchlist"], ro["matchlist"])
    _compare_traces(rg["trace"], ro["trace"], rel=rel)
    np.testing.assert_allclose(rg["Rt"], ro["Rt"], rtol=0, atol=1e-6)  # (NaN == NaN)
    return rg, ro


# ------------------------------------------------------------------------------------------------ ties, single call
SINGLE_TIES = L.single_call_tie_cases()


@pytest.mark.parametrize("corr", [L.NN, L.NNR])
@pytest.mark.parametrize("case", SINGLE_TIES, ids=[c["name"] for c in SINGLE_TIES])
def test_ties_single_call(ctx, api, oracle, case, corr):
    """chunk 32 on both sweeps: ties inside chunk 0, across 31 | 32 and 511 | 512, tie rows in both row blocks; NNR: targets between the
    source rows 31 | 32 and 255 | 256.  The first index wins (ghicp_reg.cpp:715-724, 622-650)."""
    r = L.regimes(case["ks"], case["kt"], 1)
    assert (r["chunk_b"], r["chunk_a"], r["rowblocks"]) == (32, 32, 2)
    rg, _ = _register_both(ctx, api, oracle, case["feature"], corr, case["kpS"], case["kpT"], case.get("FD"), case["bbx"], max_iter=4)
    m = L.match_once(case["kpS"], case["kpT"], case.get("FD"), case["feature"], corr, case["bbx"])
    np.testing.assert_array_equal(rg["matchlist"][0], m["matchrow"])  # the independent restatement, directly
    assert rg["trace"][0]["cor"] == m["cor"]
    assert rg["trace"][0]["cdmean"] == pytest.approx(m["cdmean"], rel=1e-12) and rg["trace"][0]["penalty"] == pytest.approx(m["penalty"], rel=1e-12)


# ------------------------------------------------------------------------------------------------ shapes
@pytest.fixture(scope="module")
def shape_pair(synth, oracle):
    return L.shape_pair(synth, oracle.bbx_magnitude)


def _shape_fd(feature, ks, kt):
    return None if feature == L.NONE else L.fake_bsc_fd(np.random.default_rng(100 + ks * 7 + kt), ks, kt)


@pytest.mark.parametrize("feature", [L.NONE, L.BSC])
@pytest.mark.parametrize("corr", [L.NN, L.NNR])
@pytest.mark.parametrize("ks,kt", L.SHAPES)
def test_shapes_nn_nnr(ctx, api, oracle, shape_pair, ks, kt, corr, feature):
    """the per-stage kernels at the row block (255 / 256 / 257), around one CHUNK_MAX (513), below one minimum chunk (31) and in the second
    1024-round of the compaction (1025 rows; 1025 columns for NNR's column arg-min)"""
    S, T, bbx = shape_pair
    rg, _ = _register_both(ctx, api, oracle, feature, corr, S[:ks], T[:kt], _shape_fd(feature, ks, kt), bbx, max_iter=12)
    if min(ks, kt) >= 31:
        assert rg["iters"] >= 2, (ks, kt, rg["iters"])


@pytest.mark.parametrize("feature", [L.NONE, L.BSC])
@pytest.mark.parametrize("ks,kt", L.KM_SHAPES)
def test_shapes_km_fused_loop_against_the_oracle(ctx, api, oracle, shape_pair, ks, kt, feature):
    """the persistent pair loop with its fused stages -- tests/test_gpu_loop_fused.py holds it to the unfused path, this to the oracle"""
    S, T, bbx = shape_pair
    rg, _ = _register_both(ctx, api, oracle, feature, L.KM, S[:ks], T[:kt], _shape_fd(feature, ks, kt), bbx, max_iter=L.KM_MAX_ITER)
    if min(ks, kt) >= 31:
        assert rg["iters"] >= 2, (ks, kt, rg["iters"])


# ------------------------------------------------------------------------------------------------ batched chunk regimes
def _filler_strings(rng, ks, kt):
    fS = rng.integers(0, 256, size=(4, ks, 56), dtype=np.uint8)
    fT = rng.integers(0, 256, size=(kt, 56), dtype=np.uint8)
    m = min(ks, kt)
    fT[:m] = fS[0, :m] ^ (rng.random((m, 56)) < 0.03).astype(np.uint8)  # keypoint i <-> keypoint i: close strings
    return fS, fT


@pytest.mark.parametrize("feature", [L.NONE, L.BSC])
@pytest.mark.parametrize("corr", [L.NN, L.NNR])
@pytest.mark.parametrize("batch", list(L.BATCHES))
def test_batched_chunk_regimes(ctx, api, synth, oracle, shape_pair, batch, corr, feature):
    """ghicp_register_clouds hands its pairs to the loop as one batch, whose size decides the chunks (the mirror of pick_chunks says which).
    The batch holds the tie pairs of the regime -- tied columns on its chunk boundaries -- and, with the same shapes, pairs of the rotated and
    jittered keypoints; the same handles serve many pairs.  Once with max_iter = 1 (the first iteration's 4x4 is the result: what the CPU test
    shows a wrong tie partner to move) and once with 6.  Per pair against the oracle; no bit-equality with the single call (other partial sums)."""
    if SIM and batch == "chunkmax":
        pytest.skip("2048 pairs through the host SIMT interpreter run for minutes; the MI355X runs them")
    n, shapes = L.BATCHES[batch]
    for (ks, kt, _, _, _), want in zip(shapes, L.BATCH_EXPECT[batch]):
        got = L.regimes(ks, kt, n)
        assert {k: got[k] for k in want} == want, (ks, kt, got)
    S, T, bbx = shape_pair
    rng = np.random.default_rng(5)
    distinct = [(c["kpS"], c["kpT"], c.get("fS"), c.get("fT"), c["bbx"], c["name"]) for c in L.batch_tie_cases(batch, feature)]
    for ks, kt, _, _, _ in shapes:
        fS, fT = _filler_strings(rng, ks, kt) if feature == L.BSC else (None, None)
        distinct.append((S[:ks], T[:kt], fS, fT, bbx, "jittered-%dx%d" % (ks, kt)))
    ft_g = api.FEATURE_BSC if feature == L.BSC else api.FEATURE_NONE
    ft_o = oracle.BSC if feature == L.BSC else oracle.NONE
    iou = 0.6 if feature == L.BSC else 0.9
    cfg = api.pair_config(ft_g, corr, dof=6, est_iou=iou, voxel=0.2, pattern=synth.bsc_pattern_glibc(), max_iter=1)
    handles = []
    for kS, kT, fS, fT, b, _ in distinct:
        hS = ctx.cloud_from_features(cfg, kS, fS, b)
        hT = ctx.cloud_from_features(cfg, kT, None if fT is None else np.repeat(fT[None], 4, axis=0), b)
        handles.append((hS, hT))
    # every distinct pair once, then the pairs of the smallest shape again and again until the batch has its size
    small = [i for i, d in enumerate(distinct) if d[0].shape[0] == min(x[0].shape[0] for x in distinct)]
    which = [i if i < len(distinct) else small[(i - len(distinct)) % len(small)] for i in range(n)]
    pairs = [handles[w] for w in which]
    assert set(which) == set(range(len(distinct)))
    try:
        multi_iteration = False
        for max_iter in (1, 6):
            cfg = api.pair_config(ft_g, corr, dof=6, est_iou=iou, voxel=0.2, pattern=synth.bsc_pattern_glibc(), max_iter=max_iter)
            got = ctx.register_clouds(cfg, pairs)
            refs = []
            for kS, kT, fS, fT, b, _ in distinct:
                po = oracle.default_params(ft_o, corr, 6, iou, 1.5, b, max_iter=max_iter)
                refs.append(oracle.register(po, kS, kT, None if fS is None else oracle.fd_bsc(fS, fT).astype(np.float64)))
            for st, w in zip(got, which):
                r, name = refs[w], distinct[w][5]
                assert st.iterations == r["iters"] and st.converged == r["trace"][-1]["converged"], (name, max_iter)
                np.testing.assert_allclose(np.array(st.Rt[:]).reshape(4, 4), r["Rt"], rtol=0, atol=1e-6, err_msg="%s max_iter=%d" % (name, max_iter))
                assert st.rmse_after == pytest.approx(r["trace"][-1]["rmse_after"], rel=1e-9), (name, max_iter)
                multi_iteration |= st.iterations >= 2
        assert multi_iteration
    finally:
        for a, b in handles:
            a.close()
            b.close()


# ------------------------------------------------------------------------------------------------ degenerate matches
DEGENERATE = L.degenerate_cases()


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_matches(ctx, api, oracle, name):
    """FEATURE_NONE, NN: rank-deficient and mirrored correspondences through the loop's own solve (dev_solve), both sides of min_cor
    (ghicp_reg.cpp:796), one correspondence, and none -- whose NaN records compare NaN == NaN and whose call returns cleanly"""
    c = DEGENERATE[name]
    rg, ro = _register_both(ctx, api, oracle, L.NONE, L.NN, c["kpS"], c["kpT"], None, c["bbx"], max_iter=6)
    e = c["expect"]
    if "cor" in e:
        assert rg["trace"][0]["cor"] == e["cor"] and rg["trace"][0]["converged"] == (1 if e["cor"] < 10 else 0)
        assert rg["iters"] == (1 if e["cor"] < 10 else ro["iters"]) and (e["cor"] < 10 or rg["iters"] >= 2)
    if e.get("cor") == 0:
        assert np.isnan(rg["trace"][0]["rmse"]) and np.isnan(rg["trace"][0]["rmse_after"]) and np.isnan(rg["Rt"][:3]).all()
    if "all_take" in e:
        assert (rg["matchlist"][0] == e["all_take"]).all()
    R = rg["trace"][0]["Rt"][:3, :3]
    if not e.get("cor") == 0:  # whatever the rank of the correspondences: a proper rotation
        assert np.abs(R.T @ R - np.eye(3)).sum(axis=1).max() <= L.RIGID_ORTHO_TOL and abs(np.linalg.det(R) - 1) <= L.RIGID_DET_TOL


@pytest.mark.parametrize("corr", [L.NN, L.NNR])
def test_fpfh_energy_with_a_nan_feature_row(ctx, api, oracle, shape_pair, corr):
    """the similarity of a constant histogram is NaN (fd_fpfh): its row never wins an arg-min and CDmean is NaN -- NN accepts nothing
    (best < NaN), NNR needs no penalty and iterates; records and match lists equal the oracle's, NaN-aware.  (Not for Kuhn-Munkres: a
    non-finite weight is an error of that solver.)"""
    S, T, bbx = shape_pair
    c = L.fpfh_nan_case(oracle.fd_fpfh)
    rg, _ = _register_both(ctx, api, oracle, "fpfh", corr, S[:c["ks"]], T[:c["kt"]], c["FD"], bbx, max_iter=10, rel=1e-7)  # device pow() vs glibc pow()
    assert np.isnan(rg["trace"][0]["cdmean"]) and (rg["matchlist"][:, c["row"]] == -1).all()
    assert rg["trace"][0]["cor"] == 0 if corr == L.NN else rg["trace"][0]["cor"] > 10


# ------------------------------------------------------------------------------------------------ the rigid solve
RIGID = L.rigid_cases()


@pytest.mark.parametrize("name,src,tgt,unique", RIGID, ids=[c[0] for c in RIGID])
def test_rigid_svd(ctx, api, oracle, name, src, tgt, unique):
    """ghicp_rigid_svd (k_rigid_svd) and ghicp_rigid_svd_host:
    1. device == host == oracle.rigid_svd, bit for bit;
    2. R is a proper rotation within the f32 rounding of its nine entries.  Every entry is an f32 rounding of an entry of an f64-orthonormal
       matrix, |E_ij| <= 2^-25.  R^T R - I = E^T R + R^T E + E^T E: an entry is at most 2^-25 (|col i|_1 + |col j|_1) <= 2^-25 2 sqrt(3), a row
       sum 6 sqrt(3) 2^-25 = 3.10e-7; det(R + E) - 1 = sum cof_ij E_ij + O(E^2) with cof = R: |det R - 1| <= 3 sqrt(3) 2^-25 = 1.55e-7;
    3. against the f64 SVD Umeyama: rotation angle and |dt| where the rotation is unique, the excess of the correspondence RMSE over the
       f64 optimum's everywhere (rank-deficient sets included) -- tolerances measured on the CPU (tests/test_loop_edges_cpu.py), not here."""
    Rg, Rh, Ro = ctx.rigid_svd(src, tgt), api.rigid_svd_host(src, tgt), oracle.rigid_svd(src, tgt)
    np.testing.assert_array_equal(Rg, Ro)
    np.testing.assert_array_equal(Rh, Ro)
    ortho, det, _ = L.rigid_quality(Rg, src, tgt)
    assert ortho <= L.RIGID_ORTHO_TOL and det <= L.RIGID_DET_TOL, (ortho, det)
    np.testing.assert_array_equal(Rg[3], [0, 0, 0, 1])
    ang, dt, ex = L.rigid_against_f64(Rg, src, tgt)
    if unique:
        assert ang <= L.RIGID_ANGLE_TOL and dt <= L.RIGID_DT_TOL, (ang, dt)
    assert ex <= L.RIGID_RMSE_TOL, ex
