"""The persistent pair loop's fused stages (pair_loop.hip: pl_sweep_km / pl_graph_km -- one combined-distance pass per iteration decides the graph's
membership while it takes the sums, the fill reads the row bitmask) against the three passes of before (GHICP_LOOP_FUSE=0: pl_sweep / pl_graph):
every field of every iteration record, the iteration count, the 4x4 and the match lists must be the SAME BITS.  The shapes stand at the edges
of the code's tiles: the 256-row blocks, the 512-column chunk, the padding rows of ks < kt and ks > kt, the 32-bit mask word and the 64-column
block.  A count / fill mismatch (km_status bit 8) fails the registration call itself, so every case that returns has shown that it did not fire.
Parity with the oracle is what tests/test_gpu_loop.py, the golden and the full-size tests assert; here the reference is the unfused path."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_ITER = 8
SHAPES = [(255, 257), (256, 256), (257, 255), (300, 512), (300, 513), (513, 300), (64, 65), (65, 64), (3, 5)]


def _context(api, **env):
    """a context of its own: the switches are read from the environment once, when a context is created"""
    import torch

    os.environ.update(env)
    try:
        if os.environ.get("GHICP_SIM") == "1":
            from hipsim import simctx

            return simctx.make_context(api)
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        return api.Context(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def contexts(api):
    fused = _context(api)
    plain = _context(api, GHICP_LOOP_FUSE="0")
    yield fused, plain
    fused.close()
    plain.close()


@pytest.fixture(scope="module")
def pair(synth, oracle):
    """source keypoints of a synthetic scan; the target is the source moved by 12 degrees and 1.7 m (keypoint i <-> keypoint i), so that the
    loop has a motion to recover"""
    p = synth.gauss_pair(n_kp=600)
    S = p.source[p.kp_source].astype(np.float64)
    a = np.deg2rad(12.0)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    T = S @ R.T + np.array([1.5, -0.8, 0.3]) + 0.02 * np.random.default_rng(1).standard_normal(S.shape)
    return S, T, float(oracle.bbx_magnitude(p.source))


def _fake_bsc_fd(rng, ks, kt):
    """u16 feature distances as test_gpu_loop.py makes them (60..200, the true partner 5..40), but only half of the true partners are close
    and 1 % of all entries are false friends (5..45): the matching then changes while the feature weight decays, and the loop takes its
    max_iter iterations instead of two"""
    FD = rng.integers(60, 200, size=(ks, kt)).astype(np.float64)
    low = rng.random((ks, kt)) < 0.01
    FD[low] = rng.integers(5, 45, size=int(low.sum()))
    idx = np.arange(min(ks, kt))
    idx = idx[rng.random(idx.size) < 0.5]
    FD[idx, idx] = rng.integers(5, 40, size=idx.size)
    return FD


def _same(a, b, what):
    assert a["iters"] == b["iters"], what
    assert len(a["trace"]) == len(b["trace"]) == a["iters"], what
    for it, (x, y) in enumerate(zip(a["trace"], b["trace"])):
        assert set(x) == set(y)
        for k in x:
            np.testing.assert_array_equal(np.asarray(x[k]), np.asarray(y[k]), err_msg="%s it=%d %s" % (what, it, k))  # identical bits, NaN == NaN
    np.testing.assert_array_equal(a["Rt"], b["Rt"], err_msg=str(what))
    np.testing.assert_array_equal(a["matchlist"], b["matchlist"], err_msg=str(what))


def _both(contexts, params, kpS, kpT, FD):
    import torch

    out = []
    for c in contexts:
        FDg = None if FD is None else torch.from_numpy(FD).to(c.dev)
        out.append(c.register(params, kpS, kpT, FDg, want_matchlist=True))
    return out


@pytest.mark.parametrize("ks,kt", SHAPES)
def test_fused_equals_unfused_bsc_km(contexts, api, pair, ks, kt):
    S, T, bbx = pair
    FD = _fake_bsc_fd(np.random.default_rng(100 + ks * 7 + kt), ks, kt)
    pg = api.default_params(api.FEATURE_BSC, api.CORR_KM, 6, 0.6, 1.5, bbx, max_iter=MAX_ITER)
    a, b = _both(contexts, pg, S[:ks], T[:kt], FD.astype(np.int16))
    _same(a, b, (ks, kt))
    if (ks, kt) == (3, 5):
        assert a["iters"] == 1 and a["trace"][0]["converged"] == 1 and a["trace"][0]["cor"] < pg.min_cor  # stops at iteration 0
    elif min(ks, kt) >= 255:
        assert a["iters"] >= 4, (ks, kt, a["iters"])  # iterations 0-1 (count pass) and later ones (membership inside the sweep) both ran
    else:
        assert a["iters"] >= 2, (ks, kt, a["iters"])


def _cd_row(api, pg, S, T, FD, trace, it, i):
    """CD(i, .) of iteration `it` as the loop computes it (ghicp_reg.cpp:122, 259): the source keypoint moved by the iterations before"""
    s = np.append(S[i], 1.0)
    for r in trace[:it]:
        s = r["Rt"] @ s
    ed = float(np.float32(0.005 * pg.bbx_magnitude)) * np.sqrt(((s[:3] - T) ** 2).sum(axis=1))
    wfd = np.exp(-1.0 * it / pg.weight_changing_rate)
    return (1.0 - wfd) * ed + wfd * FD[i]


def test_rows_without_and_with_only_explicit_entries(contexts, api, pair):
    """Row 7 has no entry below the penalty (feature distance 250 to everybody), row 11 has ALL its kt entries below it
    (feature distance 0 to everybody): checked here from the records' penalties, at an iteration of the count pass and at one of the fused
    sweep -- an empty mask row and a row of full words (kt = 130: two full words and a partial one)."""
    S, T, bbx = pair
    ks, kt = 140, 130
    FD = _fake_bsc_fd(np.random.default_rng(5), ks, kt)
    FD[7, :] = 250
    FD[11, :] = 0
    pg = api.default_params(api.FEATURE_BSC, api.CORR_KM, 6, 0.6, 1.5, bbx, max_iter=MAX_ITER)
    a, b = _both(contexts, pg, S[:ks], T[:kt], FD.astype(np.uint16).view(np.int16))
    _same(a, b, "empty and full rows")
    assert a["iters"] >= 3
    for it in (0, 2):
        pen = a["trace"][it]["penalty"]
        assert (_cd_row(api, pg, S[:ks], T[:kt], FD, a["trace"], it, 7) > 1.5 * pen).all(), it  # (far from the threshold: no rounding question)
        assert (_cd_row(api, pg, S[:ks], T[:kt], FD, a["trace"], it, 11) < 0.75 * pen).all(), it


def test_fused_equals_unfused_fpfh_km(contexts, api, pair):
    S, T, bbx = pair
    ks, kt = 130, 150
    rng = np.random.default_rng(11)
    FD = (0.2 + 0.6 * rng.random((ks, kt))).astype(np.float32)
    FD[np.arange(ks), np.arange(ks)] = 0.97
    pg = api.default_params(api.FEATURE_FPFH, api.CORR_KM, 6, 0.6, 1.5, bbx, max_iter=MAX_ITER)
    a, b = _both(contexts, pg, S[:ks], T[:kt], FD)
    _same(a, b, "fpfh")
    assert a["iters"] >= 3  # iteration 2 takes the fused membership


def test_fused_equals_unfused_none_km(contexts, api, pair):
    """no feature: the penalty is this iteration's CDmean, so every iteration takes the sweep without membership and the count pass"""
    S, T, bbx = pair
    pg = api.default_params(api.FEATURE_NONE, api.CORR_KM, 6, 0.9, 1.5, bbx, max_iter=MAX_ITER)
    a, b = _both(contexts, pg, S[:150], T[:130], None)
    _same(a, b, "none")
    assert a["iters"] >= 3


def test_two_slots_take_large_then_small_pairs(api, synth, oracle):
    """One register_clouds batch of ten pairs of different n through TWO slots (GHICP_LOOP_SLOTS=2), largest graphs first: a slot runs a large
    pair and afterwards smaller ones on the same mask region, whose words of the large pair's rows are then stale.  Every pair must come out as
    when it is registered alone on the unfused context."""
    fused = _context(api, GHICP_LOOP_SLOTS="2")
    plain = _context(api, GHICP_LOOP_FUSE="0")
    rng = np.random.default_rng(41)
    cfg = api.pair_config(api.FEATURE_BSC, api.CORR_KM, dof=6, est_iou=0.6, voxel=0.2, pattern=synth.bsc_pattern_glibc(), max_iter=6)
    p = synth.gauss_pair(n_kp=300)
    bbx = float(oracle.bbx_magnitude(p.source))
    S = p.source[p.kp_source].astype(np.float64)
    ang = np.deg2rad(12.0)
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    T = S @ R.T + np.array([1.5, -0.8, 0.3]) + 0.02 * rng.standard_normal(S.shape)
    shapes = [(260, 250), (120, 100), (64, 199), (200, 190), (90, 90), (230, 257), (33, 70), (150, 65), (97, 96), (40, 41)]
    feats = []
    for ks, kt in shapes:
        fS = rng.integers(0, 256, size=(4, ks, 56), dtype=np.uint8)
        fT = rng.integers(0, 256, size=(4, kt, 56), dtype=np.uint8)
        m = min(ks, kt)
        half = np.arange(m)[rng.random(m) < 0.5]  # half of the true partners have close strings ...
        fT[0, half] = fS[0, half] ^ (rng.random((half.size, 56)) < 0.03).astype(np.uint8)
        false = np.arange(ks)[rng.random(ks) < 0.3]  # ... and a third of the rows a false friend (through another view of the source)
        fS[1, false] = fT[0, rng.integers(0, kt, false.size)] ^ (rng.random((false.size, 56)) < 0.03).astype(np.uint8)
        feats.append((S[:ks], T[:kt], fS, fT))
    mk = lambda cx: [(cx.cloud_from_features(cfg, kS, fS, bbx), cx.cloud_from_features(cfg, kT, fT, bbx)) for kS, kT, fS, fT in feats]  # noqa: E731
    hf, hp = mk(fused), mk(plain)
    fused.set_loop_cost_hints([float(max(ks, kt)) for ks, kt in shapes])
    got = fused.register_clouds(cfg, hf)
    alone = [plain.register_clouds(cfg, [h])[0] for h in hp]
    assert max(a.iterations for a in alone) >= 4
    for a, b, sh in zip(alone, got, shapes):
        assert a.iterations == b.iterations and a.converged == b.converged and list(a.Rt) == list(b.Rt) and a.rmse_after == b.rmse_after, sh
    for a, b in hf + hp:
        a.close()
        b.close()
    fused.close()
    plain.close()
