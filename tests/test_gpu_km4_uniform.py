"""The Kuhn-Munkres solver's wave-uniform state in scalar registers (km4_dev.h: k4_uni on the search's row, label, entry count, scan and
stack pointers and on the flood's queue): the matching must be, bit for bit, the restatement's of the reference's km.cpp and the
reference's own, in the standard and in the compact layout, at the sizes where a window or a ballot ends (63, 64, 65, 128, 129) and on the
families of tests/km4_uniform_cases.py -- marches longer than a window, rows with 3 / 4 / 6 / 7 tight entries, roots that match at once, a
search that steps back on its first step -- and through the literal fallback.  One loop-level case: ten pairs through two slots."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import km4_uniform_cases as U  # noqa: E402

pytestmark = pytest.mark.gpu


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
def solved(oracle):
    """every case with the oracle's matching (and the reference's own, where it was built), computed once"""
    out = []
    for fam, n, w in U.cases():
        ref = oracle.km(w)[0]
        own = oracle.km_reference(w)
        if own is not None:
            np.testing.assert_array_equal(ref, own, err_msg="oracle against km.cpp, %s n=%d" % (fam, n))
        out.append((fam, n, w, ref))
    return out


@pytest.fixture(scope="module")
def contexts(api):
    std = _context(api, GHICP_KM_COMPACT="0")
    cpt = _context(api, GHICP_KM_COMPACT_FROM="1")
    yield std, cpt
    std.close()
    cpt.close()


def test_matching_equals_the_reference_traversal_in_both_layouts(contexts, solved):
    std, cpt = contexts
    for fam, n, w, ref in solved:
        np.testing.assert_array_equal(std.km_solve(w).cpu().numpy(), ref, err_msg="standard %s n=%d" % (fam, n))
        np.testing.assert_array_equal(cpt.km_solve(w).cpu().numpy(), ref, err_msg="compact %s n=%d" % (fam, n))


def test_matching_through_the_hazard_fallback(api, solved):
    """flag 4 (GHICP_KM_FORCE_HAZARD): the phase of root n / 2 ends in the literal solver, a call of its own off the hot path"""
    for env in ({"GHICP_KM_COMPACT": "0"}, {"GHICP_KM_COMPACT_FROM": "1"}):
        c = _context(api, GHICP_KM_FORCE_HAZARD="1", **env)
        for fam, n, w, ref in solved:
            if n <= 65:  # the literal solver is one lane running the reference line by line
                np.testing.assert_array_equal(c.km_solve(w).cpu().numpy(), ref, err_msg="%s %s n=%d" % (env, fam, n))
        c.close()


def test_ten_pairs_through_two_slots(api, synth, oracle):
    """One register_clouds batch of ten pairs through TWO slots (GHICP_LOOP_SLOTS=2): a slot pops a pair, runs its iterations and pops the
    next -- the popped index, the pair's descriptor and its loop state are what the kernel now holds in scalar registers.  Every pair must
    come out as when it is registered alone (no Kuhn-Munkres batch of this size leaves the persistent loop, so that is the reference)."""
    two = _context(api, GHICP_LOOP_SLOTS="2")
    one = _context(api)
    rng = np.random.default_rng(43)
    cfg = api.pair_config(api.FEATURE_BSC, api.CORR_KM, dof=6, est_iou=0.6, voxel=0.2, pattern=synth.bsc_pattern_glibc(), max_iter=5)
    p = synth.gauss_pair(n_kp=300)
    bbx = float(oracle.bbx_magnitude(p.source))
    S = p.source[p.kp_source].astype(np.float64)
    ang = np.deg2rad(12.0)
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    T = S @ R.T + np.array([1.5, -0.8, 0.3]) + 0.02 * rng.standard_normal(S.shape)
    shapes = [(129, 128), (120, 100), (64, 65), (63, 64), (90, 90), (128, 129), (33, 70), (65, 64), (97, 96), (40, 41)]
    feats = []
    for ks, kt in shapes:
        fS = rng.integers(0, 256, size=(4, ks, 56), dtype=np.uint8)
        fT = rng.integers(0, 256, size=(4, kt, 56), dtype=np.uint8)
        m = min(ks, kt)
        half = np.arange(m)[rng.random(m) < 0.5]
        fT[0, half] = fS[0, half] ^ (rng.random((half.size, 56)) < 0.03).astype(np.uint8)
        false = np.arange(ks)[rng.random(ks) < 0.3]
        fS[1, false] = fT[0, rng.integers(0, kt, false.size)] ^ (rng.random((false.size, 56)) < 0.03).astype(np.uint8)
        feats.append((S[:ks], T[:kt], fS, fT))
    mk = lambda cx: [(cx.cloud_from_features(cfg, kS, fS, bbx), cx.cloud_from_features(cfg, kT, fT, bbx)) for kS, kT, fS, fT in feats]  # noqa: E731
    h2, h1 = mk(two), mk(one)
    got = two.register_clouds(cfg, h2)
    alone = [one.register_clouds(cfg, [h])[0] for h in h1]
    assert max(a.iterations for a in alone) >= 3
    for a, b, sh in zip(alone, got, shapes):
        assert a.iterations == b.iterations and a.converged == b.converged and list(a.Rt) == list(b.Rt) and a.rmse_after == b.rmse_after, sh
    for a, b in h2 + h1:
        a.close()
        b.close()
    two.close()
    one.close()
