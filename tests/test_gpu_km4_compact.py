"""The compact LDS layout of the Kuhn-Munkres state (km4_dev.h: the column stack and the CSR offsets in a per-slot region of global
memory, 36 instead of 44 B per row, so that graphs of n = 925..1131 fit four to a CU).  GHICP_KM_COMPACT_FROM=1, the library's test hook,
forces it on every graph, so the shapes can be the small ones where the solver takes another path: the matching must be, bit for bit, what
the standard layout gives and what the restatement of the reference's km.cpp gives."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import km4_compact_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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
    """every case with the oracle's matching, computed once"""
    return [(fam, n, w, oracle.km(w)[0]) for fam, n, w in K.cases()]


@pytest.fixture(scope="module")
def contexts(api):
    std = _context(api, GHICP_KM_COMPACT="0")
    cpt = _context(api, GHICP_KM_COMPACT_FROM="1")
    yield std, cpt
    std.close()
    cpt.close()


def test_compact_equals_standard_equals_oracle(contexts, solved):
    std, cpt = contexts
    for fam, n, w, ref in solved:
        m_s = std.km_solve(w).cpu().numpy()
        m_c = cpt.km_solve(w).cpu().numpy()
        np.testing.assert_array_equal(m_s, ref, err_msg="standard %s n=%d" % (fam, n))
        np.testing.assert_array_equal(m_c, ref, err_msg="compact %s n=%d" % (fam, n))
        np.testing.assert_array_equal(m_c, m_s)


def test_compact_through_the_hazard_fallback(api, solved):
    """flag 4 (GHICP_KM_FORCE_HAZARD): one phase of every solve ends in the literal solver, which then works on the compact arrays"""
    c = _context(api, GHICP_KM_COMPACT_FROM="1", GHICP_KM_FORCE_HAZARD="1")
    for fam, n, w, ref in solved:
        if n <= 65:  # the literal solver is one lane running the reference line by line
            np.testing.assert_array_equal(c.km_solve(w).cpu().numpy(), ref, err_msg="%s n=%d" % (fam, n))
    c.close()


def test_compact_on_a_real_matrix(contexts, oracle):
    """iteration 10 of a bench pair (n = 351, four per CU in the standard layout) under the forcing hook"""
    z = np.load(os.path.join(GOLD, "km_cfg2_it10.npz"))
    n = int(z["n"])
    w = np.full((n, n), float(z["bg"]))
    w[z["rows"].astype(np.int64), z["cols"].astype(np.int64)] = z["vals"]
    ref = oracle.km(w)[0]
    for c in contexts:
        np.testing.assert_array_equal(c.km_solve(w).cpu().numpy(), ref)


def test_loop_batch_with_both_layouts_in_one_class(api, synth, oracle):
    """One register_clouds batch of small synthetic pairs, the compact layout forced from n = 200 on (GHICP_KM_COMPACT_FROM=200): half of the
    pairs take it, half the standard one, all in ONE class -- one launch, slots that change layout from pair to pair.  Every pair's iterations
    and 4x4 must be those of the same pair registered alone with the standard layout."""
    cpt = _context(api, GHICP_KM_COMPACT_FROM="200")
    std = _context(api, GHICP_KM_COMPACT="0")
    rng = np.random.default_rng(41)
    cfg = api.pair_config(api.FEATURE_BSC, api.CORR_KM, dof=6, est_iou=0.6, voxel=0.2, pattern=synth.bsc_pattern_glibc(), max_iter=6)
    p = synth.gauss_pair(n_kp=300)
    bbx = float(oracle.bbx_magnitude(p.source))
    shapes = [(120, 100), (260, 250), (64, 199), (200, 190), (90, 90), (230, 257)]
    feats = []
    for ks, kt in shapes:
        fS = rng.integers(0, 256, size=(4, ks, 56), dtype=np.uint8)
        fT = rng.integers(0, 256, size=(4, kt, 56), dtype=np.uint8)
        m = min(ks, kt)
        fT[0, :m] = fS[0, :m] ^ (rng.random((m, 56)) < 0.03).astype(np.uint8)
        feats.append((p.source[p.kp_source[:ks]].astype(np.float64), p.target[p.kp_target[:kt]].astype(np.float64), fS, fT))
    mk = lambda cx: [(cx.cloud_from_features(cfg, kS, fS, bbx), cx.cloud_from_features(cfg, kT, fT, bbx)) for kS, kT, fS, fT in feats]  # noqa: E731
    hc, hs = mk(cpt), mk(std)
    cpt.kernel_timing(True)
    got = cpt.register_clouds(cfg, hc)
    stats = cpt.pair_loop_stats()
    _, launches = cpt.kernel_time("pair_loop_dispatch")
    cpt.kernel_timing(False)
    assert stats["launches"] == 1 and launches == 1, (stats, launches)  # one batch, one class, one dispatch
    alone = [std.register_clouds(cfg, [h])[0] for h in hs]
    assert max(a.iterations for a in alone) > 1
    for a, b, sh in zip(alone, got, shapes):
        assert a.iterations == b.iterations and a.converged == b.converged and list(a.Rt) == list(b.Rt), sh
    for a, b in hc + hs:
        a.close()
        b.close()
    cpt.close()
    std.close()
