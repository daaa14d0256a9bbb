"""Generalized ICP that applies the trimmed rejector: ghicp_gicp_trimmed_from and its batched form ghicp_gicp_clouds_trimmed (Context.gicp /
Context.gicp_clouds with trim_ratio, CRegistration::trimmed_gicp_reg) against the CPU restatement with an actual sort
(tests/cpp/gicp_trimmed_cpu.cpp), with the assertions of test_gpu_gicp.py's _compare: index work exact, the pose within the project's
5e-7 / 5e-6.  Then the shapes at which the new kernels can go wrong -- nothing to trim, exact ties at the threshold, the block and select-grid
edges, too few kept, rejection before the trim -- and the batch against the per-pair call, bit for bit.

Few outer iterations and inner steps wherever the case allows: on the host interpreter every inner step is 512 workgroups."""
import os
import subprocess

import numpy as np
import pytest

import gicp_restatement as G
import gicp_trimmed_restatement as GT
from conftest import rot_err, trans_err
from test_gicp_trimmed_cpu import CLEAN_SHARE, STAT_KEYS, contaminated_pair
from test_gpu_gicp import ROOT, _compare, _dump
from test_gpu_refine import displaced, lattice
from test_icp_cpu import small_pair

pytestmark = pytest.mark.gpu

K, INNER = 10, 4  # of the edge cases (the parity cases run gicp_reg's own 20 / 20)


def f32(M):
    return np.ascontiguousarray(M, np.float64).astype(np.float32)


def both(api, *a, **kw):
    """The same parameters for the library and for the restatement."""
    pg, po = api.gicp_params(*a, **kw), G.params(*a, **kw)
    return pg, po


def nv_of(ratio, count):
    return min(count, int(np.floor(np.float32(ratio) * np.float32(count))))


def same_single(a, b):
    for k in STAT_KEYS:
        assert a[k] == b[k], (k, a[k], b[k])
    np.testing.assert_array_equal(a["T"], b["T"])
    np.testing.assert_array_equal(a["transformed"].cpu().numpy(), b["transformed"].cpu().numpy())


def close_to_restatement(rg, ro, label):
    Tg, To = rg["T"].astype(np.float64), ro["T"].astype(np.float64)
    print("%s: iterations %d reason %d kept %d | rot %.3g trans %.3g vs CPU" % (label, rg["iterations"], rg["reason"], rg["correspondences"],
                                                                              rot_err(Tg, To), trans_err(Tg, To)))
    assert rg["done"] == ro["done"] == 1
    assert (rg["iterations"], rg["converged"], rg["reason"]) == (ro["iterations"], ro["converged"], ro["reason"])
    assert rg["correspondences"] == ro["correspondences"]
    assert rot_err(Tg, To) <= 5e-7 and trans_err(Tg, To) <= 5e-6


@pytest.fixture(scope="module")
def small(synth):
    return small_pair(synth)


@pytest.fixture(scope="module")
def contaminated(synth):
    return contaminated_pair(synth)


# ------------------------------------------------------------------------------------------------ 1. parity against the restatement
@pytest.mark.parametrize("ratio", [0.9, 0.5])
def test_small_pair_matches_cpu(ctx, api, oracle, small, ratio):
    src, tgt, _ = small
    pg, po = both(api, 12, False, False, 0.2, 0.1, 20)
    ro = GT.gicp_trimmed(oracle, src, tgt, po, ratio)
    rg = ctx.gicp(src, tgt, pg, trim_ratio=ratio)
    _compare(rg, ro, None, "small pair ratio %.1f" % ratio)
    assert rg["correspondences"] == nv_of(ratio, len(src)) < len(src)


def test_ratio_zero_takes_the_estimate_of_the_gate(ctx, api, oracle, small):
    src, tgt, _ = small
    pg, po = both(api, 6, False, True, 0.2, 0.1, 20)
    ro = GT.gicp_trimmed(oracle, src, tgt, po, 0.0)
    rg = ctx.gicp(src, tgt, pg, trim_ratio=0.0)
    _compare(rg, ro, None, "small pair, ratio = overlap %.4f" % rg["overlap"])
    assert 0.1 < rg["overlap"] < 1.0 and rg["correspondences"] == nv_of(rg["overlap"], len(src)) < len(src)
    assert ctx.gicp(src, tgt, api.gicp_params(1, False, True, 0.2, 0.1, K, 1e6, 1))["correspondences"] == len(src)  # untrimmed: the gate alone


def test_contaminated_pair_matches_cpu_and_the_truth(ctx, api, oracle, contaminated):
    src, tgt, gt = contaminated
    pg, po = both(api, 40, False, False, 0.2, 0.1, 20)
    ro = GT.gicp_trimmed(oracle, src, tgt, po, CLEAN_SHARE)
    rg = ctx.gicp(src, tgt, pg, trim_ratio=CLEAN_SHARE)
    _compare(rg, ro, gt, "contaminated pair")  # gt: 2e-3 rotation, 0.02 m translation
    again = ctx.gicp(src, tgt, pg, trim_ratio=CLEAN_SHARE)  # fixed reduction order, integer select: bit-identical
    same_single(again, rg)


# ------------------------------------------------------------------------------------------------ 2. nothing to trim
def test_ratio_one_is_the_untrimmed_call_bit_for_bit(ctx, api, small):
    src, tgt, gt = small
    guess = f32(displaced(gt, 0.5, (0.08, -0.05, 0.02)))
    prm = api.gicp_params(2, False, False, 0.2, 0.1, K, 1e6, INNER)
    same_single(ctx.gicp(src, tgt, prm, trim_ratio=1.0), ctx.gicp(src, tgt, prm))
    prm = api.gicp_params(2, False, True, 0.2, 0.1, K, 1e6, INNER)  # with the gate, which sees the guess-moved source
    same_single(ctx.gicp(src, tgt, prm, guess=guess, trim_ratio=1.0), ctx.gicp(src, tgt, prm, guess=guess))


def test_an_estimate_above_one_keeps_everything(ctx, api, small):
    _, tgt, _ = small
    src = tgt[:500].copy()  # every point has a neighbour at distance 0: calOverlap = (0.01 + n) / n
    prm = api.gicp_params(3, False, True, 0.2, 0.1, K, 1e6, INNER)
    r = ctx.gicp(src, tgt, prm, trim_ratio=0.0)
    assert r["overlap"] > 1.0 and r["correspondences"] == 500  # floor(ratio * count) >= count
    same_single(r, ctx.gicp(src, tgt, prm))


# ------------------------------------------------------------------------------------------------ 3. exact ties at the threshold
NA, NB = 96, 104


def tie_pair():
    """Target: the 7 x 7 x 7 integer lattice.  Source: NA lattice nodes + (0.25, 0, 0) (d^2 = 0.0625 exactly) and NB nodes + (0, 0.375, 0)
    (d^2 = 0.140625 exactly), in mixed order: under the identity the keys are two runs of equal distances, split by the source index alone."""
    tgt = np.stack(np.meshgrid(*([np.arange(7)] * 3), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    rng = np.random.default_rng(7)
    nodes = tgt[rng.permutation(len(tgt))[: NA + NB]]
    off = np.zeros((NA + NB, 3), np.float32)
    off[:NA] = (0.25, 0.0, 0.0)
    off[NA:] = (0.0, 0.375, 0.0)
    order = rng.permutation(NA + NB)
    return (nodes + off)[order], tgt


# rank nv: inside the first run (index passes of the smaller distance); at the first tie of the second run (the istar == 0 shortcut: nothing of
# it is kept); in its middle (index passes); at its last tie (all but one kept)
@pytest.mark.parametrize("nv", [40, NA, NA + 37, NA + NB - 1])
def test_exact_ties_at_the_threshold(ctx, api, oracle, nv):
    src, tgt = tie_pair()
    d2 = ((src[:, None, :] - tgt[None, :, :]) ** 2).sum(-1).min(1)
    assert sorted(set(d2.tolist())) == [0.0625, 0.140625] and (d2 == 0.0625).sum() == NA
    ratio = float(np.float32((nv + 0.5) / (NA + NB)))
    assert nv_of(ratio, NA + NB) == nv
    pg, po = both(api, 1, False, False, 0.2, 0.1, 6)
    ro = GT.gicp_trimmed(oracle, src, tgt, po, ratio)
    rg = ctx.gicp(src, tgt, pg, trim_ratio=ratio)
    assert ro["correspondences"] == nv and ro["iterations"] == 1
    close_to_restatement(rg, ro, "ties, nv = %d" % nv)


# ------------------------------------------------------------------------------------------------ 4. block and select-grid edges
@pytest.mark.parametrize("n", [4, 255, 256, 257, 2048, 2049])  # one block of 256 and its neighbours; cdiv(ns, 2048) select blocks
def test_source_sizes_at_the_block_edges(ctx, api, oracle, small, n):
    src, tgt, _ = small
    pg, po = both(api, 2, False, False, 0.2, 0.1, K, 1e6, INNER)
    for ratio in (0.7,) + ((1.0,) if n == 4 else ()):
        ro = GT.gicp_trimmed(oracle, src[:n], tgt, po, ratio)
        rg = ctx.gicp(src[:n], tgt, pg, trim_ratio=ratio)
        close_to_restatement(rg, ro, "ns = %d ratio %.1f" % (n, ratio))
        assert rg["correspondences"] == nv_of(ratio, n)
        assert (rg["reason"] == 5) == (nv_of(ratio, n) < 4)


@pytest.mark.parametrize("nv", [3, 0])
def test_fewer_than_four_kept_return_the_guess(ctx, api, small, nv):
    src, tgt, gt = small
    g32 = f32(displaced(gt, 0.5, (0.08, -0.05, 0.02)))
    ratio = float(np.float32((nv + 0.5) / len(src)))
    assert nv_of(ratio, len(src)) == nv
    r = ctx.gicp(src, tgt, api.gicp_params(5, False, False, 0.2, 0.1, K, 1e6, INNER), guess=g32, trim_ratio=ratio)
    assert (r["done"], r["converged"], r["reason"], r["iterations"], r["correspondences"]) == (1, 0, 5, 0, nv)
    np.testing.assert_array_equal(r["T"], g32)
    np.testing.assert_array_equal(r["transformed"].cpu().numpy(), ctx.transform_cloud_f32(src, g32).cpu().numpy())


def test_rejection_by_distance_comes_before_the_trim(ctx, api, oracle, small):
    src, tgt, gt = small
    guess32 = f32(displaced(gt, 3.0, (0.2, -0.15, 0.05)))
    max_dist, ratio = 0.15, 0.6
    covS, covT = G.covariances(oracle, src, K), G.covariances(oracle, tgt, K)
    survivors = len(G.correspondences(oracle, src, tgt, covS, covT, guess32, max_dist)[0])
    assert 4 < survivors < len(src)
    pg, po = both(api, 1, False, False, 0.2, 0.1, K, max_dist, INNER)
    rg = ctx.gicp(src, tgt, pg, guess=guess32, trim_ratio=ratio)
    ro = GT.gicp_trimmed(oracle, src, tgt, po, ratio, guess=guess32)
    close_to_restatement(rg, ro, "%d of %d within %.2f m" % (survivors, len(src), max_dist))
    assert rg["correspondences"] == nv_of(ratio, survivors)  # `count` is the survivors, not the source


def test_bad_ratios_are_argument_errors(ctx, api, small):
    src, tgt, _ = small
    for gate in (False, True):
        prm = api.gicp_params(3, False, gate, 0.2, 0.1, K, 1e6, INNER)
        for bad in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(api.GhicpError):
                ctx.gicp(src[:300], tgt, prm, trim_ratio=bad)
    with pytest.raises(api.GhicpError):  # the estimate of a gate that is switched off
        ctx.gicp(src[:300], tgt, api.gicp_params(3, False, False, 0.2, 0.1, K, 1e6, INNER), trim_ratio=0.0)
    assert ctx.gicp(src[:300], tgt, prm, trim_ratio=0.5)["done"] == 1  # and the context is as good as before


# ------------------------------------------------------------------------------------------------ 5. the batch = the per-pair call
TEPS, REPS = 1e-4, 1e-4  # as in test_gpu_gicp_clouds.py: the pairs that start near the truth stop before max_iter
B_ITER = 6


def bparams(api, gate):
    p = api.gicp_params(B_ITER, False, gate, 0.3, 0.1, K, 0.4, INNER)
    p.transformation_epsilon, p.rotation_epsilon = TEPS, REPS
    return p


class Batch:
    """Sources of different sizes over one lattice target.  A different share of every source lies 9 m to the side, beyond the target (its
    lattice spans 7 m): no correspondence within 0.4 m there, and an overlap estimate of its own for every pair.  The pairs: a large source from a
    displaced pose; smaller ones (a second block of 256 just begun; less than one block); a source of 2 points (fewer than 4 kept); a pair the
    gate refuses; the large source again from the pose it was made with, which converges before the displaced one."""

    def __init__(self, ctx, api):
        self.ctx, self.api = ctx, api
        cfg = api.pair_config(api.FEATURE_NONE, api.CORR_NN, dof=6, voxel=0.2, max_iter=10)
        tgt = lattice(3000, 1)
        made = displaced(np.eye(4), 0.3, (0.03, -0.02, 0.01))
        inv = np.linalg.inv(made)
        rng = np.random.default_rng(4)
        raws = []
        for n, aside in ((2500, 0.2), (700, 0.3), (257, 0.1), (100, 0.25), (2, 0.0)):
            x = tgt[rng.permutation(len(tgt))[:n]].astype(np.float64)
            x[: int(aside * n), 0] += 9.0
            raws.append((x @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
        self.clouds = [ctx.cloud_create(cfg, x) for x in raws + [tgt]]
        for c in self.clouds:
            c.prepare_gicp(K, 1e-3)
        self.ms = [int(c.info().m) for c in self.clouds]
        self.ds = [c.download()["ds"] for c in self.clouds]
        off = displaced(made, 0.5, (0.05, -0.03, 0.02))
        far = displaced(made, 0.0, (900.0, 0.0, 0.0))
        self.pairs = [(0, off), (4, off), (1, off), (1, far), (2, off), (0, made), (3, off)]
        self._ref = {}

    def per_pair(self, gate, ratio, p):
        i, init = self.pairs[p]
        if (gate, ratio, p) not in self._ref:
            self._ref[gate, ratio, p] = self.ctx.gicp(self.ds[i], self.ds[5], bparams(self.api, gate), want_transformed=False, guess=f32(init),
                                                      trim_ratio=ratio)
        return self._ref[gate, ratio, p]

    def batch(self, gate, ratio, max_concurrent=0):
        return self.ctx.gicp_clouds(bparams(self.api, gate), [(self.clouds[i], self.clouds[5]) for i, _ in self.pairs],
                                    np.stack([init for _, init in self.pairs]), max_concurrent, trim_ratio=ratio)


@pytest.fixture(scope="module")
def batch(ctx, api):
    b = Batch(ctx, api)
    yield b
    for c in b.clouds:
        c.close()


def assert_batch_is_per_pair(batch, gate, ratio, got):
    assert len(got) == len(batch.pairs)
    for p, g in enumerate(got):
        r = batch.per_pair(gate, ratio, p)
        for k in STAT_KEYS:
            assert g[k] == r[k], "pair %d: %s = %r, the per-pair call gives %r" % (p, k, g[k], r[k])
        np.testing.assert_array_equal(g["T"], r["T"] if r["done"] else f32(batch.pairs[p][1]))


def test_batch_with_per_pair_ratios_is_the_per_pair_call(batch):
    assert batch.ms[0] > 2048 and 256 < batch.ms[2] <= 258 and 4 <= batch.ms[3] <= 256 and batch.ms[4] < 4, batch.ms
    got = batch.batch(True, 0.0)
    print("iterations", [g["iterations"] for g in got], "reasons", [g["reason"] for g in got], "overlap", [round(g["overlap"], 4) for g in got],
          "kept", [g["correspondences"] for g in got])
    assert_batch_is_per_pair(batch, True, 0.0, got)
    assert got[3]["done"] == 0 and got[3]["iterations"] == 0 and got[3]["overlap"] < 0.1  # refused
    assert (got[1]["done"], got[1]["reason"], got[1]["iterations"]) == (1, 5, 0) and got[1]["correspondences"] < 4
    ran = [0, 2, 4, 5, 6]
    assert len(set(round(got[p]["overlap"], 3) for p in ran if p != 5)) == 4  # a ratio of its own for every source
    for p in ran:  # trimmed: fewer kept than the source has points, floor(overlap * survivors) of them
        assert 4 <= got[p]["correspondences"] < batch.ms[batch.pairs[p][0]] and got[p]["iterations"] >= 1
    assert got[5]["iterations"] < got[0]["iterations"], "the pair at its truth no longer stops first: the fixture does not test the freeze"
    two = batch.batch(True, 0.0, 4)  # chunks of 4 and 3 pairs
    for a, b in zip(two, got):
        for k in STAT_KEYS:
            assert a[k] == b[k], k
        np.testing.assert_array_equal(a["T"], b["T"])


def test_batch_with_one_ratio_is_the_per_pair_call(batch):
    ratio = 0.04  # of the 75 points of the smallest source within 0.4 m: 3 kept -- it stops while the others go on
    got = batch.batch(False, ratio)
    print("iterations", [g["iterations"] for g in got], "reasons", [g["reason"] for g in got], "kept", [g["correspondences"] for g in got])
    assert_batch_is_per_pair(batch, False, ratio, got)
    assert all(g["done"] == 1 for g in got)  # no gate
    assert (got[6]["reason"], got[6]["iterations"]) == (5, 0) and got[6]["correspondences"] < 4
    assert got[0]["iterations"] >= 1 and got[0]["correspondences"] >= 4
    with pytest.raises(batch.api.GhicpError):
        batch.batch(False, 0.0)
    with pytest.raises(batch.api.GhicpError):
        batch.batch(True, 1.25)


# ------------------------------------------------------------------------------------------------ 6. the drop-in
def test_trimmed_gicp_dropin_on_gpu(ctx, oracle, small, tmp_path):
    """tests/cpp/test_gicp_trimmed_dropin.cpp: CRegistration<pcl::PointXYZ>::trimmed_gicp_reg with gicp_reg's arguments."""
    exe = tmp_path / "test_gicp_trimmed_dropin"
    libdir, libname = os.path.join(ROOT, "gh-icp_amd"), "ghicp_hip"
    if getattr(ctx, "simulated", False):  # GHICP_SIM=1: the same C ABI from tests/hipsim
        libdir, libname = os.path.join(ROOT, "tests", "hipsim", "_build"), "ghicp_sim"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_gicp_trimmed_dropin.cpp"),
                           "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-o", str(exe)])
    src, tgt, _ = small
    _dump(tmp_path / "S.bin", src)
    _dump(tmp_path / "T.bin", tgt)
    out = subprocess.run([str(exe), str(tmp_path / "S.bin"), str(tmp_path / "T.bin")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l.split() for l in out.stdout.splitlines() if l.split() and l.split()[0] in ("RESULT", "ROW", "OUT")]
    head = next(l for l in lines if l[0] == "RESULT")
    ok, iters, reason, nout, kept = (int(v) for v in head[1:6])
    ro = GT.gicp_trimmed(oracle, src, tgt, G.params(40, False, True, 0.3, 0.1, 20), 0.0)
    assert ok == 1 and nout == len(src) and (iters, reason, kept) == (ro["iterations"], ro["reason"], ro["correspondences"])
    assert kept == nv_of(ro["overlap"], len(src)) < len(src)
    Tg = np.array([[float(v) for v in l[1:]] for l in lines if l[0] == "ROW"])
    To = ro["T"].astype(np.float64)
    assert rot_err(Tg, To) <= 5e-7 and trans_err(Tg, To) <= 5e-6
    outc = np.array([[float(v) for v in l[1:]] for l in lines if l[0] == "OUT"], np.float32)
    np.testing.assert_allclose(outc, ro["transformed"], atol=2e-4)
