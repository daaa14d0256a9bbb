"""GPU parity of generalized ICP (CRegistration::gicp_reg, reference src/common_reg.cpp:216-284; ghicp_gicp / ghicp_gicp_covariances)
against the CPU restatement (tests/cpp/gicp_cpu.cpp).  Index work (correspondence counts, iteration counts, convergence
reasons) is exact; the covariances are bit-exact up to the N2 allowance; the 4x4 is held to the north-star tolerance (1e-4 rotation,
1e-3 m translation) and, more tightly, to what the shared contract delivers."""
import os
import struct
import subprocess

import numpy as np
import pytest

import gicp_restatement as G
from conftest import rot_err, trans_err
from test_gicp_cpu import scan_pair
from test_icp_cpu import small_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cov_parity(ctx, oracle, xyz, k, label):
    cg = ctx.gicp_covariances(xyz, k).cpu().numpy()
    co = G.covariances(oracle, xyz, k)
    rows = np.flatnonzero((cg != co).any(axis=1))
    diff = float(np.abs(cg - co).max())
    print("covariances %s k=%d: %d of %d rows differ, largest difference %.3g" % (label, k, rows.size, len(xyz), diff))
    assert rows.size <= 3, (label, k, rows[:10])  # N2: a scatter entry straddling a rounding boundary
    return cg


def test_gicp_covariances_bit_exact(ctx, api, oracle, synth):
    src, tgt, _ = small_pair(synth)
    for k in (1, 20):
        _cov_parity(ctx, oracle, src, k, "small source")
        _cov_parity(ctx, oracle, tgt, k, "small target")
    p = synth.tls_pair(120_000, config_id=2)
    ds = p.target[oracle.voxel_filter(p.target, 0.1)][:, :3]
    _cov_parity(ctx, oracle, ds, 20, "cfg2 0.1 m voxel")
    c1 = ctx.gicp_covariances(src, 1).cpu().numpy()  # k = 1: the query alone, zero scatter -> diag(eps, 1, 1)
    np.testing.assert_array_equal(c1, np.tile([1e-3, 0, 0, 1, 0, 1], (len(src), 1)))
    with pytest.raises(api.GhicpError):
        ctx.gicp_covariances(src, 21)


def _compare(rg, ro, gt=None, label=""):
    Tg, To = rg["T"].astype(np.float64), ro["T"].astype(np.float64)
    print("%s: iterations %d reason %d correspondences %d | rot %.3g trans %.3g vs CPU | fitness %.9g / %.9g" % (
        label, rg["iterations"], rg["reason"], rg["correspondences"], rot_err(Tg, To), trans_err(Tg, To), rg["fitness"], ro["fitness"]))
    assert rg["done"] == ro["done"] == 1
    assert rg["overlap"] == ro["overlap"]
    assert (rg["iterations"], rg["converged"], rg["reason"]) == (ro["iterations"], ro["converged"], ro["reason"])
    assert rg["correspondences"] == ro["correspondences"]
    assert rot_err(Tg, To) <= 1e-4 and trans_err(Tg, To) <= 1e-3
    # what the shared contract delivers on the MI355X: <= 6.5e-8 rotation, 0 m translation (identical float translations)
    assert rot_err(Tg, To) <= 5e-7 and trans_err(Tg, To) <= 5e-6
    if gt is not None:
        assert rot_err(Tg, gt) < 2e-3 and trans_err(Tg, gt) < 0.02
    np.testing.assert_allclose(rg["transformed"].cpu().numpy(), ro["transformed"], atol=2e-4)
    np.testing.assert_allclose(rg["fitness"], ro["fitness"], rtol=1e-3)


@pytest.mark.parametrize("trimmed", [False, True])
def test_gicp_matches_cpu(ctx, api, oracle, synth, trimmed):
    src, tgt, gt = small_pair(synth)
    ro = G.gicp(oracle, src, tgt, G.params(40, False, trimmed, 0.2, 0.1, 20))
    res = {}
    for reciprocal in (False, True):
        rg = ctx.gicp(src, tgt, api.gicp_params(40, reciprocal, trimmed, 0.2, 0.1, 20))
        _compare(rg, ro, gt, "small pair trimmed=%d reciprocal=%d" % (trimmed, reciprocal))
        res[reciprocal] = rg
    # GICP does its own correspondence search: the reciprocal flag changes nothing
    np.testing.assert_array_equal(res[False]["T"], res[True]["T"])
    np.testing.assert_array_equal(res[False]["transformed"].cpu().numpy(), res[True]["transformed"].cpu().numpy())


def test_gicp_scan_pair(ctx, api, oracle, synth):
    S0, T, coarse, truth = scan_pair(oracle, synth)
    ro = G.gicp(oracle, S0, T, G.params(30, False, True, 0.3, 0.1, 20))
    rg = ctx.gicp(S0, T, api.gicp_params(30, False, True, 0.3, 0.1, 20))
    _compare(rg, ro, None, "scan pair")
    total = rg["T"].astype(np.float64) @ coarse
    assert rot_err(total, truth) < 5e-3 and trans_err(total, truth) < 0.05  # pulls the estimate back to the truth
    again = ctx.gicp(S0, T, api.gicp_params(30, False, True, 0.3, 0.1, 20))  # sums reduced in a fixed order: bit-identical
    np.testing.assert_array_equal(again["T"], rg["T"])
    np.testing.assert_array_equal(again["transformed"].cpu().numpy(), rg["transformed"].cpu().numpy())
    assert again["fitness"] == rg["fitness"] and again["mse"] == rg["mse"]


def test_gicp_edge_cases(ctx, api, oracle, synth):
    src, tgt, _ = small_pair(synth, n=3000)
    r = ctx.gicp(src + np.float32(500.0), tgt, api.gicp_params(10, False, True, 0.2, 0.5))
    assert r["done"] == 0 and r["overlap"] < 0.01 and not r["T"].any()  # refused: T untouched (reference returns false)
    r = ctx.gicp(src, tgt, api.gicp_params(2))
    assert r["iterations"] == 2 and r["reason"] == 1 and r["converged"] == 1
    for n in (1, 3):  # ns < 4: PCL throws before the first step
        r = ctx.gicp(src[:n], tgt, api.gicp_params(5))
        assert r["done"] == 1 and r["converged"] == 0 and r["reason"] == 5 and r["iterations"] == 0 and r["correspondences"] == n
        np.testing.assert_array_equal(r["T"], np.eye(4, dtype=np.float32))
    r = ctx.gicp(src, tgt, api.gicp_params(5, max_correspondence_distance=1e-4))
    ro = G.gicp(oracle, src, tgt, G.params(5, max_correspondence_distance=1e-4))
    assert (r["reason"], r["iterations"], r["correspondences"]) == (ro["reason"], ro["iterations"], ro["correspondences"]) and r["reason"] == 5
    r = ctx.gicp(src, np.zeros((0, 3), np.float32), api.gicp_params(5))  # empty target
    assert r["done"] == 1 and r["reason"] == 5 and r["iterations"] == 0
    np.testing.assert_array_equal(r["transformed"].cpu().numpy(), src)
    r = ctx.gicp(np.zeros((0, 3), np.float32), tgt, api.gicp_params(5))
    assert r["reason"] == 5 and r["iterations"] == 0
    for bad in (dict(covariance_k=21), dict(covariance_k=0), dict(max_inner_iter=0)):
        with pytest.raises(api.GhicpError):
            ctx.gicp(src, tgt, api.gicp_params(5, **bad))


def test_gicp_leaves_icp_unchanged(ctx, api, synth):
    """ghicp_gicp reuses the k-NN, grid and loop buffer slots of ghicp_icp: an ICP run after it is bit-identical to one before it."""
    src, tgt, _ = small_pair(synth, n=8000)
    prm = api.icp_params(30, False, True, api.ICP_POINT_TO_PLANE, 0.2, 0.1, 12)
    a = ctx.icp(src, tgt, prm)
    g = ctx.gicp(tgt, src, api.gicp_params(20, covariance_k=20))
    assert g["done"] == 1
    b = ctx.icp(src, tgt, prm)
    np.testing.assert_array_equal(a["T"], b["T"])
    np.testing.assert_array_equal(a["transformed"].cpu().numpy(), b["transformed"].cpu().numpy())
    assert (a["iterations"], a["reason"], a["correspondences"], a["mse"], a["fitness"]) == (b["iterations"], b["reason"], b["correspondences"], b["mse"], b["fitness"])


def _dump(path, pts):
    with open(path, "wb") as f:
        f.write(struct.pack("i", pts.shape[0]))
        f.write(np.ascontiguousarray(pts, np.float32).tobytes())


def test_gicp_dropin_on_gpu(ctx, oracle, synth, tmp_path):
    """tests/cpp/test_gicp_dropin.cpp: CRegistration<pcl::PointXYZ>::gicp_reg as a reference program calls it."""
    exe = tmp_path / "test_gicp_dropin"
    libdir, libname = os.path.join(ROOT, "gh-icp_amd"), "ghicp_hip"
    if getattr(ctx, "simulated", False):  # GHICP_SIM=1: the same C ABI from tests/hipsim
        libdir, libname = os.path.join(ROOT, "tests", "hipsim", "_build"), "ghicp_sim"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_gicp_dropin.cpp"),
                           "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-o", str(exe)])
    src, tgt, gt = small_pair(synth)
    _dump(tmp_path / "S.bin", src)
    _dump(tmp_path / "T.bin", tgt)
    out = subprocess.run([str(exe), str(tmp_path / "S.bin"), str(tmp_path / "T.bin")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "GICP done in" in out.stdout and "The fitness score of this registration is" in out.stdout
    lines = [l.split() for l in out.stdout.splitlines() if l.split() and l.split()[0] in ("RESULT", "ROW", "OUT")]
    head = next(l for l in lines if l[0] == "RESULT")
    ok, iters, reason, nout = (int(v) for v in head[1:5])
    ro = G.gicp(oracle, src, tgt, G.params(40, False, True, 0.3, 0.1, 20))
    assert ok == 1 and nout == len(src) and (iters, reason) == (ro["iterations"], ro["reason"])
    Tg = np.array([[float(v) for v in l[1:]] for l in lines if l[0] == "ROW"])
    To = ro["T"].astype(np.float64)
    assert rot_err(Tg, To) <= 1e-4 and trans_err(Tg, To) <= 1e-3
    assert rot_err(Tg, gt) < 2e-3 and trans_err(Tg, gt) < 0.02
    outc = np.array([[float(v) for v in l[1:]] for l in lines if l[0] == "OUT"], np.float32)
    np.testing.assert_allclose(outc, ro["transformed"], atol=2e-4)
