"""CPU checks of the generalized-ICP restatement (tests/cpp/gicp_cpu.cpp: CRegistration::gicp_reg, reference
src/common_reg.cpp:216-284, under the contract of DESIGN.md N8) against independent code -- scipy's KD-tree and numpy's eigh for
the covariances, central finite differences for the Gauss-Newton Jacobian -- and the ground truth of the ICP tests' inputs; plus the
drop-in header's gicp_reg compiled like a reference caller."""
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial import cKDTree

import gicp_restatement as G
from conftest import rot_err, trans_err
from test_icp_cpu import small_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scan_pair(oracle, synth):
    """The 120 k-hit TLS pair after the 0.2 m voxel filter, the source pushed 1 degree / 0.18 m off the truth
    (test_gpu_icp.py::test_icp_after_coarse_registration_of_a_scan_pair).  Returns (source, target, coarse, truth)."""
    pair = synth.tls_pair(120_000)
    S = pair.source[oracle.voxel_filter(pair.source, 0.2)][:, :3]
    T = pair.target[oracle.voxel_filter(pair.target, 0.2)][:, :3]
    a = np.deg2rad(1.0)
    d = np.eye(4)
    d[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    d[:3, 3] = [0.15, -0.1, 0.03]
    coarse = d @ pair.gt
    return oracle.transform_cloud(S, coarse), T, coarse, pair.gt


def _sym(c6):
    return np.array([[c6[0], c6[1], c6[2]], [c6[1], c6[3], c6[4]], [c6[2], c6[4], c6[5]]])


def test_covariances_match_kdtree_and_eigh(oracle, synth):
    _, tgt, _ = small_pair(synth, n=3000)
    eps = 1e-3
    for k in (6, 20):
        cov = G.covariances(oracle, tgt, k, eps)
        _, nb = cKDTree(tgt.astype(np.float64)).query(tgt.astype(np.float64), k)
        bad = checked = 0
        for i in range(0, len(tgt), 7):
            P = tgt[nb[i]].astype(np.float64)
            w, v = np.linalg.eigh(np.cov(P.T, bias=True))
            if w[1] - w[0] < 1e-3 * w[2]:
                continue  # ambiguous smallest eigenvector
            checked += 1
            ref = v @ np.diag([eps, 1.0, 1.0]) @ v.T
            if np.abs(_sym(cov[i]) - ref).max() > 2e-3:
                bad += 1
        assert checked > 300 and bad <= 2
        # every covariance is symmetric positive definite with the spectrum (eps, 1, 1)
        w = np.linalg.eigvalsh(np.stack([_sym(c) for c in cov[::11]]))
        np.testing.assert_allclose(w, np.tile([eps, 1.0, 1.0], (w.shape[0], 1)), atol=1e-9)


def test_gauss_newton_jacobian_matches_finite_differences(oracle, synth):
    src, tgt, _ = small_pair(synth)
    covS, covT = G.covariances(oracle, src, 20), G.covariances(oracle, tgt, 20)
    si, tj, M = G.correspondences(oracle, src, tgt, covS, covT, np.eye(4, dtype=np.float32))
    assert len(si) == len(src)
    x = np.array([0.05, -0.02, 0.01, 0.004, -0.003, 0.02])
    H, g, e = G.gn_sums(oracle, src, tgt, si, tj, M, x)
    for p in range(6):
        h = 1e-6
        xp, xm = x.copy(), x.copy()
        xp[p] += h
        xm[p] -= h
        _, gp, ep = G.gn_sums(oracle, src, tgt, si, tj, M, xp)
        _, gm, em = G.gn_sums(oracle, src, tgt, si, tj, M, xm)
        # f = sum r^T M r: df/dx = 2 J^T M r; d(J^T M r)/dx ~ J^T M J (Gauss-Newton drops the second-derivative term, which
        # vanishes for the translation columns and is small for the rotation ones)
        fd = (ep - em) / (2 * h)
        assert abs(fd - 2 * g[p]) <= 1e-6 * max(1.0, abs(2 * g[p])) + 1e-7 * e, (p, fd, 2 * g[p])
        if p < 3:
            np.testing.assert_allclose((gp - gm) / (2 * h), H[:, p], rtol=1e-6, atol=1e-6 * np.abs(H).max())
    assert np.all(np.linalg.eigvalsh(H) > 0)


def test_restatement_recovers_the_ground_truth(oracle, synth):
    src, tgt, gt = small_pair(synth)
    r = G.gicp(oracle, src, tgt, G.params(40, covariance_k=20))
    assert r["done"] == 1 and r["converged"] == 1 and 1 <= r["iterations"] <= 40 and r["correspondences"] == len(src)
    T = r["T"].astype(np.float64)
    assert rot_err(T, gt) < 2e-3 and trans_err(T, gt) < 0.02
    np.testing.assert_allclose(r["transformed"], src @ r["T"][:3, :3].T + r["T"][:3, 3], atol=1e-4)
    assert r["fitness"] < 1e-3 and np.all((r["inner"] >= 1) & (r["inner"] <= 20))


def test_restatement_registers_a_scan_pair(oracle, synth):
    """The reference's own 1e6 correspondence distance (every nearest neighbour pulls) meets the bound on this pair."""
    S0, T, coarse, truth = scan_pair(oracle, synth)
    r = G.gicp(oracle, S0, T, G.params(30, trimmed=True, thre_dis=0.3, covariance_k=20))
    assert r["done"] == 1 and r["converged"] == 1
    total = r["T"].astype(np.float64) @ coarse
    assert rot_err(total, truth) < 5e-3 and trans_err(total, truth) < 0.05


def test_restatement_edge_cases(oracle, synth):
    src, tgt, _ = small_pair(synth, n=3000)
    r = G.gicp(oracle, src + np.float32(500.0), tgt, G.params(10, trimmed=True, thre_dis=0.2, min_overlap=0.5))
    assert r["done"] == 0 and r["overlap"] < 0.01  # refused
    r = G.gicp(oracle, src, tgt, G.params(2))
    assert r["iterations"] == 2 and r["reason"] == 1 and r["converged"] == 1  # ITERATIONS
    r = G.gicp(oracle, src[:3], tgt, G.params(5))
    assert r["done"] == 1 and r["converged"] == 0 and r["reason"] == 5 and r["iterations"] == 0  # fewer than 4 correspondences
    np.testing.assert_array_equal(r["T"], np.eye(4, dtype=np.float32))
    r = G.gicp(oracle, src, tgt, G.params(5, max_correspondence_distance=1e-4))  # nothing within 0.1 mm: PCL throws at once
    assert r["reason"] == 5 and r["iterations"] == 0 and r["correspondences"] < 4


def test_dropin_gicp_reg_compiles(tmp_path):
    """A reference program calling CRegistration<pcl::PointXYZ>::gicp_reg compiles and links against the drop-in headers."""
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_gicp_dropin.cpp"),
                           "-c", "-o", str(tmp_path / "test_gicp_dropin.o")])
    lib = os.path.join(ROOT, "gh-icp_amd", "libghicp_hip.so")
    if os.path.exists(lib):  # build() made the library: link like a caller does
        subprocess.check_call(["g++", str(tmp_path / "test_gicp_dropin.o"), "-L", os.path.dirname(lib), "-lghicp_hip", "-Wl,-rpath," + os.path.dirname(lib),
                               "-o", str(tmp_path / "test_gicp_dropin")])
