"""The CPU restatement of the generalized ICP that applies the trimmed rejector (tests/cpp/gicp_trimmed_cpu.cpp) on its own:
with nothing to trim it is the restatement of gicp_reg, and on a pair whose source is partly NOT in the target it ends at the truth where the
untrimmed loop does not.  tests/test_gpu_gicp_trimmed.py holds the GPU to this restatement."""
import numpy as np
import pytest

import gicp_restatement as G
import gicp_trimmed_restatement as GT
from conftest import rot_err, trans_err
from test_icp_cpu import small_pair

STAT_KEYS = ("done", "iterations", "converged", "reason", "correspondences", "overlap", "mse", "fitness")

# The contaminated pair: the first quarter of small_pair's source (its rows are in random order) is moved rigidly by 0.8 m / 0.5 m in the
# ground plane, beside the surfaces it was scanned from: the nearest target point of such a point is a wrong correspondence.  Found on the CPU
# restatement alone (40 iterations, k = 20, the reference's epsilons): untrimmed, GICP ends 3.2e-3 / 0.115 m from the truth; keeping the clean
# share, 2.7e-5 / 1e-4 m.
DISPLACED_SHARE = 0.25
DISPLACED_BY = (0.8, 0.5, 0.0)
CLEAN_SHARE = 1.0 - DISPLACED_SHARE


def contaminated_pair(synth):
    src, tgt, gt = small_pair(synth)
    src = src.copy()
    src[: int(DISPLACED_SHARE * len(src))] += np.array(DISPLACED_BY, np.float32)
    return src, tgt, gt


@pytest.mark.parametrize("gate", [False, True])
def test_ratio_one_is_the_restatement_of_gicp_reg(oracle, synth, gate):
    src, tgt, _ = small_pair(synth)
    prm = G.params(40, False, gate, 0.2, 0.1, 20)
    a, b = G.gicp(oracle, src, tgt, prm), GT.gicp_trimmed(oracle, src, tgt, prm, 1.0)
    for k in STAT_KEYS:
        assert a[k] == b[k], k
    assert a["done"] == 1 and a["correspondences"] == len(src)
    np.testing.assert_array_equal(a["T"], b["T"])
    np.testing.assert_array_equal(a["transformed"], b["transformed"])


def test_trimming_recovers_the_truth_on_a_contaminated_pair(oracle, synth):
    src, tgt, gt = contaminated_pair(synth)
    prm = G.params(40, False, False, 0.2, 0.1, 20)
    plain = G.gicp(oracle, src, tgt, prm)
    trimmed = GT.gicp_trimmed(oracle, src, tgt, prm, CLEAN_SHARE)
    Tp, Tt = plain["T"].astype(np.float64), trimmed["T"].astype(np.float64)
    print("untrimmed: rot %.3g trans %.3g (%d iterations) | trimmed to %.2f: rot %.3g trans %.3g (%d iterations, %d kept)" % (
        rot_err(Tp, gt), trans_err(Tp, gt), plain["iterations"], CLEAN_SHARE, rot_err(Tt, gt), trans_err(Tt, gt), trimmed["iterations"],
        trimmed["correspondences"]))
    assert trimmed["done"] == 1 and trimmed["converged"] == 1
    assert trimmed["correspondences"] == int(np.floor(np.float32(CLEAN_SHARE) * np.float32(len(src))))
    assert rot_err(Tt, gt) < 2e-3 and trans_err(Tt, gt) < 0.02  # the ground-truth bounds of test_gpu_gicp.py
    assert rot_err(Tt, gt) < rot_err(Tp, gt) and trans_err(Tt, gt) < trans_err(Tp, gt)
