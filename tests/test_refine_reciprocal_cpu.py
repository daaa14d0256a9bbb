"""CPU checks of the interface of the batched fine registration with reciprocal correspondences (include/ghicp_c.h, gh-icp_amd/api.py) and
of its host-testable arithmetic: the grid plan and the cell-budget rule (gh-icp_amd/csrc/refine_recip_plan.h)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ghicp_refine_clouds_reciprocal"


def test_header_declares_the_entry_point():
    h = open(os.path.join(ROOT, "include", "ghicp_c.h")).read()
    m = re.search(r"int ghicp_refine_clouds_reciprocal\(([^;]*)\);", h)
    assert m
    args = " ".join(m.group(1).split())
    for piece in ("ghicp_ctx* ctx", "const ghicp_icp_params* params", "int32_t n_pairs", "const ghicp_cloud* const* S", "const ghicp_cloud* const* T",
                  "const double* Rt_init", "int32_t max_concurrent", "ghicp_refine_result* out"):
        assert piece in args, piece
    assert "use_reciprocal != 0" in h  # what ghicp_refine_clouds does not cover is still said where callers read it
    assert re.search(r"int ghicp_refine_clouds\(([^;]*)\);", h)


def test_api_lists_the_entry_point(api):
    assert NAME in api.EXPORTS
    assert callable(api.Context.refine_clouds_reciprocal) and callable(api.Context.refine_clouds)
    lib = os.path.join(ROOT, "gh-icp_amd", "libghicp_hip.so")
    if os.path.exists(lib):  # the argument checks come before any device work
        L = api.load()
        f = getattr(L, NAME)
        f.restype = ctypes.c_int
        assert f(*([ctypes.c_void_p(0)] * 3), 0, *([ctypes.c_void_p(0)] * 3), 0, ctypes.c_void_p(0)) == 1  # GHICP_ERR_ARG on a NULL context


def test_grid_plan_and_budget_rule_under_sanitizers(tmp_path):
    """Boxes of zero extent, one long axis, huge extents, tiny budgets; the ranges of a chunk: a stand-alone program, built with
    AddressSanitizer and UBSan."""
    exe = str(tmp_path / "test_refine_recip_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "gh-icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_refine_recip_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "refine_recip_plan ok" in r.stdout, r.stdout + r.stderr
