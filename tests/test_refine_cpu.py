"""CPU checks of the batched fine registration's interface (include/ghicp_c.h, gh-icp_amd/api.py) and of its one host-side helper, the
chunk planner (gh-icp_amd/csrc/refine_plan.h)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ghicp_cloud_prepare_refine", "ghicp_refine_clouds")


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "ghicp_c.h")).read()
    assert re.search(r"int ghicp_cloud_prepare_refine\(ghicp_cloud\* cloud, int32_t covariance_k\);", h)
    m = re.search(r"int ghicp_refine_clouds\(([^;]*)\);", h)
    assert m
    args = " ".join(m.group(1).split())
    for piece in ("ghicp_ctx* ctx", "const ghicp_icp_params* params", "int32_t n_pairs", "const ghicp_cloud* const* S", "const ghicp_cloud* const* T",
                  "const double* Rt_init", "int32_t max_concurrent", "ghicp_refine_result* out"):
        assert piece in args, piece
    assert "typedef struct ghicp_refine_result" in h
    assert "use_reciprocal != 0" in h  # what the batch does not cover is said where callers read it


def test_api_lists_the_entry_points(api):
    for name in NAMES:
        assert name in api.EXPORTS
    assert callable(api.Cloud.prepare_refine) and callable(api.Context.refine_clouds)
    lib = os.path.join(ROOT, "gh-icp_amd", "libghicp_hip.so")
    if os.path.exists(lib):  # the argument checks come before any device work
        L = api.load()
        L.ghicp_cloud_prepare_refine.restype = ctypes.c_int
        assert L.ghicp_cloud_prepare_refine(ctypes.c_void_p(0), 0) == 1  # GHICP_ERR_ARG on a NULL handle
        L.ghicp_refine_clouds.restype = ctypes.c_int
        assert L.ghicp_refine_clouds(*([ctypes.c_void_p(0)] * 3), 0, *([ctypes.c_void_p(0)] * 3), 0, ctypes.c_void_p(0)) == 1


def test_ctypes_mirror_has_the_layout_of_the_c_struct(api, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ghicp_c.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(ghicp_refine_result), offsetof(ghicp_refine_result, T_icp),\n'
                   '  offsetof(ghicp_refine_result, Rt_refined), offsetof(ghicp_refine_result, stats), sizeof(ghicp_icp_stats)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    size, o_t, o_rt, o_st, size_st = (int(v) for v in subprocess.check_output([exe]).split())
    R = api.RefineResult
    assert (ctypes.sizeof(R), R.T_icp.offset, R.Rt_refined.offset, R.stats.offset) == (size, o_t, o_rt, o_st)
    assert ctypes.sizeof(api.IcpStats) == size_st


def test_chunk_planner_under_sanitizers(tmp_path):
    """Chunk sizes 0 / 1 / n / n + 1, empty pair lists, tight budgets, more pairs than one chunk may hold: a stand-alone program, built with
    AddressSanitizer and UBSan."""
    exe = str(tmp_path / "test_refine_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "gh-icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_refine_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "refine_plan ok" in r.stdout, r.stdout + r.stderr
