"""CPU checks of the interface of generalized ICP from an initial pose and over cached clouds (include/ghicp_c.h, gh-icp_amd/api.py) and
of the chunk planner with the batch's costs (gh-icp_amd/csrc/refine_plan.h)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ghicp_gicp_from", "ghicp_cloud_prepare_gicp", "ghicp_gicp_clouds")


def _args(h, name):
    m = re.search(r"int %s\(([^;]*)\);" % name, h)
    assert m, name
    return " ".join(re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S).split())


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "ghicp_c.h")).read()
    a = _args(h, "ghicp_gicp_from")
    for piece in ("ghicp_ctx* ctx", "const float* xyzS, int64_t ns, int strideS", "const float* xyzT, int64_t nt, int strideT",
                  "const ghicp_gicp_params* params, const float* guess16", "float* T16", "float* transformed", "ghicp_icp_stats* stats"):
        assert piece in a, piece
    assert a.index("guess16") < a.index("T16 ")  # the guess comes before the outputs
    assert _args(h, "ghicp_cloud_prepare_gicp") == "ghicp_cloud* cloud, int32_t covariance_k, double gicp_epsilon"
    a = _args(h, "ghicp_gicp_clouds")
    for piece in ("ghicp_ctx* ctx", "const ghicp_gicp_params* params", "int32_t n_pairs", "const ghicp_cloud* const* S", "const ghicp_cloud* const* T",
                  "const double* Rt_init", "int32_t max_concurrent", "ghicp_gicp_result* out"):
        assert piece in a, piece
    assert re.search(r"typedef struct ghicp_gicp_result \{\s*float T\[16\];[^}]*ghicp_icp_stats stats;[^}]*\} ghicp_gicp_result;", h)
    # the guess semantics are said where callers read them: covariances in the source's own frame, an extension of the reference's call
    assert "OWN frame" in h and "align without a guess" in h and "EXTENSION" in h


def test_api_lists_the_entry_points(api):
    for name in NAMES:
        assert name in api.EXPORTS
    assert callable(api.Cloud.prepare_gicp) and callable(api.Context.gicp_clouds)
    assert "guess" in api.Context.gicp.__code__.co_varnames
    lib = os.path.join(ROOT, "gh-icp_amd", "libghicp_hip.so")
    if os.path.exists(lib):  # the argument checks come before any device work
        L = api.load()
        null = ctypes.c_void_p(0)
        L.ghicp_cloud_prepare_gicp.restype = ctypes.c_int
        assert L.ghicp_cloud_prepare_gicp(null, 20, ctypes.c_double(1e-3)) == 1  # GHICP_ERR_ARG on a NULL handle
        L.ghicp_gicp_clouds.restype = ctypes.c_int
        assert L.ghicp_gicp_clouds(null, null, 0, null, null, null, 0, null) == 1
        L.ghicp_gicp_from.restype = ctypes.c_int
        assert L.ghicp_gicp_from(null, null, ctypes.c_int64(0), 3, null, ctypes.c_int64(0), 3, null, null, null, null, null) == 1


def test_ctypes_mirror_has_the_layout_of_the_c_struct(api, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ghicp_c.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(ghicp_gicp_result), offsetof(ghicp_gicp_result, T),\n'
                   '  offsetof(ghicp_gicp_result, stats), sizeof(ghicp_icp_stats)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    size, o_t, o_st, size_st = (int(v) for v in subprocess.check_output([exe]).split())
    R = api.GicpResult
    assert (ctypes.sizeof(R), R.T.offset, R.stats.offset) == (size, o_t, o_st)
    assert ctypes.sizeof(api.IcpStats) == size_st


def test_chunk_planner_with_the_gicp_costs_under_sanitizers(tmp_path):
    """The cases of test_refine_plan.cpp with the batch's costs (48 B more per point, no histograms per pair), and that the plan of
    ghicp_refine_clouds is unchanged: a stand-alone program, built with AddressSanitizer and UBSan."""
    exe = str(tmp_path / "test_gicp_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "gh-icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_gicp_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "gicp_plan ok" in r.stdout, r.stdout + r.stderr
