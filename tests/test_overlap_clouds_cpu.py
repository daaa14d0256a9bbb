"""CPU checks of the interface of the batched calOverlap over cached clouds (include/ghicp_c.h, gh-icp_amd/api.py) and of its chunk planner and
block -> pair search (gh-icp_amd/csrc/overlap_plan.h)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ghicp_cloud_prepare_overlap", "ghicp_overlap_clouds", "ghicp_overlap_matrix")


def _args(h, name):
    m = re.search(r"int %s\(([^;]*)\);" % name, h)
    assert m, name
    return " ".join(re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S).split())


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "ghicp_c.h")).read()
    assert _args(h, "ghicp_cloud_prepare_overlap") == "ghicp_cloud* cloud, float thre_dis"
    assert _args(h, "ghicp_overlap_clouds") == ("ghicp_ctx* ctx, float thre_dis, int32_t n_pairs, const ghicp_cloud* const* S, const ghicp_cloud* const* T, "
                                                "const double* Rt , int32_t max_concurrent, ghicp_overlap_result* out")
    assert _args(h, "ghicp_overlap_matrix") == ("ghicp_ctx* ctx, float thre_dis, int32_t n_clouds, const ghicp_cloud* const* clouds, const double* poses, "
                                                "float* out")
    assert re.search(r"typedef struct ghicp_overlap_result \{\s*int64_t hits;[^}]*int64_t n;[^}]*float ratio;[^}]*int32_t pad_;\s*\} ghicp_overlap_result;", h)
    assert h.index("ghicp_gicp_clouds(") < h.index("ghicp_cloud_prepare_overlap(") < h.index("ghicp_pairqueue_create(")  # after the batched GICP block
    # the arithmetic of the pair poses is written down where a caller (and test_gpu_overlap_clouds.py) reads it
    block = h[h.index("int ghicp_overlap_clouds("):h.index("int ghicp_overlap_matrix(")]
    assert "left to right" in block and "R_j^T R_i" in block and "t_i - t_j" in block and "ghicp_inv_transform" in block


def test_api_lists_the_entry_points(api):
    for name in NAMES:
        assert name in api.EXPORTS
    assert callable(api.Cloud.prepare_overlap) and callable(api.Context.overlap_clouds) and callable(api.Context.overlap_matrix)
    lib = os.path.join(ROOT, "gh-icp_amd", "libghicp_hip.so")
    if os.path.exists(lib):  # the argument checks come before any device work
        L = api.load()
        null = ctypes.c_void_p(0)
        L.ghicp_cloud_prepare_overlap.restype = ctypes.c_int
        assert L.ghicp_cloud_prepare_overlap(null, ctypes.c_float(0.5)) == 1  # GHICP_ERR_ARG on a NULL handle
        L.ghicp_overlap_clouds.restype = ctypes.c_int
        assert L.ghicp_overlap_clouds(null, ctypes.c_float(0.5), 0, null, null, null, 0, null) == 1  # ... and on a NULL context
        L.ghicp_overlap_matrix.restype = ctypes.c_int
        assert L.ghicp_overlap_matrix(null, ctypes.c_float(0.5), 0, null, null, null) == 1


def test_ctypes_mirror_has_the_layout_of_the_c_struct(api, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ghicp_c.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(ghicp_overlap_result), offsetof(ghicp_overlap_result, hits),\n'
                   '  offsetof(ghicp_overlap_result, n), offsetof(ghicp_overlap_result, ratio), offsetof(ghicp_overlap_result, pad_)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    size, o_hits, o_n, o_ratio, o_pad = (int(v) for v in subprocess.check_output([exe]).split())
    R = api.OverlapResult
    assert (ctypes.sizeof(R), R.hits.offset, R.n.offset, R.ratio.offset, R.pad_.offset) == (size, o_hits, o_n, o_ratio, o_pad)
    assert (R.hits.size, R.n.size, R.ratio.size) == (8, 8, 4)


def test_chunk_planner_and_block_search_under_sanitizers(tmp_path):
    """tests/cpp/test_overlap_plan.cpp: the sizes [257, 1, 0, 256, 513, 64, 0] (every block index maps back to the right pair and in-pair
    block, pairs without blocks are never returned), max_concurrent 0, 1, 2, n and n + 1, an empty list, all-zero sizes, a block cap that
    forces a split in the middle.  A stand-alone program, built with AddressSanitizer and UBSan."""
    exe = str(tmp_path / "test_overlap_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "gh-icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_overlap_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "overlap_plan ok" in r.stdout, r.stdout + r.stderr
