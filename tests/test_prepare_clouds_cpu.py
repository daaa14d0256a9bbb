"""CPU checks of the interface of the batched prepare (include/ghicp_c.h, gh-icp_amd/api.py) and of its chunk planner
(gh-icp_amd/csrc/prepare_plan.h)."""
import ctypes
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ghicp_prepare_spec_default", "ghicp_clouds_prepare", "ghicp_ctx_prepare_host_waits", "ghicp_cloud_get_prepared", "ghicp_cloud_download_prepared")

MAX_CLOUDS, MAX_POINTS, MAX_CELLS = 64, (1 << 31) - 2, 1 << 28  # the library's limits (prepare_plan.h)


def _args(h, name):
    m = re.search(r"int %s\(([^;]*)\);" % name, h)
    assert m, name
    return " ".join(re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S).split())


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "ghicp_c.h")).read()
    assert _args(h, "ghicp_prepare_spec_default") == "ghicp_prepare_spec* s"
    assert _args(h, "ghicp_clouds_prepare") == "ghicp_ctx* ctx, int32_t n_clouds, ghicp_cloud* const* clouds , const ghicp_prepare_spec* spec"
    assert _args(h, "ghicp_cloud_get_prepared") == "const ghicp_cloud* cloud, ghicp_cloud_prepared* out"
    assert _args(h, "ghicp_cloud_download_prepared") == "const ghicp_cloud* cloud, int32_t which, void* out"
    assert _args(h, "ghicp_ctx_prepare_host_waits") == "const ghicp_ctx* ctx, int64_t* waits"
    for name in ("ghicp_prepare_spec", "ghicp_grid_info", "ghicp_cloud_prepared"):
        assert re.search(r"typedef struct %s \{[^}]*\} %s;" % (name, name), h), name
    enum = re.search(r"enum \{ (GHICP_PREP_FINE_PTS,[^}]*) \};", h)
    assert [s.strip() for s in enum.group(1).split(",")] == [
        "GHICP_PREP_FINE_PTS", "GHICP_PREP_FINE_START", "GHICP_PREP_COARSE_PTS", "GHICP_PREP_COARSE_START", "GHICP_PREP_OVERLAP_PTS",
        "GHICP_PREP_OVERLAP_START", "GHICP_PREP_NORMALS", "GHICP_PREP_COVARIANCES"]
    assert h.index("ghicp_clouds_recompute(") < h.index("ghicp_clouds_prepare(") < h.index("ghicp_pairqueue_create(")


def test_api_lists_the_entry_points(api):
    for name in NAMES:
        assert name in api.EXPORTS
    assert callable(api.Context.prepare_clouds) and callable(api.Cloud.prepared) and callable(api.Cloud.download_prepared)
    assert [api.PREP_FINE_PTS, api.PREP_FINE_START, api.PREP_COARSE_PTS, api.PREP_COARSE_START, api.PREP_OVERLAP_PTS, api.PREP_OVERLAP_START,
            api.PREP_NORMALS, api.PREP_COVARIANCES] == list(range(8))
    lib = os.path.join(ROOT, "gh-icp_amd", "libghicp_hip.so")
    if os.path.exists(lib):  # the argument checks come before any device work
        L = api.load()
        null = ctypes.c_void_p(0)
        for name in NAMES:
            getattr(L, name).restype = ctypes.c_int
        assert L.ghicp_prepare_spec_default(null) == 1  # GHICP_ERR_ARG
        s = api.PrepareSpec()
        s.refine = s.normals_k = s.gicp_k = s.overlap = 7
        assert L.ghicp_prepare_spec_default(ctypes.byref(s)) == 0
        assert (s.refine, s.normals_k, s.gicp_k, s.overlap, s.pad_) == (0, 0, 0, 0, 0) and s.gicp_epsilon == 1e-3 and s.thre_dis == 0.5
        assert L.ghicp_clouds_prepare(null, 0, null, ctypes.byref(s)) == 1  # a NULL context
        assert L.ghicp_cloud_get_prepared(null, null) == 1 and L.ghicp_cloud_download_prepared(null, 0, null) == 1
        assert L.ghicp_ctx_prepare_host_waits(null, null) == 1


def test_ctypes_mirrors_have_the_layout_of_the_c_structs(api, tmp_path):
    fields = {"ghicp_prepare_spec": ["refine", "normals_k", "gicp_k", "overlap", "thre_dis", "pad_", "gicp_epsilon"],
              "ghicp_grid_info": ["mn", "inv", "dim", "n", "ncell", "pad_"],
              "ghicp_cloud_prepared": ["refine_ready", "normals_k", "gicp_ready", "gicp_k", "overlap_ready", "pad_", "thre_dis", "pad2_", "gicp_epsilon",
                                       "fine", "coarse", "overlap"]}
    mirrors = {"ghicp_prepare_spec": api.PrepareSpec, "ghicp_grid_info": api.GridInfo, "ghicp_cloud_prepared": api.CloudPrepared}
    body = "".join('  printf("%%zu", sizeof(%s));%s  printf("\\n");\n' % (s, "".join(' printf(" %%zu %%zu", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, f, s, f) for f in fs))
                   for s, fs in fields.items())
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ghicp_c.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = subprocess.check_output([exe]).decode().strip().split("\n")
    for (s, fs), line in zip(fields.items(), lines):
        v = [int(x) for x in line.split()]
        M = mirrors[s]
        assert [f for f, _ in M._fields_] == fs
        assert ctypes.sizeof(M) == v[0], s
        for i, f in enumerate(fs):
            assert (getattr(M, f).offset, getattr(M, f).size) == (v[1 + 2 * i], v[2 + 2 * i]), (s, f)


# ------------------------------------------------------------------------------------------------ planner
def plan_py(sizes, max_clouds=MAX_CLOUDS, max_points=MAX_POINTS, max_cells=MAX_CELLS):
    """the rule of prepare_plan.h restated: consecutive clouds; a chunk is closed when the next cloud would make it exceed max_clouds
    clouds, reach max_points points or exceed max_cells cells of one grid kind; a cloud always gets a chunk, if need be alone"""
    chunks, first = [], 0
    while first < len(sizes):
        count, pts, cells = 0, 0, [0, 0, 0]
        while first + count < len(sizes) and count < max_clouds:
            m, c = sizes[first + count][0], sizes[first + count][1:]
            if not (pts + m < max_points and all(cells[k] + c[k] <= max_cells for k in range(3))):
                break
            pts += m
            cells = [cells[k] + c[k] for k in range(3)]
            count += 1
        count = max(count, 1)
        chunks.append((first, count))
        first += count
    return chunks


def cases():
    rnd = random.Random(5)
    out = []
    for n in (0, 1, 64, 65, 200):  # uniform small clouds: only the cloud count splits
        out.append(([(1000, 5000, 700, 300)] * n, None))
    for _ in range(40):  # random sizes under small limits, so that every limit is hit
        n = rnd.randrange(0, 90)
        out.append(([(rnd.randrange(0, 400), rnd.randrange(0, 900), rnd.randrange(0, 900), rnd.randrange(0, 900)) for _ in range(n)],
                    (rnd.choice((1, 3, 8, 64)), rnd.randrange(300, 3000), rnd.randrange(800, 6000))))
    big = (MAX_POINTS - 1, 1 << 26, 1 << 26, 1 << 26)  # a cloud at the point and cell limits: fits, alone or with empty neighbours
    out.append(([big], None))
    out.append(([(0, 0, 0, 0), big, (0, 0, 0, 0), big, (10, 1, 1, 1)], None))
    out.append(([(MAX_POINTS // 2, 9, 9, 9), (MAX_POINTS - MAX_POINTS // 2 - 1, 9, 9, 9), (1, 9, 9, 9)], None))  # the sum stays one below the limit, then reaches it
    out.append(([(5, 1 << 26, 0, 0)] * 4 + [(5, 0, 1 << 27, 0)] * 2 + [(5, 0, 0, 1)] + [(5, 1, 1 << 27, 1 << 28)], None))  # cell sums that hit the limit exactly, then cross it
    out.append(([(100, 10, 10, 10)] * 10, (64, 301, 30)))  # both sums cross exactly at a boundary
    return out


def check_plan(sizes, chunks, limits):
    max_clouds, max_points, max_cells = limits or (MAX_CLOUDS, MAX_POINTS, MAX_CELLS)
    nxt = 0
    for first, count in chunks:  # the chunks cover the list in order
        assert first == nxt and count >= 1
        nxt = first + count
        part = sizes[first:first + count]
        if count > 1:  # no chunk breaks a limit (a cloud alone is always taken)
            assert count <= max_clouds and sum(p[0] for p in part) < max_points
            for k in range(3):
                assert sum(p[1 + k] for p in part) <= max_cells
    assert nxt == len(sizes)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_chunk_planner_against_its_restatement(tmp_path, sanitize):
    exe = str(tmp_path / "test_prepare_plan")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + flags + ["-I", os.path.join(ROOT, "gh-icp_amd", "csrc"),
                                                                       os.path.join(ROOT, "tests", "cpp", "test_prepare_plan.cpp"), "-o", exe])
    cs = cases()
    text = ""
    for sizes, limits in cs:
        text += "%d %d %d %d\n" % ((len(sizes),) + (limits or (0, 0, 0)))
        text += "".join("%d %d %d %d\n" % s for s in sizes)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got, cur = [], []
    for line in r.stdout.split("\n"):
        if line == "end":
            got.append(cur)
            cur = []
        elif line:
            cur.append(tuple(int(v) for v in line.split()))
    assert len(got) == len(cs)
    for (sizes, limits), chunks in zip(cs, got):
        assert chunks == plan_py(sizes, *(limits or ())), (sizes[:8], limits)
        check_plan(sizes, chunks, limits)
    # the uniform lists split by the cloud count alone
    assert [len(g) for g in got[:5]] == [0, 1, 1, 2, 4] and got[3] == [(0, 64), (64, 1)]
