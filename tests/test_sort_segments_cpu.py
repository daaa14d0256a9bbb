"""The host plan of the segmented radix sort (gh-icp_amd/csrc/sort_plan.h) through tests/cpp/test_sort_plan.cpp: digit places from the key bits
present, and the tile / chunk partition of the segments.  The kernels that run on the plan are tested by tests/test_gpu_sort_segments.py, on the GPU
and -- with every other `gpu` test -- on the host SIMT interpreter (tests/test_sim_cpu.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, CHUNK = 4096, 64


def build(tmp_path, sanitize):
    exe = str(tmp_path / "test_sort_plan")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + flags + ["-I", os.path.join(ROOT, "gh-icp_amd", "csrc"),
                                                                       os.path.join(ROOT, "tests", "cpp", "test_sort_plan.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_place_plan_and_tile_partition(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    seg_cases = [[0, 1], [0, TILE - 1], [0, TILE], [0, TILE + 1], [0, 0, 0, 7], [0, TILE, 2 * TILE - 1, 2 * TILE - 1, 4 * TILE],
                 [0, CHUNK * TILE, 2 * CHUNK * TILE + 1, 2 * CHUNK * TILE + 1], [0] + [300 * (i + 1) for i in range(64)], [0, (1 << 31) - 3]]
    text = "".join("p %d %d\n" % (b, w) for w in (8, 9) for b in range(0, 65))
    text += "".join("s %d %s\n" % (len(o) - 1, " ".join(map(str, o))) for o in seg_cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for w in (8, 9):
        for bits in range(0, 65):
            got = [int(v) for v in lines.pop(0).split()]
            places, widths = got[0], got[1:]
            # the fewest places that digits of at most w bits allow, 9-bit digits only where they save a place; widths sum to the bits, differ by at most one
            want = min(-(-bits // 8), -(-bits // w))
            assert places == want == len(widths) and sum(widths) == bits, (bits, w, got)
            if places:
                assert max(widths) - min(widths) <= 1 and max(widths) <= w and min(widths) >= 1, (bits, w, got)
                assert max(widths) <= 8 or -(-bits // 8) > places, (bits, w, got)
    # what the issue aims at
    plan = lambda bits, w=9: [int(v) for v in subprocess.run([exe], input="p %d %d\n" % (bits, w), capture_output=True, text=True).stdout.split()][1:]
    assert sorted(plan(34)) == [8, 8, 9, 9] and plan(39, 8) == [8, 8, 8, 8, 7] and plan(34, 8) == [7, 7, 7, 7, 6] and plan(24) == [8, 8, 8] and plan(27) == [9, 9, 9]
    for off in seg_cases:
        longest = int(lines.pop(0))
        assert longest == max(b - a for a, b in zip(off, off[1:]))
        t = c = 0
        for i, o in enumerate(off):
            assert [int(v) for v in lines.pop(0).split()] == [o, t, c], (off, i)
            if i + 1 < len(off):
                nt = -(-(off[i + 1] - o) // TILE)
                t += nt
                c += -(-nt // CHUNK)
