"""Static check of the persistent pair loop's register budget: pair_loop.hip is cross-compiled for gfx950 with the Makefile's flags and the
code object's METADATA is read for the six instantiations of k_pair_loop (feature 3 / 0 / 2, each with and without the solver's profile
counters, in the order the metadata lists them): at most 128 VGPRs (four slots per CU), and no more spilled VGPRs or private segment than the ceilings below.
The ceilings are this tree's values; each is at or below its value before the solver's wave-uniform state moved into scalar registers
(spilled VGPRs 16 / 6 / 16 / 8 / 27 / 27, private segment 640 / 368 / 640 / 368 / 656 / 484 B).  Metadata fields only: no instruction is looked for."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gh-icp_amd", "csrc")

KERNELS = ["ILi3ELb1E", "ILi3ELb0E", "ILi0ELb1E", "ILi0ELb0E", "ILi2ELb1E", "ILi2ELb0E"]  # k_pair_loop<FT, PROF>
BEFORE_SPILL = [16, 6, 16, 8, 27, 27]
BEFORE_PRIVATE = [640, 368, 640, 368, 656, 484]
CEIL_SPILL = [4, 4, 4, 4, 10, 10]
CEIL_PRIVATE = [480, 352, 480, 352, 496, 436]


def _make_var(name):
    text = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^%s\s*\?=\s*(.*)$" % name, text, re.M)
    assert m, name
    return m.group(1).strip()


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", _make_var("HIPCC"))
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc")
    flags = _make_var("FLAGS").replace("$(ARCH)", _make_var("ARCH")).split()
    out = str(tmp_path_factory.mktemp("regs") / "pair_loop.s")
    subprocess.check_call([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(CSRC, "pair_loop.hip"), "-o", out], cwd=CSRC, stderr=subprocess.DEVNULL)
    recs, cur = [], None
    for line in open(out):
        m = re.match(r"\s+(?:- )?\.(name|vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "name":
            cur = {"name": m.group(2)} if "k_pair_loop" in m.group(2) else None
            if cur is not None:
                recs.append(cur)
        elif cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return recs


def test_six_instantiations_in_the_expected_order(metadata):
    assert len(metadata) == 6
    for r, k in zip(metadata, KERNELS):
        assert "k_pair_loop" + k in r["name"], (r["name"], k)


def test_registers_spills_and_private_segment(metadata):
    for i, r in enumerate(metadata):
        print(r)
        assert r["vgpr_count"] <= 128, r
        assert CEIL_SPILL[i] <= BEFORE_SPILL[i] and CEIL_PRIVATE[i] <= BEFORE_PRIVATE[i]
        assert r["vgpr_spill_count"] <= CEIL_SPILL[i], r
        assert r["private_segment_fixed_size"] <= CEIL_PRIVATE[i], r
