"""The compiler's resource counts of k_donor_scores for gfx950 (CPU tier: hipcc cross-compiles without a GPU).  The kernel keeps a
lane's accumulators, up to nine of 64 bits, and its hypotheses' bit positions in registers for every cell it walks:
none of its four instantiations (1, 2, 4 and 9 rounds of 64 hypotheses) may use scratch or LDS, and each stays at or below 128
VGPRs, so that four waves or more are resident per SIMD.  Resource counts only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ROUNDS = (1, 2, 4, 9)


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "donors.s")
    src = os.path.join(ROOT, "badger_amd", "csrc", "donors_kernels.hip")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-Wno-unused-function",
                    "-Wno-inline-asm", "-Wno-unused-command-line-argument", "-I", os.path.join(ROOT, "include"), "-o", out, src],
                   check=True, timeout=600)
    return open(out).read()


def _resources(text, name):
    """-> (VGPRs, AGPRs, scratch bytes per lane, LDS bytes per block) of the kernel whose mangled name holds `name`"""
    m = re.search(r"^\s*\.amdhsa_kernel (_ZN\S*%s\S*)\n(.*?)\.end_amdhsa_kernel" % name, text, re.S | re.M)
    assert m, name + " not found in the generated code"
    meta = dict(re.findall(r"\.set %s\.(num_vgpr|num_agpr|private_seg_size), (\d+)" % re.escape(m.group(1)), text))
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
    return int(meta["num_vgpr"]), int(meta["num_agpr"]), int(meta["private_seg_size"]), lds


def test_every_instantiation_is_there(text):
    found = sorted(int(r) for r in re.findall(r"^\s*\.amdhsa_kernel _ZN\S*14k_donor_scoresILi(\d+)E", text, re.M))
    assert found == list(ROUNDS)


@pytest.mark.parametrize("rounds", ROUNDS)
def test_donor_kernel_budget(text, rounds):
    name = "14k_donor_scoresILi%dE" % rounds
    vgpr, agpr, scratch, lds = _resources(text, name)
    print("k_donor_scores<%d>: %d VGPRs, %d AGPRs, %d bytes of scratch, %d bytes of LDS" % (rounds, vgpr, agpr, scratch, lds))
    assert scratch == 0, name + " spills"
    assert lds == 0, (name, lds)
    assert vgpr + agpr <= 128, (name, vgpr, agpr)
