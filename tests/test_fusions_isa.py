"""The compiler's resource counts of k_fusion_scan for gfx950 (CPU tier: hipcc cross-compiles without a GPU).  Like the gene kernels
it counts on many resident waves per compute unit to hide the table's latency: it may not use scratch, stays at or
below 128 VGPRs, and declares exactly the 4,096 bytes of its per-wave table of 256 (feat, cnt, first, last) entries in LDS.
Resource counts only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "fusion.s")
    src = os.path.join(ROOT, "badger_amd", "csrc", "fusion_kernels.hip")
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


def test_fusion_kernel_budget(text):
    name = "13k_fusion_scanE"
    vgpr, agpr, scratch, lds = _resources(text, name)
    print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch, %d bytes of LDS" % (name, vgpr, agpr, scratch, lds))
    assert scratch == 0, name + " spills"
    assert lds == 4096, (name, lds)
    assert vgpr + agpr <= 128, (name, vgpr, agpr)
