"""The compiler's resource counts of the discovery kernels for gfx950 (CPU tier: hipcc cross-compiles without a GPU).  Like the gene
kernels they count on many resident waves per compute unit to hide the table's latency: none of them may use
scratch, each stays at or below 128 VGPRs, and none declares LDS but k_sites_stats, whose block sums its four figures in 32 bytes.
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
    out = str(tmp_path_factory.mktemp("isa") / "discover.s")
    src = os.path.join(ROOT, "badger_amd", "csrc", "discover_kernels.hip")
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


@pytest.mark.parametrize("name, max_vgpr, want_lds", (("14k_sites_insertE", 128, 0), ("13k_sites_statsE", 128, 32),
                                                      ("14k_sites_pileupE", 128, 0), ("14k_sites_selectE", 128, 0)))
def test_discovery_kernel_budget(text, name, max_vgpr, want_lds):
    vgpr, agpr, scratch, lds = _resources(text, name)
    print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch, %d bytes of LDS" % (name, vgpr, agpr, scratch, lds))
    assert scratch == 0, name + " spills"
    assert lds == want_lds, (name, lds)
    assert vgpr + agpr <= max_vgpr, (name, vgpr, agpr)
