"""The compiler's resource counts of the clustering kernels for gfx950 (CPU tier: hipcc cross-compiles without a GPU).  Every
kernel of csrc/demux_kernels.hip stays without scratch and at or below 128 VGPRs, so that four waves or more are resident per
SIMD; k_cluster_assign, the hot one, keeps its per-cluster score in a register and hands the entries round by v_readlane, so it
uses no LDS either.  Resource counts only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("k_cluster_counts", "k_cluster_assign", "k_cluster_words", "k_cluster_geno", "k_cluster_renumber")


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "demux.s")
    src = os.path.join(ROOT, "badger_amd", "csrc", "demux_kernels.hip")
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


def test_every_kernel_is_there(text):
    found = sorted(set(re.findall(r"^\s*\.amdhsa_kernel _ZN\S*?\d+(k_cluster_[a-z]+)E", text, re.M)))
    assert found == sorted(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_cluster_kernel_budget(text, kernel):
    vgpr, agpr, scratch, lds = _resources(text, "%d%sE" % (len(kernel), kernel))
    print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch, %d bytes of LDS" % (kernel, vgpr, agpr, scratch, lds))
    assert scratch == 0, kernel + " spills"
    assert vgpr + agpr <= 128, (kernel, vgpr, agpr)
    if kernel == "k_cluster_assign":
        assert lds == 0, (kernel, lds)
