"""Resources of k_split_scan in the generated gfx950 code (CPU tier: hipcc cross-compiles without a GPU): no scratch, a register
count that keeps eight one-wave blocks per SIMD, and no more LDS than the kernel had with its own copy of the adapter scan
(5,392 bytes: the ring of 1,024 cell words, four arrays over the wave's reads, the round's two scalars)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_BYTES = 5392


@pytest.fixture(scope="module")
def split_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "split.s")
    src = os.path.join(ROOT, "badger_amd", "csrc", "split_kernels.hip")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-Wno-unused-function",
                    "-Wno-unused-command-line-argument", "-o", out, src], check=True, timeout=600)
    text = open(out).read()
    m = re.search(r"^(_ZN\S*k_split_scan\S*):[^\n]*\n(.*?)\n\s*\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
    assert m, "k_split_scan not found in the generated code"
    meta = dict(re.findall(r"\.set \S*k_split_scan\S*\.(num_vgpr|num_agpr|private_seg_size), (\d+)", text))
    return m.group(2).split("\n"), m.group(3), meta


def test_split_kernel_budget(split_isa):
    body, desc, meta = split_isa
    assert int(meta["private_seg_size"]) == 0, "k_split_scan uses scratch"
    assert int(meta["num_vgpr"]) + int(meta.get("num_agpr", 0)) <= 64, "more than 64 registers: fewer than 8 waves per SIMD"
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
    assert lds <= LDS_BYTES, "k_split_scan takes more LDS than before"
    code = [l.strip() for l in body if l.strip() and not l.strip().startswith(";")]
    assert sum(l.startswith("v_bitop3_b32") for l in code) >= 2 * 4 * 5, "the recurrences are no longer three-input operations"
