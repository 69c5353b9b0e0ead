"""Resources of k_chimera_search in the generated gfx950 code (CPU tier: hipcc cross-compiles without a GPU): no scratch, and a
register count that keeps eight one-wave blocks per SIMD, the occupancy its launch shape (blocks of 64, 2.3 KB of LDS) assumes."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def chimera_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "chimera.s")
    src = os.path.join(ROOT, "badger_amd", "csrc", "chimera_kernels.hip")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-Wno-unused-function",
                    "-Wno-unused-command-line-argument", "-o", out, src], check=True, timeout=600)
    text = open(out).read()
    m = re.search(r"^(_ZN\S*k_chimera_search\S*):[^\n]*\n(.*?)\n\s*\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
    assert m, "k_chimera_search not found in the generated code"
    meta = dict(re.findall(r"\.set \S*k_chimera_search\S*\.(num_vgpr|num_agpr|private_seg_size), (\d+)", text))
    return m.group(2).split("\n"), m.group(3), meta


def test_chimera_kernel_budget(chimera_isa):
    body, desc, meta = chimera_isa
    assert int(meta["private_seg_size"]) == 0, "k_chimera_search uses scratch"
    assert int(meta["num_vgpr"]) + int(meta.get("num_agpr", 0)) <= 64, "more than 64 registers: fewer than 8 waves per SIMD"
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
    assert 32 * lds <= 160 * 1024, "32 one-wave blocks no longer fit a CU's LDS"
    code = [l.strip() for l in body if l.strip() and not l.strip().startswith(";")]
    assert not any(l.startswith(("scratch_", "buffer_store", "buffer_load")) for l in code)
    assert sum(l.startswith("v_bitop3_b32") for l in code) >= 4 * 4 * 5, "the recurrences are no longer three-input operations"
    assert any(l.startswith("ds_min_u64") or l.startswith("ds_min_rtn_u64") for l in code), "the packed key is combined by an LDS minimum"
