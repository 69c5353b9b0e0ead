"""The compiler's resource counts of the per-gene UMI kernels for gfx950 (CPU tier: hipcc cross-compiles without a GPU).
k_umi_insert_genes (both forms) and k_group_emit are memory-bound table kernels that count on many resident waves:
neither may use scratch, and each stays at or below 64 VGPRs - the kernels they run beside in csrc/umi_kernels.hip report 6 to
30.  Resource counts only."""
import os
import shutil
import subprocess

import pytest

from test_genes_isa import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "umi.s")
    src = os.path.join(ROOT, "badger_amd", "csrc", "umi_kernels.hip")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-Wno-unused-function",
                    "-Wno-inline-asm", "-Wno-unused-command-line-argument", "-I", os.path.join(ROOT, "include"), "-o", out, src],
                   check=True, timeout=600)
    return open(out).read()


@pytest.mark.parametrize("name", ("18k_umi_insert_genesILb1EE", "18k_umi_insert_genesILb0EE", "12k_group_emitE"))
def test_per_gene_kernel_budget(text, name):
    vgpr, agpr, scratch, lds = _resources(text, name)
    print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch, %d bytes of LDS" % (name, vgpr, agpr, scratch, lds))
    assert scratch == 0, name + " spills"
    assert lds == 0, (name, lds)
    assert vgpr + agpr <= 64, (name, vgpr, agpr)



# VGPRs of the kernels that took the shared probe (find_or_claim) and the shared wave grouping (wave_groups), as the compiler
# reported them for the commit before the fold, each with its own copy of both loops
BEFORE_THE_FOLD = {"12k_umi_insertE": 14, "12k_mol_insertILb1EE": 26, "12k_mol_insertILb0EE": 12, "11k_umi_cellsE": 10, "12k_umi_parentE": 30}


@pytest.mark.parametrize("name", sorted(BEFORE_THE_FOLD))
def test_shared_probe_and_grouping_cost_no_registers(text, name):
    """k_umi_insert 14 VGPRs, k_mol_insert 26 with the aggregation and 12 without, k_umi_cells 10, k_umi_parent 30 before the
    probe and the grouping were folded into one function each: none may use scratch or LDS, or more than two
    VGPRs above that"""
    vgpr, agpr, scratch, lds = _resources(text, name)
    print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch, %d bytes of LDS" % (name, vgpr, agpr, scratch, lds))
    assert scratch == 0, name + " spills"
    assert lds == 0, (name, lds)
    assert vgpr + agpr <= BEFORE_THE_FOLD[name] + 2, (name, vgpr, agpr)
