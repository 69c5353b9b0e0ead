"""The wave shapes of tests/umi_cases.py through every entry point of csrc/umi_kernels.hip that groups the lanes of a wave by
key (wave_groups): bdg_umi_dedup_dev, bdg_molecule_reps_dev and bdg_umi_dedup_genes_dev, the last two with the aggregation on
and off.  A wave in which every lane holds one key, every lane its own, two keys in turn, a key on lanes 0 and 63 only, no key
at all, and a key across the boundary of two waves; 1, 63, 64, 65 and 257 reads; a lane without a key being a read without a
cell, and a read without a usable UMI, a molecule or a gene.  Every output against the Python rules, exactly."""
import pytest

import molecule_cases as mc
import umi_cases as uc
import umi_gene_cases as ug
from badger_amd import _native
from badger_amd import umi_dedup as ud
from test_molecule_reads_gpu import _device as _mol_device, _same as _mol_same
from test_umi_kernels_gpu import _device as _cell_device, _same as _cell_same
from test_umi_per_gene_gpu import _device as _gene_device, _same as _gene_same

pytestmark = pytest.mark.gpu

CELLS = [1000, 2000, 0xFFFFFFF0]


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _molecule_case(shape, n, absent):
    """key k: cell k % 3, molecule wave_umi(k // 3); no key: no cell, or no molecule.  cDNA lengths with ties and zeros."""
    rank, has, mol = [], [], []
    for i, k in enumerate(uc.wave_keys(shape, n)):
        rank.append(CELLS[(i if k is None else k) % 3])
        has.append(0 if k is None and absent == "cell" else 1)
        mol.append(ud.NONE if k is None and absent != "cell" else ud.umi_code(uc.wave_umi((i if k is None else k) // 3)))
    return mc.Case("wave_%s_%d_%s" % (shape, n, absent), CELLS, rank, has, mol, [i * 37 % 5 * 40 for i in range(n)])


def _gene_case(shape, n, absent):
    """key k: the group (cell k % 3, feature k // 3); no key: no cell, or a record that is not ASSIGNED.  Four UMIs in turn, one
    read in seven without a usable one (a molecule of its own)"""
    reads = []
    for i, k in enumerate(uc.wave_keys(shape, n)):
        umi = "" if i % 7 == 3 else uc.wave_umi(i % 4)
        if k is not None:
            reads.append((k % 3, k // 3, ug.A, umi))
        else:
            reads.append((None, i, ug.A, umi) if absent == "cell" else (i % 3, i // 3, ug.gn.LOW, umi))
    return ug.GeneCase("wave_%s_%d_%s" % (shape, n, absent), reads)


@pytest.mark.parametrize("n", uc.WAVE_SIZES)
def test_wave_shapes(ctx, n):
    for shape in uc.WAVE_SHAPES:
        for absent in ("cell", "umi"):
            what = "%s, %d reads, lanes without a key: no %s" % (shape, n, absent)
            case = uc.wave_case(shape, n, absent)
            for dist in (0, 1):
                _cell_same(case, _cell_device(ctx, case, 12, dist), uc.rule(case, 12, dist), what)
            case = _molecule_case(shape, n, absent)
            want = case.rule()
            for aggregate in (True, False):
                _mol_same(case, _mol_device(ctx, case, aggregate), want, "%s, aggregate %d" % (what, aggregate))
            case = _gene_case(shape, n, absent)
            want = ug.rule(case, 12, 1)
            for aggregate in (True, False):
                ctx.umi_dedup_genes_set_aggregate(aggregate)
                try:
                    _gene_same(case, _gene_device(ctx, case, 12, 1), want, "%s, aggregate %d" % (what, aggregate))
                finally:
                    ctx.umi_dedup_genes_set_aggregate(True)
