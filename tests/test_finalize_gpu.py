"""k_finalize_reads against the record rule at every decision boundary, bit for bit.

The reads come from tests/finalize_cases.py: a class of reads on each side of each threshold of the rule, on both strands
(what each class is and that it is delivered is checked without a GPU, tests/test_finalize_cases.py), and batches that put
chosen reads on chosen lanes, because the kernel's reverse pass is steered by its whole wave (who needs the pass, whether any
lane's window holds an N, the longest window).  Every record is compared with TWO references: the Python restatement of the
rule in finalize_cases.py, written from the reference without the oracle's extract function, and orc.extract_batch.
Everything is an integer; nothing has a tolerance.  Needs a real MI355X: `pytest -m gpu`."""
from collections import Counter

import numpy as np
import pytest

import finalize_cases as fc
from badger_amd import _native, synth

pytestmark = pytest.mark.gpu

CONFIGS = [(10, _native.STRAND_RULE_DEFAULT), (12, _native.STRAND_RULE_DEFAULT), (12, _native.STRAND_RULE_NO_POLYA)]
COUNTERS = {"hits", "clusters", "filter_in", "filter_skipped", "filter_kept", "requeued", "alignments", "filter_in_clusters", "filter_searches"}
assert (_native.STRAND_RULE_DEFAULT, _native.STRAND_RULE_NO_POLYA) == (fc.RULE_DEFAULT, fc.RULE_NO_POLYA)


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _check(ctx, orc, batch, umi_len, rule, lead=None):
    """one batch through bdg_extract_batch under `rule`; lead: a read put in front and skipped through off[1:]"""
    reads = batch.reads
    bases, off = synth.list_to_reads(reads if lead is None else [lead] + reads)
    ctx.extract_set_strand_rule(rule)
    try:
        got = ctx.extract_batch(bases, off if lead is None else off[1:], umi_len)
        status = ctx.extract_status()
        counters = ctx.extract_counters()
    finally:
        ctx.extract_set_strand_rule(_native.STRAND_RULE_DEFAULT)
    assert status[0] == 0, status
    assert set(counters) == COUNTERS and counters["hits"] > 0 and counters["alignments"] > 0, counters
    skip = 0 if lead is None else 1
    for name, want in (("the restatement", fc.records(reads, umi_len, rule)),
                       ("the oracle", orc.extract_batch(bases, off, umi_len, threads=8, rule=rule)[skip:])):
        assert len(got) == len(want) == len(reads)
        bad = np.nonzero(got != want)[0]
        assert not len(bad), "%s, umi_len %d, rule %d: %d of %d records differ from %s; first: read %d (lane %d of wave %d), class %s\n" \
            "got  %s\nwant %s\n%s" % (batch.name, umi_len, rule, len(bad), len(reads), name, bad[0], bad[0] % 64, bad[0] // 64,
                                      batch.labels[bad[0]], got[bad[0]], want[bad[0]], fc.describe(reads[bad[0]], umi_len, rule))
    return got


@pytest.mark.parametrize("umi_len,rule", CONFIGS)
def test_reads_on_every_boundary(ctx, orc, umi_len, rule):
    counts = Counter()
    for b in fc.generator_batches():
        got = _check(ctx, orc, b, umi_len, rule)
        counts.update(b.labels)
        print("%-24s %5d reads in %3d classes, %5d valid" % (b.name, len(b.reads), len(set(b.labels)), int(got["valid"].sum())))
    for name, n in counts.items():
        print("%-72s %d" % (name, n))
    assert min(counts.values()) >= fc.PER and set(c.split("/")[0] for c in counts) == set(fc.GENERATORS)


@pytest.mark.parametrize("umi_len,rule", CONFIGS)
def test_wave_shaped_batches(ctx, orc, umi_len, rule):
    for b in fc.wave_batches():
        _check(ctx, orc, b, umi_len, rule)
        print("%-40s %5d reads: %s" % (b.name, len(b.reads), dict(Counter(x.split(":")[0] for x in b.labels))))


@pytest.mark.parametrize("umi_len,rule", CONFIGS)
def test_every_class_shuffled_among_synthetic_reads(ctx, orc, umi_len, rule):
    b = fc.shuffled_batch()
    got = _check(ctx, orc, b, umi_len, rule)
    assert len(b.reads) == len(fc.all_cases()) + 300 and 0.3 < got["valid"].mean() < 0.95


def test_wave_shaped_batches_as_a_sub_range(ctx, orc):
    """(i) to (iv) again as a sub-range of a larger buffer: off[0] != 0 and no multiple of 16, so that no read starts where it
    started before relative to the 16-byte vectors the kernel loads its windows with"""
    n = 0
    for b in fc.wave_batches():
        if b.name.startswith(("wave_all_rev", "wave_one_", "waves_of_one_ncol_each")):
            for lead in ("ACGTTGCAAGGCTCAGACTGCATGCAATCGACATGAC", "G" * 133):
                assert len(lead) % 16
                _check(ctx, orc, b, 12, _native.STRAND_RULE_DEFAULT, lead=lead)
            n += 1
    assert n == 2 * 9
