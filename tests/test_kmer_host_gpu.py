"""The host side of the k-mer lookups (csrc/genes_kernels.hip, csrc/alleles_kernels.hip: the staged calls over host buffers and
the resident-wave launches) against the rules of badger_amd/genes.py and badger_amd/alleles.py, every field of every record.
Reads that lie in a window of a larger buffer, so that their offsets do not start at 0 (the staging ships the window rebased to
0); and more reads than any grid of resident waves holds, twice on one context, so that every launcher takes its grid-stride
path, the second time with its cached blocks-per-unit figure."""
import numpy as np
import pytest

import alleles_cases as ac
import genes_cases as gc
import iso_cases as ic
from badger_amd import _native
from badger_amd import alleles as al
from badger_amd import genes as gn

pytestmark = pytest.mark.gpu

K = 11


def _flat(seqs, lead=b"", tail=b""):
    """the reads behind `lead` and in front of `tail` in one buffer -> (bases, offsets: the first is len(lead))"""
    flat = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    return (np.frombuffer(lead + b"".join(flat) + tail, dtype=np.uint8),
            (len(lead) + np.concatenate([[0], np.cumsum([len(s) for s in flat], dtype=np.int64)])).astype(np.uint64))


def _revcomp(s):
    return gn.span_sequence(s, 0, len(s), 1).decode()


@pytest.fixture(scope="module")
def model():
    """two genes, three transcripts: gene 0 has two that differ in base 60, gene 1 has one; a site in each gene; the checker's
    two indices"""
    rng = np.random.default_rng(2611)
    t0, t2 = gc.rand_seq(rng, 90), gc.rand_seq(rng, 70)
    t1 = t0[:60] + ac.other_letter(rng, t0[60]) + t0[61:]
    seqs, feats = [t0, t1, t2], [0, 0, 1]
    local = gn.local_indices(feats)[0]
    variants = al.Variants(["a", "b"], [t0[20], t2[30]], [ac.other_letter(rng, t0[20]), ac.other_letter(rng, t2[30])], [0, 1],
                           [(0, 0, 20), (0, 1, 20), (1, 2, 30)])
    a_seqs, a_values = al.allele_sequences(variants, [s.encode() for s in seqs], K)
    return dict(seqs=seqs, feats=feats, local=local, variants=variants, a_seqs=a_seqs, a_values=a_values,
                index=gn.build_index(seqs, feats, K, local), a_index=al.build_index(a_seqs, a_values, variants.gene, 2, K))


@pytest.fixture()
def ctx(model):
    """a context of its own per test (nothing cached), both tables built"""
    c = _native.Context(0)
    c.genes_index_build_iso(*_flat(model["seqs"]), np.asarray(model["feats"], np.uint32), model["local"], K)
    c.alleles_index_build(*_flat(model["a_seqs"]), model["a_values"], model["variants"].gene, 2, K)
    yield c
    c.close()


def _rule(model, reads, spans, allele_genes=None):
    """the checkers' records of the reads; the allele records under the gene records allele_genes (default: the checker's own)"""
    index = model["index"]
    gene = gn.assign_reads(index, reads, 1)
    iso = gn.iso_assign_reads(index, reads, gene, 1)
    sp_gene, sp_iso = gn.assign_spans(index, reads, spans, 1, 1)
    alleles, crowded = al.assign_reads(model["a_index"], reads, gene if allele_genes is None else allele_genes)
    assert crowded == 0
    return dict(gene=gene, iso=iso, sp_gene=sp_gene, sp_iso=sp_iso, alleles=alleles)


def _device(ctx, bases, off, spans, gene_recs):
    """genes_assign, iso_assign, genes_assign_spans without and with a margin, alleles_assign -> tuples per call"""
    out = {}
    out["genes_assign"] = gc.rec_tuples(ctx.genes_assign(bases, off, 1))
    g, i = ctx.iso_assign(bases, off, 1, 1)
    out["iso_assign"] = (gc.rec_tuples(g), ic.iso_tuples(i))
    out["genes_assign_spans"] = gc.rec_tuples(ctx.genes_assign_spans(bases, off, spans, 1, 0))
    g, i = ctx.genes_assign_spans(bases, off, spans, 1, 1)
    out["genes_assign_spans, margin"] = (gc.rec_tuples(g), ic.iso_tuples(i))
    recs, crowded = ctx.alleles_assign(bases, off, gene_recs)
    out["alleles_assign"] = (recs.tolist(), crowded)
    return out


def _want(rule):
    return {"genes_assign": gc.rec_tuples(rule["gene"]),
            "iso_assign": (gc.rec_tuples(rule["gene"]), ic.iso_tuples(rule["iso"])),
            "genes_assign_spans": gc.rec_tuples(rule["sp_gene"]),
            "genes_assign_spans, margin": (gc.rec_tuples(rule["sp_gene"]), ic.iso_tuples(rule["sp_iso"])),
            "alleles_assign": (rule["alleles"].tolist(), 0)}


def test_offsets_that_do_not_start_at_0(ctx, model):
    t0, t1, t2 = model["seqs"]
    v = model["variants"]
    # 35 bases of gene 0 with the alt allele of its site, an empty read, 38 bases of gene 1 over its site stored as the reverse
    # complement, 30 bases over the base in which the two transcripts of gene 0 differ
    reads = [t0[10:20] + v.alt[0] + t0[21:45], "", _revcomp(t2[20:58]), t1[45:75]]
    spans = np.array([(3, 33, 0), (0, 0, 0), (0, 38, 1), (2, 29, 0)], dtype=_native.SPAN_DTYPE)
    assert [len(r) for r in reads] == [35, 0, 38, 30]
    rule = _rule(model, reads, spans)
    want = _want(rule)
    # the case says something: genes and an isoform call on both paths, the rc span found only as a span, an allele record
    assert [g[0] for g in want["genes_assign"]] == [0, gn.NONE, gn.NONE, 0]
    assert [g[0] for g in want["genes_assign_spans"]] == [0, gn.NONE, 1, 0]
    assert want["iso_assign"][1][3][0] == 2 and want["genes_assign_spans, margin"][1][3][0] == 2      # (compat: transcript 1 alone)
    assert want["alleles_assign"][0] == [(0, 0, 0, K)]
    # the junk in front is text of gene 1 and the junk behind text of gene 0: a read looked up at the wrong place finds keys
    lead, tail = t2[:37].encode(), t0[:20].encode()
    at_0 = _device(ctx, *_flat(reads), spans, rule["gene"])
    bases, off = _flat(reads, lead, tail)
    assert int(off[0]) == 37
    behind = _device(ctx, bases, off, spans, rule["gene"])
    for call in want:
        assert behind[call] == want[call], call + ": the records behind 37 bytes and the checker's differ"
        assert at_0[call] == behind[call], call + ": the records from offset 0 and behind 37 bytes differ"


def test_more_reads_than_resident_waves(ctx, model):
    t0, t1, t2 = model["seqs"]
    v = model["variants"]
    rng = np.random.default_rng(8)
    L = K + 2
    eight = [t0[15:15 + L], t0[15:20] + v.alt[0] + t0[21:15 + L], t2[25:25 + L], t2[25:30] + v.alt[1] + t2[31:25 + L],
             t0[52:52 + L], t1[52:52 + L], gc.rand_seq(rng, L), _revcomp(t0[40:40 + L])]
    spans8 = np.array([(0, L, 0)] * 4 + [(1, L, 0), (0, L, 0), (0, L - 1, 0), (0, L, 1)], dtype=_native.SPAN_DTYPE)
    assert len(set(eight)) == 8 and all(len(r) == L for r in eight)
    # (13 bases around an alt allele hold no key of the gene index: the allele pass gets gene records that name each read's gene)
    genes8 = ac.gene_recs([0, 0, 1, 1, 0, 0, 1, 0])
    rule = _rule(model, eight, spans8, genes8)                     # (the checker runs over the eight reads only)
    assert [int(f) for f in rule["gene"]["feature"]] == [0, gn.NONE, 1, gn.NONE, 0, 0, gn.NONE, gn.NONE]
    assert int(rule["sp_gene"]["feature"][7]) == 0 and [int(c) for c in rule["sp_iso"]["compat"][[4, 5]]] == [1, 2]
    assert rule["alleles"].tolist() == [(0, 0, 3, 0), (1, 0, 0, 3), (2, 1, 3, 0), (3, 1, 0, 3)]
    n = 20000                                                      # above 256 compute units x 32 single-wave blocks
    which = np.arange(n) % 8
    bases, off = _flat([eight[j] for j in which.tolist()])
    tiled = {name: recs[which] for name, recs in rule.items() if name != "alleles"}
    m = len(rule["alleles"])
    alleles = np.tile(rule["alleles"], n // 8)
    alleles["read"] += np.repeat(np.arange(n // 8, dtype=np.uint32) * 8, m)
    want = _want(dict(tiled, alleles=alleles))
    for round_ in (0, 1):                                          # the second time every launcher has its figure cached
        got = _device(ctx, bases, off, spans8[which], genes8[which])
        for call in want:
            assert got[call] == want[call], "%s, round %d: read i does not have the checker's record of read i %% 8" % (call, round_)
