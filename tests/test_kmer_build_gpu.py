"""The builds of the three k-mer tables (csrc/genes_probe.hpp: kmer_walk under k_genes_insert, k_iso_insert, k_alleles_insert and
k_sites_insert, kmer_stats under k_genes_stats, k_alleles_stats and k_sites_stats, and the host's frame around them) over one set
of boundary inputs, against the numpy checkers of badger_amd/genes.py, badger_amd/alleles.py and badger_amd/discover.py: the six
figures of every table, and every table's content by looking the sequences themselves up as reads.  Exact equality throughout.

The sequences, for k = 11, 21 and 31: lengths around k, around a chunk of 64 positions and around the chunk plus a window, with
empty sequences between them; an N at both sides of the chunk seam and where the last window of the first chunk ends; a
homopolymer over two seams (the left-neighbour rule, which lane 0 of a round cannot apply); 5,000 short sequences, more than an
insert grid has waves, each with a key of its own behind a prefix they share (so that a sequence no wave walked is a key less,
and the shared keys are settled by many waves at once); and all of it behind 37 bytes the offsets do not reference."""
import numpy as np
import pytest

import alleles_cases as ac
import genes_cases as gc
import iso_cases as ic
from badger_amd import _native
from badger_amd import alleles as al
from badger_amd import discover as ds
from badger_amd import genes as gn

pytestmark = pytest.mark.gpu

LEAD = 37
N_FEATURES, N_VARIANTS, N_SHORT = 8, 40, 5000
EMPTY_TABLE = [0, 0, 0, 64, 0, 0]


def _sequences(k):
    rng = np.random.default_rng(4300 + k)
    seqs = []
    for n in (k - 1, k, k + 1, 63, 64, 65, 64 + k - 1, 64 + k, 128 + k):
        seqs += [gc.rand_seq(rng, n), ""]
    seam = list(gc.rand_seq(rng, 200))
    for p in (63, 64, 64 + k - 1):
        seam[p] = "N"
    seqs += ["".join(seam), "A" * 150]
    prefix = gc.rand_seq(rng, k - 4)                               # k + 3 bases each: four windows, the last one the sequence's own
    seqs += [prefix + "".join("ACGT"[(q >> (2 * d)) & 3] for d in range(6, -1, -1)) for q in range(N_SHORT)]
    return seqs, gc.rand_seq(rng, LEAD).encode(), gc.rand_seq(rng, 50).encode()


def _flat(seqs, lead=b"", tail=b""):
    flat = [s.encode() for s in seqs]
    return (np.frombuffer(lead + b"".join(flat) + tail, dtype=np.uint8),
            (len(lead) + np.concatenate([[0], np.cumsum([len(s) for s in flat], dtype=np.int64)])).astype(np.uint64))


@pytest.fixture(scope="module", params=(11, 21, 31))
def case(request):
    """the sequences of one k, what every table is built from, and the checkers' figures and records: computed once"""
    k = request.param
    seqs, lead, tail = _sequences(k)
    n = len(seqs)
    feats = (np.arange(n) % N_FEATURES).astype(np.uint32)
    local = gn.local_indices(feats)[0]
    values = (np.arange(n) % (2 * N_VARIANTS)).astype(np.uint32)
    var_genes = (np.arange(N_VARIANTS) % N_FEATURES).astype(np.uint32)
    index = gn.build_index(seqs, feats, k, local)
    a_index = al.build_index(seqs, values, var_genes, N_FEATURES, k)
    s_index = ds.build_index(seqs, feats, k)
    gene = gn.assign_reads(index, seqs, 1)
    a_recs = ac.gene_recs(var_genes[values >> 1])                  # every sequence as a read of its own variant's gene
    s_recs = ac.gene_recs(feats)                                   # ... and of its own feature
    want = dict(stats=[int(x) for x in index.stats()], a_stats=[int(x) for x in a_index.stats()[0]], kpv=a_index.stats()[1].tolist(),
                s_stats=[int(x) for x in s_index.stats()], gene=gc.rec_tuples(gene),
                iso=ic.iso_tuples(gn.iso_assign_reads(index, seqs, gene, 1)), alleles=al.assign_reads(a_index, seqs, a_recs),
                counts=ds.pileup(s_index, seqs, s_recs))
    # the case says something: keys of one feature and keys of several, isoform calls, allele records, evidence
    assert 0 < want["stats"][2] < want["stats"][1] and want["stats"][1] > N_SHORT and want["stats"][3] >= 2 * want["stats"][0]
    assert sum(g[0] != gn.NONE for g in want["gene"]) > N_SHORT // 2 and any(i[0] for i in want["iso"])
    assert len(want["alleles"][0]) > N_SHORT // 2 and want["alleles"][1] == 0 and int(want["counts"].sum()) > 0
    return dict(k=k, seqs=seqs, lead=lead, tail=tail, feats=feats, local=local, values=values, var_genes=var_genes, a_recs=a_recs,
                s_recs=s_recs, want=want)


@pytest.fixture()
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def test_genes_and_sites_tables(ctx, case):
    k, want = case["k"], case["want"]
    bases, off = _flat(case["seqs"], case["lead"], case["tail"])
    assert int(off[0]) == LEAD
    ctx.genes_index_build(bases, off, case["feats"], k)            # k_genes_insert, k_genes_stats
    assert ctx.genes_index_stats().tolist() == want["stats"]
    assert gc.rec_tuples(ctx.genes_assign(bases, off, 1)) == want["gene"]
    ctx.genes_index_build_iso(bases, off, case["feats"], case["local"], k)   # ... and k_iso_insert
    assert ctx.genes_index_stats().tolist() == want["stats"]
    gene, iso = ctx.iso_assign(bases, off, 1, 1)
    assert gc.rec_tuples(gene) == want["gene"] and ic.iso_tuples(iso) == want["iso"]
    ctx.sites_index_build(bases, off, case["feats"], k)            # k_sites_insert, k_sites_stats
    assert ctx.sites_index_stats().tolist() == want["s_stats"]
    # the same key set in both tables: under linear probing the occupied slots do not depend on what else a slot holds
    assert ctx.sites_index_stats().tolist() == ctx.genes_index_stats().tolist()
    ctx.sites_pileup(bases, off, case["s_recs"])
    counts = ctx.sites_counts()
    assert counts.shape == (int(off[-1]), 4) and not counts[:LEAD].any()          # (a site is a position of the caller's buffer)
    assert (counts[LEAD:] == want["counts"]).all()


def test_alleles_table(ctx, case):
    k, want = case["k"], case["want"]
    bases, off = _flat(case["seqs"], case["lead"], case["tail"])
    ctx.alleles_index_build(bases, off, case["values"], case["var_genes"], N_FEATURES, k)   # k_alleles_insert, k_alleles_stats
    stats, per_value = ctx.alleles_index_stats()
    assert stats.tolist() == want["a_stats"] and per_value.tolist() == want["kpv"]
    recs, crowded = ctx.alleles_assign(bases, off, case["a_recs"])
    assert (recs.tolist(), crowded) == (want["alleles"][0].tolist(), want["alleles"][1])


def test_no_sequences(ctx, case):
    k = case["k"]
    bases, off = _flat(case["seqs"][:30], case["lead"])
    none_u32 = np.zeros(0, np.uint32)
    at = off[:1]                                                   # n_seqs = 0: one offset, 37, and bases nobody may read
    ctx.genes_index_build(bases, at, none_u32, k)
    ctx.alleles_index_build(bases, at, none_u32, case["var_genes"], N_FEATURES, k)
    ctx.sites_index_build(bases, at, none_u32, k)
    assert [int(x) for x in gn.build_index([], [], k).stats()] == EMPTY_TABLE
    assert ctx.genes_index_stats().tolist() == EMPTY_TABLE and ctx.sites_index_stats().tolist() == EMPTY_TABLE
    stats, per_value = ctx.alleles_index_stats()
    assert stats.tolist() == EMPTY_TABLE and per_value.tolist() == [0] * (2 * N_VARIANTS)
    ctx.genes_index_build_iso(bases, at, none_u32, np.zeros(0, np.uint8), k)
    assert ctx.genes_index_stats().tolist() == EMPTY_TABLE
    gene, iso = ctx.iso_assign(bases, off, 1, 1)
    assert not (gene["flags"] & gn.ASSIGNED).any() and (gene["n_found"] == 0).all() and (iso["flags"] == gn.ISO_NOGENE).all()
    assert ctx.alleles_assign(bases, off, case["a_recs"][:30])[0].tolist() == []
    ctx.sites_pileup(bases, off, case["s_recs"][:30])
    assert ctx.sites_counts().shape == (LEAD, 4) and not ctx.sites_counts().any()


# The refusals every build shares, as the library worded them before the builds shared their checks.
@pytest.mark.parametrize("build, prefix", (("genes", "genes"), ("genes_iso", "genes"), ("alleles", "alleles"), ("sites", "sites")))
def test_refusal_texts(ctx, build, prefix):
    k = 15
    seqs = [gc.rand_seq(np.random.default_rng(5), 40) for _ in range(3)]
    bases, off = _flat(seqs)
    u32, local, lib, h = np.arange(3, dtype=np.uint32), np.zeros(3, np.uint8), ctx.lib, ctx.h

    def call(bases_p=bases.ctypes.data, off_p=off.ctypes.data, per_seq_p=u32.ctypes.data, k=k):
        if build == "genes":
            return lib.bdg_genes_index_build(h, bases_p, off_p, 3, per_seq_p, k)
        if build == "genes_iso":
            return lib.bdg_genes_index_build_iso(h, bases_p, off_p, 3, per_seq_p, local.ctypes.data, k)
        if build == "alleles":
            return lib.bdg_alleles_index_build(h, bases_p, off_p, 3, per_seq_p, u32.ctypes.data, 2, 3, k)
        return lib.bdg_sites_index_build(h, bases_p, off_p, 3, per_seq_p, k)

    down = off[[0, 2, 1, 3]].copy()
    for kw, text in ((dict(k=10), prefix + ": k out of range (11 .. 31)"), (dict(k=32), prefix + ": k out of range (11 .. 31)"),
                     (dict(off_p=down.ctypes.data), prefix + ": sequence offsets must be non-decreasing"),
                     (dict(off_p=None), "null pointer"), (dict(per_seq_p=None), "null pointer"), (dict(bases_p=None), "null pointer")):
        assert call(**kw) == _native.E_ARG, kw
        assert lib.bdg_last_error(h).decode() == text, kw
    stats = {"alleles": lambda: lib.bdg_alleles_index_stats(h, np.zeros(6, np.uint64).ctypes.data, None),
             "sites": lambda: lib.bdg_sites_index_stats(h, np.zeros(6, np.uint64).ctypes.data)}
    stats = stats.get(build, lambda: lib.bdg_genes_index_stats(h, np.zeros(6, np.uint64).ctypes.data))
    built = {"alleles": "bdg_alleles_index_build", "sites": "bdg_sites_index_build"}.get(build, "bdg_genes_index_build")
    assert stats() == _native.E_ARG and lib.bdg_last_error(h).decode() == "%s: no index built (%s)" % (prefix, built)
    assert call() == 0 and stats() == 0
