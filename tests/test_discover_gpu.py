"""The discovery kernels (csrc/discover_kernels.hip) against the rule of badger_amd/discover.py: the counts as whole arrays, the
selected records as sorted sets, all six stats of the table.  k = 11, 15, 31; a substitution at every position of a 700-base
transcript, which moves the enclosed base and its partner across every lane, chunk border and step border; read lengths 0, 2k,
2k + 1, 2k + 2 and around one and two steps; the hand-derived cases (N at the site and in a flank, another gene's read, a key in two
genes, two isoforms with a shared exon, a key repeated inside its gene); lower-case poison under reads that are not ASSIGNED;
64-slot tables with a wrap; one key written by 4,096 waves; 20,000 reads on one 300-base transcript; two calls against one, and
the reset; 0, 1 and 20,000 reads; capacity one below, at and one above the count; the same reads twice and shuffled; each of the
three tables beside a build of another; every argument error over poisoned outputs."""
import numpy as np
import pytest

import discover_cases as dc
import genes_cases as gc
from badger_amd import _native
from badger_amd import alleles as al
from badger_amd import discover as dv
from badger_amd import genes as gn

pytestmark = pytest.mark.gpu

KS = (11, 15, 31)
POISON = 0xABABABAB


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _flat(seqs):
    flat = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    return (np.frombuffer(b"".join(flat), dtype=np.uint8),
            np.concatenate([[0], np.cumsum([len(s) for s in flat], dtype=np.int64)]).astype(np.uint64))


def _build(ctx, seqs, feats, k):
    """the site table on the device and in the checker; the six stats compared -> the checker's index"""
    ctx.sites_index_build(*_flat(seqs), feats, k)
    index = dv.build_index(seqs, feats, k)
    assert tuple(int(x) for x in ctx.sites_index_stats()) == tuple(index.stats())
    assert not ctx.sites_counts().any()
    return index


def _check(ctx, index, reads, recs, what, thresholds=((1, 1), (2, 200000))):
    """one call on fresh counts against the checker: the counts as arrays, the selection as sorted records -> the counts"""
    ctx.sites_reset()
    ctx.sites_pileup(*_flat(reads), recs)
    want = dv.pileup(index, reads, recs)
    got = ctx.sites_counts()
    assert got.shape == want.shape and np.array_equal(got, want), what
    for min_alt, ppm in thresholds:
        sel = ctx.sites_select(min_alt, ppm)
        assert np.array_equal(sel.view(np.uint32), dv.select(index, want, min_alt, ppm).view(np.uint32)), (what, min_alt, ppm)
    return want


@pytest.mark.parametrize("k", KS)
def test_random_small_cases(ctx, k):
    rng = np.random.default_rng(7000 + k)
    seen = 0
    for i in range(30):
        seqs, feats, reads, recs = dc.small_case(rng, k)
        seen += int(_check(ctx, _build(ctx, seqs, feats, k), reads, recs, "case %d" % i).sum())
    assert seen > 300


@pytest.mark.parametrize("k", KS)
def test_hand_derived_cases(ctx, k):
    for name, c in dc.hand_cases(k).items():
        index = _build(ctx, c["seqs"], c["features"], k)
        got = _check(ctx, index, c["reads"], c["recs"], name)
        assert {int(s): got[s].tolist() for s in np.flatnonzero(got.sum(axis=1))} == c["want"], name


@pytest.mark.parametrize("k", KS)
def test_a_substitution_at_every_position(ctx, k):
    seqs, feats, reads, recs = dc.scan_case(k)
    index = _build(ctx, seqs, feats, k)
    want = _check(ctx, index, reads, recs, "scan")
    # from the rule: read p gives every site k .. 699 - k further than k from p its own letter, and p the new one
    sites = np.arange(k, 700 - k)
    depth = want.sum(axis=1)
    assert (depth[:k] == 0).all() and (depth[700 - k:] == 0).all()
    assert (depth[sites] == 700 - (np.minimum(sites + k, 699) - np.maximum(sites - k, 0) + 1) + 1).all()
    assert len(dv.select(index, want, 1, 1)) == 700 - 2 * k
    # every read alone: the single pair at its substitution, wherever it falls in the wave
    for p in (0, k - 1, k, 63 - k, 64, 255 - k, 256 - k - 1, 256 - k, 256, 2 * (256 - k - 1), 511, 512, 699 - k, 700 - k, 699):
        _check(ctx, index, reads[p:p + 1], recs[:1], "read %d" % p, ((1, 1),))


@pytest.mark.parametrize("k", KS)
def test_read_lengths(ctx, k):
    seqs, feats, reads, recs = dc.length_case(k)
    index = _build(ctx, seqs, feats, k)
    want = _check(ctx, index, reads, recs, "lengths")
    assert want.sum() > 3000
    for i in range(len(reads)):
        _check(ctx, index, reads[i:i + 1], recs[:1], "length %d" % len(reads[i]), ((1, 1),))


def test_reads_that_take_no_part(ctx):
    """What tests the gate are the upper-case reads: gene 0's text given to gene 1 and in a read that is not ASSIGNED - without the
    gate both would count.  The lower-case reads only stand where such reads stand (lower-case letters code as N); that nothing of
    a skipped read is loaded is what the kernel's `continue` in front of the first load says."""
    rng = np.random.default_rng(8)
    t, u = gc.rand_seq(rng, 150), gc.rand_seq(rng, 150)
    index = _build(ctx, [t, u], np.array([0, 1], dtype=np.uint32), 15)
    reads = [t, t.lower(), t, t, gc.rand_seq(rng, 300).lower(), u]
    recs = dc.gene_recs([0, 0, 1, 0, 1, 1], [True, False, True, False, False, True])
    want = _check(ctx, index, reads, recs, "gate")
    assert int(want.sum()) == 2 * (150 - 30) and int(want[:150].sum()) == 120


def test_64_slot_tables_with_a_wrap(ctx):
    """one transcript of 2k + 10 bases at k = 11: 22 windows, 64 slots; among 300 random ones some keep a key in front of its home"""
    rng = np.random.default_rng(64)
    wrapped = 0
    for _ in range(300):
        t = gc.rand_seq(rng, 32)
        stats = dv.build_index([t], [0], 11).stats()
        assert stats[3] == 64
        if not stats[5]:
            continue
        wrapped += 1
        index = _build(ctx, [t], np.zeros(1, np.uint32), 11)
        assert _check(ctx, index, [t, dc._sub(t, 16)], dc.gene_recs([0, 0]), "wrap", ((1, 1),)).sum() == 10 + 1
    print("%d tables of 64 slots with a key past the wrap" % wrapped)
    assert wrapped >= 3


def test_one_key_from_4096_waves(ctx):
    """4,096 sequences of one window each: one key, one gene, and of 4,096 atomicMin the smallest site stays"""
    text = gc.rand_seq(np.random.default_rng(4), 15)
    pad = gc.rand_seq(np.random.default_rng(5), 40)
    for feats, ambiguous in ((np.zeros(4097, np.uint32), 0), (np.arange(4097, dtype=np.uint32) % 2, 1)):
        seqs = [pad] + [text] * 4096
        index = _build(ctx, seqs, feats, 15)
        assert tuple(int(x) for x in ctx.sites_index_stats())[:3] == (26 + 4096, 27, ambiguous)
        assert int(index.site[index.keys == gn.keys_of(text, 15)[0]][0]) == 40
    # the smallest site is what the partner test sees: the key stands at site 41 of the first sequence and at 4,096 later ones; the
    # pair whose partner it is counts only if the slot holds 41
    seqs = [pad + text[:1] + text] + [text] * 4096
    index = _build(ctx, seqs, np.zeros(4097, np.uint32), 15)
    want = _check(ctx, index, [seqs[0]], dc.gene_recs([0]), "minimum")
    assert want[40].sum() == 1 and want.sum() == 56 - 30


@pytest.fixture(scope="module")
def hot():
    """20,000 reads on one 300-base transcript; one reference, shared"""
    seqs, feats, reads, recs = dc.hot_case(15)
    index = dv.build_index(seqs, feats, 15)
    return dict(seqs=seqs, feats=feats, reads=reads, recs=recs, index=index, want=dv.pileup(index, reads, recs))


def test_20000_reads_on_the_same_few_hundred_addresses(ctx, hot):
    _build(ctx, hot["seqs"], hot["feats"], 15)
    want = hot["want"]
    assert want.sum() > 4000000 and want.max() > 15000
    for _ in range(2):
        ctx.sites_reset()
        ctx.sites_pileup(*_flat(hot["reads"]), hot["recs"])
        assert np.array_equal(ctx.sites_counts(), want)
    order = np.random.default_rng(1).permutation(len(hot["reads"]))
    ctx.sites_reset()
    ctx.sites_pileup(*_flat([hot["reads"][i] for i in order]), hot["recs"][order])
    assert np.array_equal(ctx.sites_counts(), want)
    sel = ctx.sites_select(5, 1000)
    assert np.array_equal(sel.view(np.uint32), dv.select(hot["index"], want, 5, 1000).view(np.uint32)) and len(sel) > 200


def test_calls_accumulate_and_reset_clears(ctx, hot):
    index = _build(ctx, hot["seqs"], hot["feats"], 15)
    reads, recs = hot["reads"][:3000], hot["recs"][:3000]
    whole = dv.pileup(index, reads, recs)
    ctx.sites_pileup(*_flat(reads[:1000]), recs[:1000])
    first = ctx.sites_counts()
    assert np.array_equal(first, dv.pileup(index, reads[:1000], recs[:1000]))
    ctx.sites_pileup(*_flat(reads[1000:]), recs[1000:])
    assert np.array_equal(ctx.sites_counts(), whole)
    # none and one read add nothing and one read's
    ctx.sites_pileup(np.zeros(0, np.uint8), np.zeros(1, np.uint64), recs[:0])
    assert np.array_equal(ctx.sites_counts(), whole)
    ctx.sites_pileup(*_flat(reads[:1]), recs[:1])
    assert np.array_equal(ctx.sites_counts(), dv.pileup(index, reads[:1], recs[:1], whole.copy()))
    ctx.sites_reset()
    assert not ctx.sites_counts().any() and len(ctx.sites_select(1, 1)) == 0
    # the device form: device arrays, the same counts
    bases, off = _flat(reads)
    d = [_native.DeviceArray.from_host(ctx, a) for a in (bases, off, np.ascontiguousarray(recs, dtype=_native.GENE_DTYPE).view(np.uint32))]
    try:
        ctx.sites_pileup_dev(d[0], d[1], len(reads), d[2])
        ctx.sites_pileup_dev(d[0], d[1], 0, d[2])
        assert np.array_equal(ctx.sites_counts(), whole)
    finally:
        for a in d:
            a.free()


def test_capacity(ctx, hot):
    _build(ctx, hot["seqs"], hot["feats"], 15)
    ctx.sites_pileup(*_flat(hot["reads"]), hot["recs"])
    want = dv.select(hot["index"], hot["want"], 1, 1)
    count = len(want)
    assert count == 270
    lib, h = ctx.lib, ctx.h
    n = np.zeros(1, dtype=np.uint64)
    for cap in (count - 1, count, count + 1, 0):
        out = np.full((cap + 1) * 8, POISON, np.uint32)
        rc = lib.bdg_sites_select(h, 1, 1, out.ctypes.data if cap else None, cap, n.ctypes.data)
        assert int(n[0]) == count and rc == (0 if cap >= count else _native.E_CAPACITY), cap
        assert (out[cap * 8:] == POISON).all(), "a store behind the capacity"
        if cap >= count:
            got = out[:count * 8].view(_native.SITE_DTYPE)
            assert np.array_equal(got[np.argsort(got["site"])].view(np.uint32), want.view(np.uint32))
            assert (out[count * 8:] == POISON).all()
    with pytest.raises(_native.BadgerHipError) as e:
        ctx.sites_select(1, 1, cap=count - 1, retry=False)
    assert e.value.code == _native.E_CAPACITY and e.value.n_records == count
    assert np.array_equal(ctx.sites_select(1, 1, cap=1).view(np.uint32), want.view(np.uint32))          # the retry with the count


def test_the_three_tables_do_not_touch_each_other(ctx):
    rng = np.random.default_rng(77)
    tx = [gc.rand_seq(rng, 400) for _ in range(12)]
    feat = np.arange(12, dtype=np.uint32)
    reads = [dc._sub(tx[i % 12], 100 + i)[50:350] for i in range(200)]
    places = [(g, 150) for g in range(12)]
    variants = al.Variants(["v%d" % g for g, _ in places], [tx[g][p] for g, p in places], [dc.other_letter(rng, tx[g][p]) for g, p in places],
                           [g for g, _ in places], [(i, g, p) for i, (g, p) in enumerate(places)])
    tx_seqs = [t.encode() for t in tx]

    def genes_state():
        return ctx.genes_index_stats().tolist(), ctx.genes_assign(*_flat(reads), 3).tolist()

    def alleles_state(recs):
        return [x.tolist() for x in ctx.alleles_index_stats()], ctx.alleles_assign(*_flat(reads), recs)[0].tolist()

    def sites_state(recs):
        ctx.sites_reset()
        ctx.sites_pileup(*_flat(reads), recs)
        return ctx.sites_index_stats().tolist(), ctx.sites_counts().tolist()

    ctx.genes_index_build(*_flat(tx), feat, 21)
    recs = ctx.genes_assign(*_flat(reads), 3)
    assert (recs["flags"] == gn.ASSIGNED).all()
    seqs, values = al.allele_sequences(variants, tx_seqs, 15)
    ctx.alleles_index_build(*_flat(seqs), values, variants.gene, 12, 15)
    index = _build(ctx, tx_seqs, feat, 11)
    g0, a0, s0 = genes_state(), alleles_state(recs), sites_state(recs)
    assert s0[1] == dv.pileup(index, reads, recs).tolist() and len(a0[1]) > 100       # the device's own gene records gate the same way
    other = [gc.rand_seq(rng, 300) for _ in range(5)]
    # a new genes table: the other two stay
    ctx.genes_index_build(*_flat(other), np.arange(5, dtype=np.uint32), 11)
    assert alleles_state(recs) == a0 and sites_state(recs) == s0
    ctx.genes_index_build(*_flat(tx), feat, 21)
    # a new allele table
    al.drop_index(ctx)
    assert genes_state() == g0 and sites_state(recs) == s0
    ctx.alleles_index_build(*_flat(seqs), values, variants.gene, 12, 15)
    # a new site table, then the empty one: 64 slots, no sites, the other two as they were
    ctx.sites_index_build(*_flat(other), np.arange(5, dtype=np.uint32), 31)
    assert genes_state() == g0 and alleles_state(recs) == a0
    dv.drop_index(ctx)
    assert ctx.sites_index_stats().tolist() == [0, 0, 0, 64, 0, 0] and ctx.sites_counts().shape == (0, 4)
    ctx.sites_pileup(*_flat(reads), recs)
    assert len(ctx.sites_select(1, 1)) == 0
    assert genes_state() == g0 and alleles_state(recs) == a0


def test_argument_errors(hot):
    ctx = _native.Context(0)
    try:
        reads, recs = hot["reads"][:4], np.ascontiguousarray(hot["recs"][:4], dtype=_native.GENE_DTYPE)
        bases, off = _flat(reads)
        out, count = np.full(64, POISON, np.uint32), np.full(2, POISON, np.uint32)
        counts = np.full(1200, POISON, np.uint32)
        lib, h = ctx.lib, ctx.h
        d = _native.DeviceArray.from_host(ctx, np.full(64, POISON, np.uint32))
        # no site index yet
        assert lib.bdg_sites_pileup(h, bases.ctypes.data, off.ctypes.data, 4, recs.ctypes.data) == _native.E_ARG
        assert b"no index built" in lib.bdg_last_error(h)
        assert lib.bdg_sites_pileup_dev(h, d.ptr, d.ptr, 1, d.ptr) == _native.E_ARG
        assert lib.bdg_sites_index_stats(h, out.ctypes.data) == _native.E_ARG
        assert lib.bdg_sites_reset(h) == _native.E_ARG
        assert lib.bdg_sites_select(h, 1, 1, out.ctypes.data, 2, count.ctypes.data) == _native.E_ARG
        assert lib.bdg_sites_counts_to_host(h, counts.ctypes.data, 300) == _native.E_ARG
        sb, so = _flat(hot["seqs"])
        feats = np.zeros(1, np.uint32)

        def build(sb_p=sb.ctypes.data, so_p=so.ctypes.data, n=1, feats_p=feats.ctypes.data, k=15):
            return lib.bdg_sites_index_build(h, sb_p, so_p, n, feats_p, k)

        for kw in (dict(k=10), dict(k=32), dict(so_p=None), dict(feats_p=None), dict(sb_p=None)):
            assert build(**kw) == _native.E_ARG, kw
        for reserved in (gn.AMBIGUOUS, gn.NONE):
            assert build(feats_p=np.array([reserved], dtype=np.uint32).ctypes.data) == _native.E_ARG
        assert b"feature id reserved" in lib.bdg_last_error(h)
        assert build(so_p=np.array([300, 0], dtype=np.uint64).ctypes.data) == _native.E_ARG
        assert build(so_p=np.array([0, 0xFFFFFFFF], dtype=np.uint64).ctypes.data) == _native.E_ARG     # 2^32 - 1 bases: refused unread
        assert b"a site is a uint32" in lib.bdg_last_error(h)
        assert lib.bdg_sites_index_stats(h, out.ctypes.data) == _native.E_ARG             # a refused build leaves no table
        assert build() == 0
        # pileup: null pointers, decreasing offsets, a reserved feature in an ASSIGNED record; nothing is counted
        good = (bases.ctypes.data, off.ctypes.data, 4, recs.ctypes.data)
        for i in (0, 1, 3):
            args = list(good)
            args[i] = None
            assert lib.bdg_sites_pileup(h, *args) == _native.E_ARG, i
        bad = off.copy()
        bad[2] = bad[1] - 1
        assert lib.bdg_sites_pileup(h, bases.ctypes.data, bad.ctypes.data, 4, recs.ctypes.data) == _native.E_ARG
        for reserved in (gn.AMBIGUOUS, gn.NONE):
            wrong = recs.copy()
            wrong["feature"][2] = reserved
            assert lib.bdg_sites_pileup(h, bases.ctypes.data, off.ctypes.data, 4, wrong.ctypes.data) == _native.E_ARG
            wrong["flags"][2] = gn.LOW                                                     # (a record that is not ASSIGNED may hold it)
            assert lib.bdg_sites_pileup(h, bases.ctypes.data, off.ctypes.data, 4, wrong.ctypes.data) == 0
            assert lib.bdg_sites_reset(h) == 0
        for i in (1, 3):
            args = [d.ptr, d.ptr, 1, d.ptr]
            args[i] = None
            assert lib.bdg_sites_pileup_dev(h, *args) == _native.E_ARG, i
        assert (d.to_host() == POISON).all()
        assert not ctx.sites_counts(300).any()
        # select and the counts: thresholds out of range, null pointers, a misaligned output, another number of sites
        sel = (1, 1, out.ctypes.data, 2, count.ctypes.data)
        for i, v in ((0, 0), (1, 0), (1, 1000001), (2, None), (4, None), (2, out.ctypes.data + 2)):
            args = list(sel)
            args[i] = v
            assert lib.bdg_sites_select(h, *args) == _native.E_ARG, (i, v)
        assert b"aligned to 4 bytes" in lib.bdg_last_error(h)
        assert (out == POISON).all() and (count == POISON).all()
        assert lib.bdg_sites_select(h, 1, 1, None, 0, count.ctypes.data) == 0 and count.view(np.uint64)[0] == 0
        assert lib.bdg_sites_index_stats(h, None) == _native.E_ARG
        for n_sites in (299, 301):
            assert lib.bdg_sites_counts_to_host(h, counts.ctypes.data, n_sites) == _native.E_ARG
        assert lib.bdg_sites_counts_to_host(h, None, 300) == _native.E_ARG
        assert (counts == POISON).all()
        assert lib.bdg_sites_pileup(h, *good) == 0 and lib.bdg_sites_counts_to_host(h, counts.ctypes.data, 300) == 0
        assert np.array_equal(counts.reshape(300, 4), dv.pileup(hot["index"], reads, recs))
        d.free()
    finally:
        ctx.close()
