"""The allele kernels (csrc/alleles_kernels.hip) against the rule of badger_amd/alleles.py: the records as sorted sets, the two
counts exactly, all six stats of the table and the usable keys per value.  k = 11, 15, 31; read lengths 0 .. 300 and around the
256 windows of each of the four chunks a wave has in flight; the hand-derived cases; 64-slot tables with a wrap; one key written by
4,096 waves; 256 against 257 variants in one read; reads whose gene has no variant; 0, 1 and 20,000 reads - more than waves in
flight; 16,384 reads of 153 records or more, so that every wave flushes its staging area before its second read; capacity one
below, at and one above the count; the same reads twice and shuffled; a small call behind a large one; the genes table beside the
allele table; every argument error over poisoned outputs."""
import numpy as np
import pytest

import alleles_cases as ac
import genes_cases as gc
from badger_amd import _native
from badger_amd import alleles as al
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


def _build(ctx, variants, tx_seqs, n_features, k):
    """the allele table on the device and in the checker; the six stats and the keys per value compared -> the checker's index"""
    seqs, values = al.allele_sequences(variants, tx_seqs, k)
    ctx.alleles_index_build(*_flat(seqs), values, variants.gene, n_features, k)
    index = al.build_index(seqs, values, variants.gene, n_features, k)
    stats, per_value = ctx.alleles_index_stats()
    want, want_per_value = index.stats()
    assert tuple(int(x) for x in stats) == tuple(want)
    assert per_value.tolist() == want_per_value.tolist()
    return index


def _dev(ctx, reads, recs, cap):
    """bdg_alleles_assign_dev over device arrays, the outputs poisoned first -> (records up to cap as stored, counts)"""
    bases, off = _flat(reads)
    n = len(reads)
    d = [_native.DeviceArray.from_host(ctx, a) for a in (bases, off, np.ascontiguousarray(recs, dtype=_native.GENE_DTYPE).view(np.uint32),
                                                         np.full((cap + 1) * 4, POISON, np.uint32), np.full(4, POISON, np.uint32))]
    try:
        ctx.alleles_assign_dev(d[0], d[1], n, d[2], d[3], cap, d[4])
        counts = d[4].to_host().view(np.uint64)
        out = d[3].to_host().view(_native.ALLELE_DTYPE)
        assert (out[cap:].view(np.uint32) == POISON).all(), "a store behind the capacity"
        return out[:cap], (int(counts[0]), int(counts[1]))
    finally:
        for a in d:
            a.free()


def _check(ctx, index, reads, recs, what):
    want, want_crowded = al.assign_reads(index, reads, recs)
    got, crowded = ctx.alleles_assign(*_flat(reads), recs)
    assert got.tolist() == want.tolist(), what
    assert crowded == want_crowded, what
    return want


@pytest.mark.parametrize("k", KS)
def test_random_small_cases(ctx, k):
    rng = np.random.default_rng(9000 + k)
    records = 0
    for i in range(40):
        case = ac.small_case(rng, k)
        index = _build(ctx, case["variants"], case["tx_seqs"], len(case["names"]), k)
        records += len(_check(ctx, index, case["reads"], case["recs"], "case %d" % i))
    assert records > 50


@pytest.mark.parametrize("k", KS)
def test_hand_derived_cases(ctx, k):
    for case in ac.hand_cases(k):
        _build(ctx, case["variants"], case["tx_seqs"], len(case["names"]), k)
        stats, per_value = ctx.alleles_index_stats()
        assert per_value.tolist() == case["per_value"] and int(stats[2]) == case["ambiguous"], case["name"]
        got, crowded = ctx.alleles_assign(*_flat(case["reads"]), case["recs"])
        assert ac.rec_tuples(got) == case["want"] and crowded == 0, case["name"]


@pytest.mark.parametrize("k", KS)
def test_read_lengths(ctx, k):
    """every length 0 .. 300 and the lengths at which a read's last window is the last of a chunk of 256 windows, one less and
    one more: prefixes and suffixes of a gene with a site every 40 bases, so that the last windows of a read carry one"""
    rng = np.random.default_rng(50 + k)
    t = gc.rand_seq(rng, 1100)
    places = list(range(7, 1100, 40))
    variants = al.Variants(["s%d" % i for i in range(len(places))], [t[p] for p in places], [ac.other_letter(rng, t[p]) for p in places],
                           [0] * len(places), [(i, 0, p) for i, p in enumerate(places)])
    index = _build(ctx, variants, [t.encode()], 1, k)
    hap = ac.with_alleles(t, [(p, variants.ref[i], variants.alt[i]) for i, p in enumerate(places)], rng.integers(0, 2, size=len(places)))
    lengths = list(range(301)) + [c * 256 + k - 1 + d for c in (1, 2, 3, 4) for d in (-1, 0, 1)]
    reads = [hap[:n] for n in lengths] + [hap[-n:] if n else "" for n in lengths]
    want = _check(ctx, index, reads, ac.gene_recs([0] * len(reads)), "lengths")
    assert len(want) > 1000


def test_64_slot_tables_with_a_wrap(ctx):
    """one variant, 2 k windows at k = 11: 64 slots; among 300 random ones some keep a key in front of its home slot"""
    rng = np.random.default_rng(64)
    wrapped = 0
    for _ in range(300):
        t = gc.rand_seq(rng, 30)
        variants = al.Variants(["w"], [t[15]], [ac.other_letter(rng, t[15])], [0], [(0, 0, 15)])
        seqs, values = al.allele_sequences(variants, [t.encode()], 11)
        stats = al.build_index(seqs, values, variants.gene, 1, 11).stats()[0]
        assert stats[3] == 64
        if not stats[5]:
            continue
        wrapped += 1
        index = _build(ctx, variants, [t.encode()], 1, 11)
        _check(ctx, index, [t, t[:15] + variants.alt[0] + t[16:]], ac.gene_recs([0, 0]), "wrap")
    print("%d tables of 64 slots with a key past the wrap" % wrapped)
    assert wrapped >= 3


def test_one_key_from_4096_waves(ctx):
    text = gc.rand_seq(np.random.default_rng(4), 15).encode()
    for values, want_per_value, want_ambiguous in ((np.ones(4096, np.uint32), [0, 1, 0, 0], 0), (np.arange(4096, dtype=np.uint32) % 2 + 2, [0, 0, 0, 0], 1)):
        ctx.alleles_index_build(*_flat([text] * 4096), values, [0, 0], 1, 15)
        stats, per_value = ctx.alleles_index_stats()
        assert tuple(int(x) for x in stats) == (4096, 1, want_ambiguous, 8192, 1, 0) and per_value.tolist() == want_per_value
    got, crowded = ctx.alleles_assign(*_flat([text]), ac.gene_recs([0]))
    assert len(got) == 0 and crowded == 0                   # (the key is ambiguous now)


def test_256_and_257_variants_in_one_read(ctx):
    rng = np.random.default_rng(5)
    for n, want_records, want_crowded in ((256, 256, 0), (257, 0, 1)):
        t, variants = ac.crowded_case(rng, 11, n)
        index = _build(ctx, variants, [t.encode()], 1, 11)
        reads = [t, t[:400], t]
        want = _check(ctx, index, reads, ac.gene_recs([0, 0, 0]), "%d variants" % n)
        got, crowded = ctx.alleles_assign(*_flat([t]), ac.gene_recs([0]))
        assert (len(got), crowded) == (want_records, want_crowded)
        assert len(want) == 2 * want_records + 36


def test_every_wave_flushes_more_than_once(ctx):
    """The flush in the middle of a wave's walk - the area written out, n_staged back to 0, the barrier in front of the refill,
    a second reservation with its own base: 16,384 reads of 153 .. 200 records each.  A wave is one of at most 32 per compute
    unit (LDS admits 22), 8,192 on 256 units, so every wave takes two reads or more, and no two of these reads fit the staging
    area of 256 records together: every wave flushes before its second read and again at its end.  Held to the checker as
    sorted sets with the exact count, and with room for half of the records."""
    rng = np.random.default_rng(31)
    t, variants = ac.crowded_case(rng, 11, 200)
    index = _build(ctx, variants, [t.encode()], 1, 11)
    shapes = [t, t[:1700], t[500:]]
    per_shape = [al.assign_reads(index, [s], ac.gene_recs([0]))[0] for s in shapes]
    assert [len(e) for e in per_shape] == [200, 154, 155]
    n = 16384
    reads = [shapes[i % 3] for i in range(n)]
    parts = []
    for s, e in enumerate(per_shape):
        which = np.arange(s, n, 3, dtype=np.uint32)
        part = np.tile(e, len(which))
        part["read"] = np.repeat(which, len(e))
        parts.append(part)
    want = np.concatenate(parts)
    want = want[np.lexsort((want["variant"], want["read"]))]
    recs = ac.gene_recs([0] * n)
    got, crowded = ctx.alleles_assign(*_flat(reads), recs, cap=len(want))
    assert crowded == 0 and len(got) == len(want)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # room for half of them: the count stays exact, every place below the capacity holds a record of the call, none twice
    cap = len(want) // 2
    stored, counts = _dev(ctx, reads, recs, cap)
    assert counts == (len(want), 0)
    key = lambda r: (r["read"].astype(np.uint64) << np.uint64(32)) | r["variant"].astype(np.uint64)  # noqa: E731
    stored = stored[np.argsort(key(stored))]
    assert len(np.unique(key(stored))) == cap
    at = np.searchsorted(key(want), key(stored))
    assert (at < len(want)).all() and np.array_equal(want[np.minimum(at, len(want) - 1)].view(np.uint32), stored.view(np.uint32))


def test_reads_of_genes_without_a_variant(ctx):
    """gene 1 has no variant.  What tests the gate are the upper-case reads: gene 0's text in a read given to gene 1, and in one
    given to feature 7, an id beyond the allele table's features (the genes table may know more genes) - without the gate both
    would give gene 0's record.  The lower-case reads only stand where reads of such genes stand: lower-case letters code as N
    and would give no record with or without the gate, so they do not show that nothing of a skipped read is loaded - no test
    here can; the kernel's `continue` in front of the first load is what says so."""
    rng = np.random.default_rng(6)
    t = gc.rand_seq(rng, 120)
    variants = al.Variants(["v"], [t[60]], [ac.other_letter(rng, t[60])], [0], [(0, 0, 60)])
    index = _build(ctx, variants, [t.encode()], 2, 15)
    reads = [t, t.lower(), t, t, gc.rand_seq(rng, 300).lower()]
    recs = ac.gene_recs([0, 1, 1, 7, 1])
    want = _check(ctx, index, reads, recs, "no variant")
    assert ac.rec_tuples(want) == [(0, 0, 15, 0)]


@pytest.fixture(scope="module")
def large(ctx):
    """20,000 reads of 40 genes, 30 of them with 8 sites each; one reference, shared"""
    rng = np.random.default_rng(20000)
    tx, ids, ref, alt, gene, occ, sites = [], [], [], [], [], [], []
    for g in range(40):
        t = gc.rand_seq(rng, 400)
        tx.append(t)
        sites.append([])
        if g % 4 == 3:
            continue
        for p in sorted(int(x) for x in rng.choice(400, size=8, replace=False)):
            occ.append((len(ids), g, p))
            ids.append("v%d" % len(ids))
            ref.append(t[p])
            alt.append(ac.other_letter(rng, t[p]))
            gene.append(g)
            sites[-1].append((p, ref[-1], alt[-1]))
    variants = al.Variants(ids, ref, alt, gene, occ)
    reads, feats = [], []
    for _ in range(20000):
        g = int(rng.integers(0, 40))
        text = ac.with_alleles(tx[g], sites[g], rng.integers(0, 2, size=len(sites[g])))
        a = int(rng.integers(0, 250))
        reads.append(text[a:a + int(rng.integers(20, 151))])
        feats.append(g)
    recs = ac.gene_recs(feats, rng.random(20000) < 0.95)
    tx_seqs = [t.encode() for t in tx]
    index = al.build_index(*al.allele_sequences(variants, tx_seqs, 15), variants.gene, 40, 15)
    want, crowded = al.assign_reads(index, reads, recs)
    assert crowded == 0 and len(want) > 20000               # (a few dozen records a wave: one flush each, at its end)
    return dict(variants=variants, tx_seqs=tx_seqs, reads=reads, recs=recs, want=want)


def test_many_reads_twice_and_shuffled(ctx, large):
    _build(ctx, large["variants"], large["tx_seqs"], 40, 15)
    want = large["want"]
    for _ in range(2):
        got, crowded = ctx.alleles_assign(*_flat(large["reads"]), large["recs"])
        assert got.tolist() == want.tolist() and crowded == 0
    order = np.random.default_rng(1).permutation(len(large["reads"]))
    got, crowded = ctx.alleles_assign(*_flat([large["reads"][i] for i in order]), large["recs"][order])
    got["read"] = order[got["read"]]
    assert sorted(got.tolist()) == want.tolist() and crowded == 0
    # a small call behind the large one, and none and one read
    got, _ = ctx.alleles_assign(*_flat(large["reads"][:7]), large["recs"][:7])
    assert got.tolist() == want[want["read"] < 7].tolist()
    got, crowded = ctx.alleles_assign(*_flat(large["reads"][:1]), large["recs"][:1])
    assert got.tolist() == want[want["read"] < 1].tolist()
    got, crowded = ctx.alleles_assign(np.zeros(0, np.uint8), np.zeros(1, np.uint64), large["recs"][:0])
    assert len(got) == 0 and crowded == 0
    stored, counts = _dev(ctx, [], large["recs"][:0], 4)
    assert counts == (0, 0) and (stored.view(np.uint32) == POISON).all()


def test_capacity(ctx, large):
    _build(ctx, large["variants"], large["tx_seqs"], 40, 15)
    reads, recs = large["reads"][:3000], large["recs"][:3000]
    want = large["want"][large["want"]["read"] < 3000]
    count = len(want)
    assert count > 3000
    for cap in (count - 1, count, count + 1, 0):
        stored, counts = _dev(ctx, reads, recs, cap)
        assert counts == (count, 0), cap
        if cap >= count:
            assert sorted(stored[:count].tolist()) == want.tolist()
            assert (stored[count:].view(np.uint32) == POISON).all()
        else:                                               # what is stored is records of the call, each once
            kept = [tuple(x) for x in stored.tolist() if x[0] != POISON]
            assert len(set(kept)) == len(kept) and set(kept) <= set(want.tolist())
    with pytest.raises(_native.BadgerHipError) as e:
        ctx.alleles_assign(*_flat(reads), recs, cap=count - 1, retry=False)
    assert e.value.code == _native.E_CAPACITY and e.value.n_records == count
    got, _ = ctx.alleles_assign(*_flat(reads), recs, cap=count)
    assert got.tolist() == want.tolist()
    got, _ = ctx.alleles_assign(*_flat(reads), recs, cap=1)             # the retry with the count
    assert got.tolist() == want.tolist()


def test_the_two_tables_do_not_touch_each_other(ctx, large):
    rng = np.random.default_rng(77)
    tx = [s.decode() for s in large["tx_seqs"]]
    feat = np.arange(40, dtype=np.uint32)
    reads = large["reads"][:500]
    ctx.genes_index_build(*_flat(tx), feat, 21)
    gene_stats = ctx.genes_index_stats().tolist()
    gene_recs = ctx.genes_assign(*_flat(reads), 3)
    _build(ctx, large["variants"], large["tx_seqs"], 40, 15)
    allele_stats = [x.tolist() for x in ctx.alleles_index_stats()]
    got = ctx.alleles_assign(*_flat(reads), large["recs"][:500])[0]
    assert ctx.genes_index_stats().tolist() == gene_stats
    assert ctx.genes_assign(*_flat(reads), 3).tolist() == gene_recs.tolist()
    # the device's own gene records gate the same way as the checker's
    index = al.build_index(*al.allele_sequences(large["variants"], large["tx_seqs"], 15), large["variants"].gene, 40, 15)
    assert ctx.alleles_assign(*_flat(reads), gene_recs)[0].tolist() == al.assign_reads(index, reads, gene_recs)[0].tolist()
    # a new genes table, of other sequences and another k
    other = [gc.rand_seq(rng, 300) for _ in range(5)]
    ctx.genes_index_build(*_flat(other), np.arange(5, dtype=np.uint32), 11)
    assert [x.tolist() for x in ctx.alleles_index_stats()] == allele_stats
    assert ctx.alleles_assign(*_flat(reads), large["recs"][:500])[0].tolist() == got.tolist()
    # an empty allele build leaves 64 empty slots and the genes table alone
    al.drop_index(ctx)
    stats, per_value = ctx.alleles_index_stats()
    assert stats.tolist() == [0, 0, 0, 64, 0, 0] and len(per_value) == 0
    assert ctx.alleles_assign(*_flat(reads), large["recs"][:500])[0].tolist() == []
    assert ctx.genes_index_stats()[3] > 64


def test_argument_errors(large):
    ctx = _native.Context(0)
    try:
        bases, off = _flat(large["reads"][:4])
        recs = large["recs"][:4]
        out, counts = np.full(16, POISON, np.uint32), np.full(4, POISON, np.uint32)
        lib, h = ctx.lib, ctx.h

        def assign(bases_p, off_p, n, recs_p, out_p, cap, counts_p):
            return lib.bdg_alleles_assign(h, bases_p, off_p, n, recs_p, out_p, cap, counts_p)

        # no allele index yet
        assert assign(bases.ctypes.data, off.ctypes.data, 4, recs.ctypes.data, out.ctypes.data, 4, counts.ctypes.data) == _native.E_ARG
        assert b"no index built" in lib.bdg_last_error(h)
        d = _native.DeviceArray.from_host(ctx, counts)
        assert lib.bdg_alleles_assign_dev(h, d.ptr, d.ptr, 1, d.ptr, d.ptr, 1, d.ptr) == _native.E_ARG
        assert lib.bdg_alleles_index_stats(h, out.ctypes.data, None) == _native.E_ARG
        seqs, values = al.allele_sequences(large["variants"], large["tx_seqs"], 15)
        sb, so = _flat(seqs)
        genes = large["variants"].gene
        nv = len(genes)

        def build(sb_p=sb.ctypes.data, so_p=so.ctypes.data, n=len(values), values_p=values.ctypes.data, genes_p=genes.ctypes.data, nv=nv,
                  nf=40, k=15):
            return lib.bdg_alleles_index_build(h, sb_p, so_p, n, values_p, genes_p, nv, nf, k)

        for kw in (dict(k=10), dict(k=32), dict(nv=nv - 1), dict(nf=int(genes.max())), dict(so_p=None), dict(values_p=None), dict(genes_p=None),
                   dict(sb_p=None)):
            assert build(**kw) == _native.E_ARG, kw
        bad = so.copy()
        bad[3] = bad[2] - 1
        assert build(so_p=bad.ctypes.data) == _native.E_ARG
        assert lib.bdg_alleles_index_stats(h, out.ctypes.data, None) == _native.E_ARG     # a refused build leaves no table
        assert build() == 0
        # a build the wrapper did not make: the wrapper asks the context how many values there are
        assert len(ctx.alleles_index_stats()[1]) == 2 * nv and lib.bdg_alleles_index_values(h, None) == _native.E_ARG
        # assign: null pointers and decreasing offsets; nothing is written
        good = (bases.ctypes.data, off.ctypes.data, 4, recs.ctypes.data, out.ctypes.data, 4, counts.ctypes.data)
        for i in (0, 1, 3, 4, 6):
            args = list(good)
            args[i] = None
            assert assign(*args) == _native.E_ARG, i
        bad = off.copy()
        bad[2] = bad[1] - 1
        assert assign(bases.ctypes.data, bad.ctypes.data, 4, recs.ctypes.data, out.ctypes.data, 4, counts.ctypes.data) == _native.E_ARG
        assert (out == POISON).all()
        for i in (1, 3, 4, 6):
            args = [d.ptr, d.ptr, 1, d.ptr, d.ptr, 1, d.ptr]
            args[i] = None
            assert lib.bdg_alleles_assign_dev(h, *args) == _native.E_ARG, i
        assert lib.bdg_alleles_assign_dev(h, d.ptr, d.ptr, 1, d.ptr, d.ptr + 4, 1, d.ptr) == _native.E_ARG    # d_out not 16-byte aligned
        assert b"aligned to 16 bytes" in lib.bdg_last_error(h)
        assert (d.to_host() == POISON).all()
        assert lib.bdg_alleles_index_stats(h, None, None) == _native.E_ARG
        assert assign(*good) in (0, _native.E_CAPACITY)
        d.free()
    finally:
        ctx.close()
