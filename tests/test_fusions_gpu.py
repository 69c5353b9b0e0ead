"""k_fusion_scan (csrc/fusion_kernels.hip) against the rule of badger_amd/fusions.py, every field of every record, through
bdg_fusion_scan and bdg_fusion_scan_dev over poisoned outputs.  The hand-derived cases at k = 11, 21, 31; read lengths k - 1, k,
k + 1, 63 + k, 64 + k, 255 + k, 256 + k, 257 + k and 600 with a gene's only hit at window 0 and at the last window; last_a and
first_b on either side of a 64 and of a 256 border, A in front and behind; the gate at min_hits and one below; gated reads over
lower-case poison bytes; 256 distinct features, and 257 behind gene records of another read; 0, 1 and 20,000 reads; 64-slot tables
with a wrap; the same reads twice and shuffled; every argument error."""
import numpy as np
import pytest

import fusion_cases as fc
import genes_cases as gc
from badger_amd import _native
from badger_amd import fusions as fu
from badger_amd import genes as gn

pytestmark = pytest.mark.gpu

KS = (11, 21, 31)
POISON = 0xABABABAB
LENGTHS = lambda k: (k - 1, k, k + 1, 63 + k, 64 + k, 255 + k, 256 + k, 257 + k, 600)   # noqa: E731


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
    ctx.genes_index_build(*_flat(seqs), np.asarray(feats, dtype=np.uint32), k)
    return gn.build_index(seqs, feats, k)


def _dev(ctx, reads, recs, min_hits):
    """bdg_fusion_scan_dev over device arrays, the output poisoned first and one record longer than the reads"""
    bases, off = _flat(reads)
    n = len(reads)
    d = [_native.DeviceArray.from_host(ctx, a) for a in (bases, off, np.ascontiguousarray(recs, dtype=_native.GENE_DTYPE).view(np.uint32),
                                                         np.full((n + 1) * 10, POISON, np.uint32))]
    try:
        ctx.fusion_scan_dev(d[0], d[1], n, d[2], min_hits, d[3])
        out = d[3].to_host()
        assert (out[n * 10:] == POISON).all(), "a store behind the last record"
        return out[:n * 10].view(_native.FUSION_DTYPE)
    finally:
        for a in d:
            a.free()


def _check(ctx, index, reads, min_hits, recs=None, what=""):
    """both entry points against the checker, every field -> the records"""
    recs = gn.assign_reads(index, reads, 1) if recs is None else recs
    want = fc.rec_tuples(fu.scan_reads(index, reads, recs, min_hits))
    assert fc.rec_tuples(ctx.fusion_scan(*_flat(reads), recs, min_hits)) == want, what
    assert fc.rec_tuples(_dev(ctx, reads, recs, min_hits)) == want, what
    return want


@pytest.mark.parametrize("k", KS)
def test_hand_derived_cases(ctx, k):
    seqs, feats = fc.three_genes(k)
    index = _build(ctx, seqs, feats, k)
    for name, read, min_hits, want in fc.hand_cases(k):
        assert _check(ctx, index, [read], min_hits, what=name) == [want], name
    # all of them in one call, with the gene records the device itself makes
    cases = [c for c in fc.hand_cases(k) if c[2] == 3]
    reads = [c[1] for c in cases]
    recs = ctx.genes_assign(*_flat(reads), 3)
    assert fc.rec_tuples(ctx.fusion_scan(*_flat(reads), recs, 3)) == [c[3] for c in cases]


@pytest.mark.parametrize("k", KS)
def test_record_agrees_with_the_gene_record(ctx, k):
    """feat_a, hits_a and hits_b are the gene record's feature, hits and second"""
    rng = np.random.default_rng(700 + k)
    scanned = 0
    for i in range(30):
        seqs, feats, reads = fc.small_case(rng, k)
        index = _build(ctx, seqs, feats, k)
        recs = ctx.genes_assign(*_flat(reads), 1)
        got = ctx.fusion_scan(*_flat(reads), recs, 1)
        assert fc.rec_tuples(got) == fc.rec_tuples(fu.scan_reads(index, reads, recs, 1)), i
        took = (got["flags"] & fu.SKIPPED) == 0
        scanned += int(took.sum())
        assert (got["feat_a"][took] == recs["feature"][took]).all() and (got["hits_a"][took] == recs["hits"][took]).all()
        assert (got["hits_b"][took] == recs["second"][took]).all()
        assert (took == (((recs["flags"] & gn.CROWDED) == 0) & (recs["second"] >= 1))).all()
    assert scanned > 10                                      # (the checker scans 56, 35 and 15 of these reads at k = 11, 21, 31)


@pytest.mark.parametrize("k", KS)
def test_read_lengths_and_a_lone_hit_at_either_end(ctx, k):
    """a random read of every length; gene 1 owns its first window and gene 2 all the others, then gene 2 its last window and gene 1
    all the others: the lone hit is window 0, or the last window of the read"""
    rng = np.random.default_rng(40 + k)
    for n in LENGTHS(k):
        s = gc.rand_seq(rng, n)
        for seqs in ([s[:k], s[1:]], [s[:n - 1], s[max(n - k, 0):]]):
            index = _build(ctx, seqs, [1, 2], k)
            want = _check(ctx, index, [s], 1, what="length %d" % n)
            if n > k + 1 and len(set(s[w:w + k] for w in range(n - k + 1))) == n - k + 1:      # (no window twice: by hand)
                lone_first = seqs[0] == s[:k]
                last = n - k
                assert want == [(2, last, 1, last, 1, 1, 0, 0, 0, fu.SPLIT) if lone_first
                                else (1, last, 0, last - 1, 2, 1, last, last, 0, fu.SPLIT | fu.A_UP)], n


@pytest.mark.parametrize("k", KS)
def test_ranges_at_the_chunk_borders(ctx, k):
    """last_a and first_b at 62 .. 65 and 254 .. 257: the last window of a chunk of 64 and of a step of 256, and the first of the next"""
    rng = np.random.default_rng(60 + k)
    ga, gb = gc.rand_seq(rng, 700), gc.rand_seq(rng, 700)
    index = _build(ctx, [ga, gb], [4, 9], k)
    reads, wants = [], []
    for edge in (64, 256):
        for d in (-2, -1, 0, 1):
            n_up = edge + d + 1                              # windows of the piece in front: its last is edge + d
            for big_up in (True, False):                     # A in front of B, and behind it
                n_down = 20 if big_up else n_up + 7
                reads.append(fc.join(k, (ga, 0, n_up), (gb, 3, n_down)))
                first_down = n_up + k - 1
                wants.append((4, n_up, 0, n_up - 1, 9, n_down, first_down, first_down + n_down - 1, 0, fu.SPLIT | fu.A_UP) if big_up
                             else (9, n_down, first_down, first_down + n_down - 1, 4, n_up, 0, n_up - 1, 0, fu.SPLIT))
    # first_b on either side of the borders as well: the piece in front ends k - 1 windows earlier
    for edge in (64, 256):
        for d in (-1, 0, 1):
            n_up = edge + d - k + 1
            reads.append(fc.join(k, (ga, 0, n_up), (gb, 3, 20)))
            wants.append((4, n_up, 0, n_up - 1, 9, 20, edge + d, edge + d + 19, 0, fu.SPLIT | fu.A_UP))
    assert _check(ctx, index, reads, 3) == wants


def test_gated_reads_are_not_read(ctx):
    """reads that would be SPLIT if they were scanned, behind gene records that fail the gate one way each, and lower-case poison
    bytes behind such records: every one gets the SKIPPED record, in an output that was poisoned"""
    k = 21
    seqs, feats = fc.three_genes(k)
    index = _build(ctx, seqs, feats, k)
    read = fc.hand_cases(k)[0][1]
    own = gn.assign_reads(index, [read], 1)
    assert (int(own["hits"][0]), int(own["second"][0])) == (30, 10)
    reads = [read] * 5 + ["x" * 500] * 3
    recs = np.repeat(own, 8)
    recs["second"][1] = 9                                   # one below min_hits
    recs["hits"][2], recs["second"][2] = 9, 9
    recs["flags"][3] = gn.CROWDED
    recs["second"][4] = 10                                  # exactly min_hits: scanned
    recs["second"][5:] = 0
    want = fu.scan_reads(index, reads, recs, 10)
    assert [int(f) for f in want["flags"]] == [3, 4, 4, 4, 3, 4, 4, 4]
    got = _check(ctx, index, reads, 10, recs)
    assert got[1] == fc.SKIPPED_REC and got[0] == fc.hand_cases(k)[0][3]


def test_256_features_and_257(ctx):
    k = 11
    rng = np.random.default_rng(256)
    seqs, feats, read = gc.crowded_case(rng, k, 256)
    index = _build(ctx, seqs, feats, k)
    want = _check(ctx, index, [read], 1)
    assert want == [(10, 1, 0, 0, 11, 1, k + 1, k + 1, 1, 0)]          # hits_b == third: no flag
    seqs, feats, read = gc.crowded_case(rng, k, 257)
    index = _build(ctx, seqs, feats, k)
    own = gn.assign_reads(index, [read], 1)
    assert int(own["flags"][0]) == gn.CROWDED
    assert _check(ctx, index, [read], 1, own) == [fc.SKIPPED_REC]      # its own record: gated
    other = own.copy()
    other["feature"], other["hits"], other["second"], other["flags"] = 10, 1, 1, gn.TIE
    assert _check(ctx, index, [read, read[:k]], 1, np.concatenate([other, other])) == \
        [fc.SKIPPED_REC, (10, 1, 0, 0, fu.NONE, 0, 0, 0, 0, 0)]      # another read's record: the 257th feature; and a read without a B


def test_no_reads_one_read_and_more_reads_than_waves(ctx):
    k = 21
    seqs, feats = fc.three_genes(k)
    index = _build(ctx, seqs, feats, k)
    cases = [c for c in fc.hand_cases(k) if c[2] == 3]
    pool, pool_want = [c[1] for c in cases], [c[3] for c in cases]
    recs = gn.assign_reads(index, pool, 1)
    assert len(ctx.fusion_scan(np.zeros(0, np.uint8), np.zeros(1, np.uint64), recs[:0], 3)) == 0
    out = np.full(10, POISON, np.uint32)
    assert ctx.lib.bdg_fusion_scan(ctx.h, None, None, 0, None, 3, out.ctypes.data) == 0 and (out == POISON).all()
    assert fc.rec_tuples(ctx.fusion_scan(*_flat(pool[:1]), recs[:1], 3)) == pool_want[:1]
    which = np.random.default_rng(5).integers(0, len(pool), size=20000)
    reads, many = [pool[i] for i in which], recs[which]
    want = [pool_want[i] for i in which]
    first = ctx.fusion_scan(*_flat(reads), many, 3)
    assert fc.rec_tuples(first) == want
    assert (ctx.fusion_scan(*_flat(reads), many, 3) == first).all()                     # twice
    assert fc.rec_tuples(_dev(ctx, reads, many, 3)) == want
    order = np.random.default_rng(6).permutation(len(reads))                            # shuffled
    assert (ctx.fusion_scan(*_flat([reads[i] for i in order]), many[order], 3) == first[order]).all()


def test_64_slot_tables_with_a_wrap(ctx):
    """two genes of 10 windows at k = 11: 64 slots; among 200 random ones some keep a key in front of its home slot"""
    rng = np.random.default_rng(64)
    wrapped = split = 0
    for _ in range(200):
        ga, gb = gc.rand_seq(rng, 20), gc.rand_seq(rng, 20)
        index = _build(ctx, [ga, gb], [0, 1], 11)
        stats = index.stats()
        assert stats[3] == 64
        wrapped += stats[5] > 0
        want = _check(ctx, index, [ga + gb, gb[2:] + "N" + ga, ga[:15] + gb[:15] + ga[5:]], 3)
        split += sum(1 for w in want if w[9] & fu.SPLIT)
    assert wrapped > 5 and split > 300


def test_argument_errors():
    k = 21
    seqs, feats = fc.three_genes(k)
    read = fc.hand_cases(k)[0][1]
    bases, off = _flat([read, read])
    recs = np.repeat(gn.assign_reads(gn.build_index(seqs, feats, k), [read], 1), 2)
    out = np.full(30, POISON, np.uint32)
    ctx = _native.Context(0)
    try:
        lib, h = ctx.lib, ctx.h
        good = [bases.ctypes.data, off.ctypes.data, 2, recs.ctypes.data, 3, out.ctypes.data]
        d = _native.DeviceArray.from_host(ctx, np.full(64, POISON, np.uint32))
        good_dev = [d.ptr, d.ptr, 1, d.ptr, 3, d.ptr]
        # no genes index yet
        assert lib.bdg_fusion_scan(h, *good) == _native.E_ARG and b"no genes index built" in lib.bdg_last_error(h)
        assert lib.bdg_fusion_scan_dev(h, *good_dev) == _native.E_ARG
        with pytest.raises(_native.BadgerHipError):
            ctx.fusion_scan(bases, off, recs, 3)
        ctx.genes_index_build(*_flat(seqs), np.asarray(feats, dtype=np.uint32), k)
        for i, bad in ((4, 0), (1, None), (3, None), (5, None), (0, None)):
            args = list(good)
            args[i] = bad
            assert lib.bdg_fusion_scan(h, *args) == _native.E_ARG, i
            if i:                                            # (device bases are not looked at by the host)
                args = list(good_dev)
                args[i] = bad
                assert lib.bdg_fusion_scan_dev(h, *args) == _native.E_ARG, i
        worse = off.copy()
        worse[2] = worse[1] - 1
        assert lib.bdg_fusion_scan(h, bases.ctypes.data, worse.ctypes.data, 2, recs.ctypes.data, 3, out.ctypes.data) == _native.E_ARG
        assert b"non-decreasing" in lib.bdg_last_error(h)
        assert lib.bdg_fusion_scan(None, *good) == _native.E_ARG and lib.bdg_fusion_scan_dev(None, *good_dev) == _native.E_ARG
        assert lib.bdg_fusion_scan_dev(h, None, None, 0, None, 3, None) == 0                 # n == 0 writes nothing
        assert (out == POISON).all() and (d.to_host() == POISON).all()
        with pytest.raises(ValueError):
            ctx.fusion_scan(bases, off, recs[:1], 3)
        assert lib.bdg_fusion_scan(h, *good) == 0 and fc.rec_tuples(out[:20].view(_native.FUSION_DTYPE)) == [fc.hand_cases(k)[0][3]] * 2
        assert (out[20:] == POISON).all()
        d.free()
    finally:
        ctx.close()
