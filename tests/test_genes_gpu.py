"""The gene-call kernels (csrc/genes_kernels.hip) against the rule of badger_amd/genes.py: every field of every record and all
six stats of the table, bit for bit.  Read lengths around the wave's 64 windows and the 256 windows a wave has in flight; an N
at every offset of a window across those edges, in reads and in transcripts; a few hundred tables of 64 and 128 slots with
long runs and wrap-around; one key written by 4,096 waves; ties, the min_hits boundary, 256 against 257 features; more reads
and transcripts than waves in flight (at most 8,192 and 4,096 on 256 compute units: 9,000 and 5,000 here); long reads; an index rebuilt
with another k; calls behind other kernel families on one context; device arrays over poisoned outputs; the host entry
against the device entry; every argument error."""
import numpy as np
import pytest

import consensus_cases as cc
import genes_cases as gc
import umi_cases as uc
from badger_amd import _native
from badger_amd import consensus as cs
from badger_amd import genes as gn

pytestmark = pytest.mark.gpu

KS = (11, 21, 31)


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
    """the index on the device and in the checker; all six stats compared -> the checker's index"""
    ctx.genes_index_build(*_flat(seqs), np.asarray(feats, dtype=np.uint32), k)
    index = gn.build_index(seqs, feats, k)
    got, want = tuple(int(x) for x in ctx.genes_index_stats()), index.stats()
    assert got == want, "stats: device %r, checker %r" % (got, want)
    return index


def _host(ctx, reads, min_hits):
    return gc.rec_tuples(ctx.genes_assign(*_flat(reads), min_hits))


def _dev(ctx, reads, min_hits):
    """bdg_genes_assign_dev over device arrays, the output poisoned first"""
    bases, off = _flat(reads)
    n = len(reads)
    d = [_native.DeviceArray.from_host(ctx, a) for a in (bases, off, np.full(max(n, 1) * 6, 0xABABABAB, np.uint32))]
    try:
        ctx.genes_assign_dev(d[0], d[1], n, min_hits, d[2])
        return gc.rec_tuples(d[2].to_host().view(_native.GENE_DTYPE)[:n])
    finally:
        for a in d:
            a.free()


def _same(reads, got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            r = reads[i]
            raise AssertionError("%s: read %d (%d bases) %r\n  device  %r\n  checker %r" % (what, i, len(r), r if len(r) < 90 else r[:87] + "...", g, w))


def _check(ctx, index, reads, min_hits, what, run=_host):
    want = gc.rec_tuples(gn.assign_reads(index, reads, min_hits))
    _same(reads, run(ctx, reads, min_hits), want, what)
    return want


def test_record_layout():
    assert _native.GENE_DTYPE == gn.REC_DTYPE and _native.GENE_DTYPE.itemsize == 24
    assert (_native.GENES_AMBIGUOUS, _native.GENES_NONE, _native.GENES_MAX_FEATURES) == (gn.AMBIGUOUS, gn.NONE, gn.MAX_FEATURES)
    assert (_native.GENE_ASSIGNED, _native.GENE_LOW, _native.GENE_TIE, _native.GENE_CROWDED) == (gn.ASSIGNED, gn.LOW, gn.TIE, gn.CROWDED)


@pytest.mark.parametrize("k", KS)
def test_read_lengths_around_the_lanes_and_the_tile(ctx, k):
    rng = np.random.default_rng(k)
    text = gc.rand_seq(rng, k + 600)
    # three genes along the text, the middle stretch shared by two of them; the reads are prefixes and suffixes of every length
    index = _build(ctx, [text[:300], text[200:500], text[450:]], [2, 1, 0], k)
    lengths = list(range(0, k + 131)) + [k + w + d for w in (255, 256, 511, 512) for d in (-2, -1, 0, 1)]
    reads = [text[:L] for L in lengths] + [text[len(text) - L:] for L in lengths] + [gc.mutate(rng, text[:L]) for L in lengths[::7]]
    want = _check(ctx, index, reads, 3, "lengths, k %d" % k)
    _check(ctx, index, reads, 3, "lengths, device arrays, k %d" % k, run=_dev)
    assert [w[3] for w in want[:k + 131]] == [max(0, L - k + 1) for L in range(k + 131)]
    assert {w[5] for w in want} >= {gn.ASSIGNED, gn.LOW}


@pytest.mark.parametrize("k", KS)
def test_an_n_at_every_offset_of_a_window_across_an_edge(ctx, k):
    rng = np.random.default_rng(40 + k)
    for edge in (64, 256):                                  # the next 64 positions' planes, the next iteration's
        clean = gc.rand_seq(rng, edge + k + 6)
        start = edge - k // 2                               # this window straddles the edge
        variants = [clean[:start + j] + "N" + clean[start + j + 1:] for j in range(k)]
        index = _build(ctx, [clean], [3], k)
        want = _check(ctx, index, [clean] + variants, 1, "N in a read, k %d, edge %d" % (k, edge))
        assert want[0][3] == edge + 7 and all(w[3] < edge + 7 for w in want[1:])
        for j in (0, k // 2 - 1, k // 2, k - 1) if k > 11 else range(k):      # ... and in the transcript
            index = _build(ctx, [variants[j], clean[:k + 3]], [3, 4], k)
            _check(ctx, index, [clean, variants[j]], 1, "N in a transcript, k %d, edge %d, offset %d" % (k, edge, j))


def test_small_tables_with_chains_and_wraps(ctx):
    rng = np.random.default_rng(5)
    longest = wrapped = 0
    for n in range(300):
        seqs, feats = gc.tiny_index_case(rng, 11, int(rng.integers(1, 41)))
        index = _build(ctx, seqs, feats, 11)
        st = ctx.genes_index_stats()
        assert int(st[3]) in (64, 128)
        longest, wrapped = max(longest, int(st[4])), wrapped + int(st[5] > 0)
        if n % 10 == 0:
            _check(ctx, index, seqs + [gc.rand_seq(rng, 40)], 1, "small table %d" % n)
    assert longest >= 4 and wrapped >= 1, (longest, wrapped)


def test_one_key_from_4096_waves(ctx):
    seqs, feats = ["A" * 200] * 4096, list(range(4096))
    index = _build(ctx, seqs, feats, 21)
    assert tuple(int(x) for x in ctx.genes_index_stats()) == (4096 * 180, 1, 1, 1 << 21, 1, 0)
    assert _check(ctx, index, ["A" * 100, "A" * 20, "C" * 100], 1, "polyA") == [
        (gn.NONE, 0, 0, 80, 80, gn.LOW), (gn.NONE, 0, 0, 0, 0, gn.LOW), (gn.NONE, 0, 0, 80, 0, gn.LOW)]
    # the same sequences, one feature: the key is that feature's
    ctx.genes_index_build(*_flat(seqs), np.full(4096, 77, np.uint32), 21)
    assert tuple(int(x) for x in ctx.genes_index_stats()) == (4096 * 180, 1, 0, 1 << 21, 1, 0)
    assert _host(ctx, ["A" * 100], 1) == [(77, 80, 0, 80, 80, gn.ASSIGNED)]


def test_one_feature_owns_every_key(ctx):
    rng = np.random.default_rng(9)
    seqs = [gc.rand_seq(rng, 400, 0.01) for _ in range(5)]
    index = _build(ctx, seqs + seqs[:2], [12345] * 7, 21)
    assert int(ctx.genes_index_stats()[2]) == 0
    want = _check(ctx, index, [s[50:350] for s in seqs] + [gc.rand_seq(rng, 300)], 3, "one feature")
    assert [w[0] for w in want] == [12345] * 5 + [gn.NONE]


@pytest.mark.parametrize("k", KS)
def test_hand_derived_cases_ties_and_min_hits(ctx, k):
    cases, _ = gc.hand_cases(k)
    for name, seqs, feats, read, min_hits, want in cases:
        _build(ctx, seqs, feats, k)
        for run in (_host, _dev):
            assert run(ctx, [read], min_hits) == [want], name


@pytest.mark.parametrize("k", (11, 31))
def test_256_against_257_features(ctx, k):
    rng = np.random.default_rng(7)
    for n, rec in ((256, (10, 1, 1, 256, 256, gn.TIE)), (257, (gn.NONE, 0, 0, 257, 257, gn.CROWDED)), (300, None)):
        seqs, feats, read = gc.crowded_case(rng, k, n)
        extra = gc.rand_seq(rng, k + 6)                       # feature 5: seven windows, in two transcripts
        index = _build(ctx, seqs + [extra, extra + "NN"], feats + [5, 5], k)
        uncrowded = "N".join(seqs[:200]) + "N" + extra
        want = _check(ctx, index, [read, uncrowded, read, extra], 1, "%d features" % n)
        assert rec is None or want[0] == rec
        assert want[1][5] == want[3][5] == gn.ASSIGNED and want[1][0] == 5 and want[1][2] == 1
        assert want[0][5] == (gn.CROWDED if n > 256 else gn.TIE)


@pytest.fixture(scope="module")
def many():
    rng = np.random.default_rng(33)
    genes = [gc.rand_seq(rng, int(rng.integers(30, 400)), 0.002) for _ in range(5000)]
    feats = [int(g) for g in rng.integers(0, 1200, size=5000)]
    for g in range(0, 5000, 9):                              # shared stretches: ambiguous keys
        genes[g] = genes[g][:20] + genes[(g + 1) % 5000][:60] + genes[g][20:]
    reads = []
    for i in range(9000):
        g = int(rng.integers(0, 5000))
        L = int(rng.integers(25, 140))
        r = genes[g][-L:] if i % 3 else gc.rand_seq(rng, L)
        reads.append(gc.mutate(rng, r) if i % 2 else r)
    index = gn.build_index(genes, feats, 21)
    return genes, feats, reads, index, gc.rec_tuples(gn.assign_reads(index, reads, 3))


def test_more_reads_and_transcripts_than_waves(ctx, many):
    genes, feats, reads, index, want = many
    _build(ctx, genes, feats, 21)
    assert int(ctx.genes_index_stats()[2]) > 1000
    _same(reads, _host(ctx, reads, 3), want, "9,000 reads")
    flags = [w[5] for w in want]
    assert flags.count(gn.ASSIGNED) > 3000 and flags.count(gn.LOW) > 2000
    # the same calls twice give the same bytes, and a small call behind the large one reuses the staging buffers
    assert _host(ctx, reads[:2000], 3) == want[:2000]
    _same(reads[:3], _host(ctx, reads[:3], 3), want[:3], "small call after the large one")
    _same(reads[4000:4001], _dev(ctx, reads[4000:4001], 3), want[4000:4001], "one read, device arrays")


def test_host_entry_against_device_entry(ctx, many):
    genes, feats, reads, index, want = many
    _build(ctx, genes, feats, 21)
    part = reads[1000:3000] + ["", "A", genes[0]]
    dev = _dev(ctx, part, 3)
    assert dev == _host(ctx, part, 3)
    assert dev[:2000] == want[1000:3000]
    assert _dev(ctx, [], 3) == [] and _host(ctx, [], 3) == []
    for min_hits in (1, 10, 0xFFFFFFFF):
        _check(ctx, index, part[:300], min_hits, "min_hits %d" % min_hits, run=_dev)


def test_long_reads(ctx):
    rng = np.random.default_rng(17)
    text = gc.rand_seq(rng, 20000, 0.0005)
    cuts = [0, 3000, 7000, 8193, 12000, 20000]
    seqs = [text[a:b] for a, b in zip(cuts, cuts[1:])] + [text[6000:9000]]
    index = _build(ctx, seqs, [4, 3, 2, 1, 0, 9], 21)
    reads = [text[:8193], text, gc.mutate(rng, text[:8193]), gc.mutate(rng, text), text[11000:] + text[:9000]]
    for run in (_host, _dev):
        want = _check(ctx, index, reads, 3, "long reads", run=run)
    assert want[1][3] > 19500 and want[1][5] == gn.ASSIGNED and want[1][0] == 0 and want[1][2] > 2500


def test_rebuilt_with_another_k_against_a_fresh_context(ctx, many):
    genes, feats, reads, index, want = many
    _build(ctx, genes, feats, 21)
    index15 = _build(ctx, genes[:1500], feats[:1500], 15)        # replaces the table of k = 21, smaller
    got = _host(ctx, reads[:1500], 2)
    fresh = _native.Context(0)
    try:
        fresh.genes_index_build(*_flat(genes[:1500]), np.asarray(feats[:1500], dtype=np.uint32), 15)
        assert (fresh.genes_index_stats() == ctx.genes_index_stats()).all()
        assert _host(fresh, reads[:1500], 2) == got
    finally:
        fresh.close()
    _same(reads[:1500], got, gc.rec_tuples(gn.assign_reads(index15, reads[:1500], 2)), "k 15 after k 21")
    _build(ctx, genes, feats, 21)                                # ... and back, larger
    _same(reads[:1500], _host(ctx, reads[:1500], 3), want[:1500], "k 21 again")


def test_behind_other_kernel_families_on_one_context(ctx, many):
    genes, feats, reads, index, want = many
    _build(ctx, genes, feats, 21)
    rng = np.random.default_rng(3)
    groups = [cc.elected(cc.molecule(rng, 300, 4, cs.ANCHOR_END)[1]) for _ in range(20)]
    cons_want = cs.consensus_groups(groups, cs.ANCHOR_END, 20)
    case = uc.case("dense", 12)
    d = [_native.DeviceArray.from_host(ctx, a) for a in (case.cells, case.rank, case.has, case.umi)]
    d_mol = _native.DeviceArray(ctx, max(case.n, 1), np.uint32)
    d_cnt = _native.DeviceArray(ctx, (max(len(case.cells), 1), 4), np.uint32)
    bases, off = _flat(reads[:500])
    g = [_native.DeviceArray.from_host(ctx, a) for a in (bases, off, np.full(500 * 6, 0xABABABAB, np.uint32))]
    try:
        # the three families queued on the context's stream one behind the other, nothing waited for in between
        ctx.umi_dedup_dev(d[1], d[2], d[3], case.n, d[0], len(case.cells), 12, 1, d_mol, d_cnt)
        ctx.genes_assign_dev(g[0], g[1], 500, 3, g[2])
        flat = [s.encode() for grp in groups for s in grp]
        cons = ctx.consensus(np.frombuffer(b"".join(flat), dtype=np.uint8),
                             np.concatenate([[0], np.cumsum([len(s) for s in flat])]).astype(np.uint64),
                             np.concatenate([[0], np.cumsum([len(grp) for grp in groups])]).astype(np.uint64), cs.ANCHOR_END, 20)
        got = gc.rec_tuples(g[2].to_host().view(_native.GENE_DTYPE))
    finally:
        for a in d + g + [d_mol, d_cnt]:
            a.free()
    _same(reads[:500], got, want[:500], "between bdg_umi_dedup_dev and bdg_consensus")
    out, out_off, out_len, _, _ = cons
    assert [out[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes() for i in range(len(groups))] == [w[0] for w in cons_want]
    _same(reads[500:900], _host(ctx, reads[500:900], 3), want[500:900], "after bdg_consensus")


def test_argument_errors(ctx):
    bases, off = _flat(["ACGT" * 20, "TTGCA" * 10])
    feats = np.array([1, 2], dtype=np.uint32)
    fresh = _native.Context(0)
    try:
        for call, word in ((lambda: fresh.genes_assign(bases, off, 3), "no index"), (lambda: fresh.genes_index_stats(), "no index"),
                           (lambda: fresh.genes_assign_dev(0, 0, 0, 3, 0), "no index"),
                           (lambda: fresh.genes_index_build(bases, off, feats, 10), "11 .. 31"),
                           (lambda: fresh.genes_index_build(bases, off, feats, 32), "11 .. 31"),
                           (lambda: fresh.genes_index_build(bases, off, np.array([1, gn.AMBIGUOUS], np.uint32), 21), "reserved"),
                           (lambda: fresh.genes_index_build(bases, off, np.array([gn.NONE, 1], np.uint32), 21), "reserved"),
                           (lambda: fresh.genes_index_build(bases, off[[0, 2, 1]], feats, 21), "non-decreasing"),
                           (lambda: fresh.genes_assign(bases, off, 3), "no index")):          # (no failed build left one behind)
            with pytest.raises(_native.BadgerHipError) as e:
                call()
            assert e.value.code == _native.E_ARG and word in str(e.value), word
        fresh.genes_index_build(bases, off, feats, 21)
        d = [_native.DeviceArray.from_host(fresh, a) for a in (bases, off, np.zeros(12, np.uint32))]
        try:
            for call, word in ((lambda: fresh.genes_assign(bases, off, 0), "min_hits"),
                               (lambda: fresh.genes_assign_dev(d[0], d[1], 2, 0, d[2]), "min_hits"),
                               (lambda: fresh.genes_assign(bases, off[[0, 2, 1]], 3), "non-decreasing"),
                               (lambda: fresh.genes_assign_dev(d[0], 0, 2, 3, d[2]), "null"),
                               (lambda: fresh.genes_assign_dev(d[0], d[1], 2, 3, 0), "null")):
                with pytest.raises(_native.BadgerHipError) as e:
                    call()
                assert e.value.code == _native.E_ARG and word in str(e.value), word
            # an argument error leaves the index as it was
            with pytest.raises(_native.BadgerHipError):
                fresh.genes_index_build(bases, off, feats, 40)
            assert gc.rec_tuples(fresh.genes_assign(bases, off, 3)) == [(1, 60, 0, 60, 60, gn.ASSIGNED), (2, 30, 0, 30, 30, gn.ASSIGNED)]
        finally:
            for a in d:
                a.free()
    finally:
        fresh.close()
    lib = _native.load()
    assert lib.bdg_genes_index_build(None, None, None, 0, None, 21) == _native.E_ARG
    assert lib.bdg_genes_assign(None, None, None, 0, 3, None) == _native.E_ARG
