"""The isoform kernels (k_iso_insert, k_iso_assign of csrc/genes_kernels.hip) against the rule of badger_amd/genes.py: every
field of every record bit for bit, and every mask the rule uses through reads of one window, whose compat is their key's mask.
Read lengths around the wave's 64 windows and the 256 a wave has in flight; a distinguishing window at every lane offset across
those edges; tables of 64 slots with chains and wraps; local indices on both sides of bit 31 and an overflowing gene; one key
from 4,096 waves with 64 local indices; 1, 2 and 64 distinct masks among 64 windows; reads without a gene between assigned
ones over a poisoned output; more reads than resident waves; the host entry against the device entry; plain and iso builds in
both orders; calls behind other kernel families on one context; every argument error."""
import numpy as np
import pytest

import genes_cases as gc
import iso_cases as ic
import umi_cases as uc
from badger_amd import _native
from badger_amd import genes as gn

pytestmark = pytest.mark.gpu

U, M, NG = gn.ISO_UNIQUE, gn.ISO_MULTI, gn.ISO_NOGENE
NOGENE = (0, gn.NONE, 0, 0, 0, NG, 0)
POS = 620


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _flat(seqs):
    flat = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    return (np.frombuffer(b"".join(flat), dtype=np.uint8),
            np.concatenate([[0], np.cumsum([len(s) for s in flat], dtype=np.int64)]).astype(np.uint64))


def _build(ctx, seqs, feats, local, k):
    """the index with masks on the device and in the checker; the six stats are the plain build's -> the checker's index"""
    ctx.genes_index_build_iso(*_flat(seqs), np.asarray(feats, dtype=np.uint32), np.asarray(local, dtype=np.uint8), k)
    index = gn.build_index(seqs, feats, k, local)
    got, want = tuple(int(x) for x in ctx.genes_index_stats()), index.stats()
    assert got == want, "stats: device %r, checker %r" % (got, want)
    return index


def _host(ctx, reads, min_hits, margin):
    g, i = ctx.iso_assign(*_flat(reads), min_hits, margin)
    return gc.rec_tuples(g), ic.iso_tuples(i)


def _dev(ctx, reads, min_hits, margin):
    """bdg_genes_assign_dev, then bdg_iso_assign_dev over its records, both outputs poisoned first"""
    bases, off = _flat(reads)
    n = len(reads)
    d = [_native.DeviceArray.from_host(ctx, a) for a in (bases, off, np.full(max(n, 1) * 6, 0xABABABAB, np.uint32),
                                                         np.full(max(n, 1) * 8, 0xABABABAB, np.uint32))]
    try:
        ctx.genes_assign_dev(d[0], d[1], n, min_hits, d[2])
        ctx.iso_assign_dev(d[0], d[1], n, d[2], margin, d[3])
        return gc.rec_tuples(d[2].to_host().view(_native.GENE_DTYPE)[:n]), ic.iso_tuples(d[3].to_host().view(_native.ISO_DTYPE)[:n])
    finally:
        for a in d:
            a.free()


def _same(reads, got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            r = reads[i]
            raise AssertionError("%s: read %d (%d bases) %r\n  device  %r\n  checker %r" % (what, i, len(r), r if len(r) < 90 else r[:87] + "...", g, w))


def _check(ctx, index, reads, min_hits, margin, what, run=_host):
    want = ic.rule(index, reads, min_hits, margin)
    got = run(ctx, reads, min_hits, margin)
    _same(reads, got[0], want[0], what + " (gene records)")
    _same(reads, got[1], want[1], what)
    assert all(i[4] == (g[1] if g[5] & gn.ASSIGNED else 0) for g, i in zip(*want))      # n_gene is the gene record's hits
    return want[1]


def _windows(seqs, k):
    """every distinct window of the sequences as a read of its own: its record's compat is the mask of its key"""
    return sorted({s[p:p + k] for s in seqs for p in range(len(s) - k + 1) if "N" not in s[p:p + k]})


def test_record_layout():
    assert _native.ISO_DTYPE == gn.ISO_DTYPE and _native.ISO_DTYPE.itemsize == 32
    assert (_native.ISO_UNIQUE, _native.ISO_MULTI, _native.ISO_NOGENE) == (U, M, NG)
    assert (_native.ISO_LOCAL_MAX, _native.ISO_MARGIN_DEFAULT) == (gn.LOCAL_MAX, gn.MARGIN_DEFAULT)


@pytest.fixture(scope="module")
def two_isoforms():
    """a text of 1,300 bases and its copy with base POS substituted: the k windows over that base tell the two apart"""
    rng = np.random.default_rng(11)
    text = gc.rand_seq(rng, 1300)
    other = text[:POS] + ("A" if text[POS] != "A" else "C") + text[POS + 1:]
    return text, other


@pytest.mark.parametrize("k", (11, 21, 31))
def test_read_lengths_around_the_lanes_and_the_tile(ctx, two_isoforms, k):
    text, other = two_isoforms
    index = _build(ctx, [text, other, text[:300]], [5, 5, 5], [0, 1, 40], k)
    lengths = [k - 1, k, k + 1, 63, 64, 65, 256, 257, 256 + k] + [64 + k - 2, 64 + k - 1, 64 + k, 255 + k, 257 + k, 512, 512 + k]
    reads = [text[:L] for L in lengths] + [text[POS - L + 1:POS + 1] for L in lengths] + [other[POS:POS + L] for L in lengths]
    for run in (_host, _dev):
        want = _check(ctx, index, reads, 1, 1, "lengths, k %d" % k, run=run)
    assert want[0] == NOGENE and want[1] == ((1 << 40) | 3, 5, 1, 0, 1, M, 0)
    # the reads that end with base POS hold 1 .. k windows over it: the first transcript's alone from k bases on
    assert all(w[0] == 1 and w[5] == U for w in want[len(lengths) + 1:2 * len(lengths)])
    assert all(w[0] == 2 and w[5] == U for w in want[2 * len(lengths) + 1:])


@pytest.mark.parametrize("k", (11, 21, 31))
def test_a_distinguishing_window_at_every_lane_offset_across_an_edge(ctx, two_isoforms, k):
    text, other = two_isoforms
    index = _build(ctx, [text, other], [3, 3], [62, 63], k)
    reads = []
    for edge in (64, 256):
        for d in range(-k - 2, k + 3):                      # the substituted base at position edge + d of the read
            start = POS - edge - d
            for src in (text, other):
                reads.append(src[start:start + edge + 2 * k + 8])
    want = _check(ctx, index, reads, 1, 1, "edges, k %d" % k)
    _check(ctx, index, reads[::5], 1, k + 1, "edges, a margin that reaches, k %d" % k, run=_dev)
    for i, w in enumerate(want):
        n = len(reads[i]) - k + 1
        assert w == (1 << (62 + i % 2), 3, n, n - k, n, U, 0)


def test_small_tables_with_chains_and_wraps(ctx):
    """the mask lands on the slot the key sits in, not on its home: every key of every table is read back"""
    rng = np.random.default_rng(5)
    longest = wrapped = 0
    for n in range(200):
        seqs, feats = gc.tiny_index_case(rng, 11, int(rng.integers(1, 41)))
        seqs, feats = seqs + [s[:len(s) // 2 + 6] for s in seqs], feats + feats          # a second, shorter transcript of each gene
        local = [int(x) for x in rng.integers(0, 64, size=len(seqs))]
        index = _build(ctx, seqs, feats, local, 11)
        st = ctx.genes_index_stats()
        assert int(st[3]) in (64, 128)
        longest, wrapped = max(longest, int(st[4])), wrapped + int(st[5] > 0)
        reads = _windows(seqs, 11)
        want = _check(ctx, index, reads + seqs, 1, 1, "small table %d" % n)
        for r, w in zip(reads, want):
            key = gn.keys_of(r, 11)
            assert w == NOGENE if index.lookup(key)[0] == gn.AMBIGUOUS else w[0] == int(index.lookup_masks(key)[0])
    assert longest >= 4 and wrapped >= 1, (longest, wrapped)


def test_local_indices_on_both_sides_of_bit_31_and_an_overflowing_gene(ctx):
    k = 21
    rng = np.random.default_rng(63)
    shared = gc.rand_seq(rng, 40)
    own = [gc.rand_seq(rng, 30) for _ in range(66)]
    picks = (0, 31, 32, 62, 63)
    index = _build(ctx, [shared + "N" + own[i] for i in picks], [4] * 5, list(picks), k)
    want = _check(ctx, index, [own[i] for i in picks] + [shared], 1, 1, "local indices 0, 31, 32, 62, 63")
    assert [w[0] for w in want] == [1 << t for t in picks] + [sum(1 << t for t in picks)]
    # 66 transcripts of one gene, the command line's local indices: the 64th, 65th and 66th share bit 63
    seqs, feats = [shared + "N" + o for o in own], [9] * 66
    local, overflow = gn.local_indices(feats)
    assert overflow.all()
    index = _build(ctx, seqs, feats, local, k)
    reads = own + [shared, own[64][:25] + "N" + own[3], own[65] + "N" + own[63][:27]]
    for run in (_host, _dev):
        want = _check(ctx, index, reads, 1, 1, "66 transcripts", run=run)
    assert [w[0] for w in want[:66]] == [1 << min(t, 63) for t in range(66)]
    assert want[66:] == [(ic.ALL, 9, 20, 0, 20, M, 0), (1 << 3, 9, 10, 5, 15, U, 0), (1 << 63, 9, 17, 0, 17, U, 0)]


def test_one_key_from_4096_waves_with_64_local_indices(ctx):
    seqs = ["A" * 200] * 4096
    local = [i % 64 for i in range(4096)]
    index = _build(ctx, seqs, [77] * 4096, local, 21)
    assert tuple(int(x) for x in ctx.genes_index_stats()) == (4096 * 180, 1, 0, 1 << 21, 1, 0)
    want = _check(ctx, index, ["A" * 100, "A" * 21, "A" * 20, "C" * 100], 1, 1, "polyA")
    assert want == [(ic.ALL, 77, 80, 0, 80, M, 0), (ic.ALL, 77, 1, 0, 1, M, 0), NOGENE, NOGENE]
    # half of the local indices only, and the key in two genes: a mask nobody uses
    index = _build(ctx, seqs, [77] * 4096, [2 * (i % 32) for i in range(4096)], 21)
    assert _check(ctx, index, ["A" * 30], 1, 1, "polyA, even bits")[0][0] == 0x5555555555555555
    index = _build(ctx, seqs, [i % 2 for i in range(4096)], local, 21)
    assert _check(ctx, index, ["A" * 100], 1, 1, "polyA of two genes") == [NOGENE]


def test_1_2_and_64_distinct_masks_among_64_windows(ctx):
    k = 21
    rng = np.random.default_rng(64)
    X = gc.rand_seq(rng, 64 + k - 1 + 300)                  # its first 64 windows are one chunk of the wave
    head = X[:64 + k - 1]
    # transcript t is X without its first t bases: window w of X is in the transcripts 0 .. w, 64 masks in 64 windows
    index = _build(ctx, [X[t:] for t in range(64)], [1] * 64, list(range(64)), k)
    for margin, compat in ((1, 1), (2, 3), (64, ic.ALL), (0xFFFFFFFF, ic.ALL)):
        want = _check(ctx, index, [head, X, X[40:]], 1, margin, "64 masks, margin %d" % margin)
        assert want[0] == (compat, 1, 64, 63, 64, U if compat == 1 else M, 0)
    # two masks: the second transcript starts at window 32; one mask: it is the first once more
    index = _build(ctx, [X, X[32:]], [1, 1], [10, 50], k)
    assert _check(ctx, index, [head, X], 1, 1, "two masks")[0] == (1 << 10, 1, 64, 32, 64, U, 0)
    index = _build(ctx, [X, X], [1, 1], [10, 50], k)
    assert _check(ctx, index, [head, X], 1, 1, "one mask")[0] == ((1 << 10) | (1 << 50), 1, 64, 0, 64, M, 0)


@pytest.fixture(scope="module")
def many():
    """1,200 genes of 2 .. 4 exon-skipping isoforms, and 9,000 short reads: 3' fragments as they are or with synth's errors,
    every third read random - more reads than the device keeps waves resident (at most 8,192 on 256 compute units)"""
    rng = np.random.default_rng(33)
    names, seqs, gene = ic.model(rng, 1200, exon_lo=20, exon_hi=60, polya=25)
    local = gn.local_indices(gene)[0]
    reads = []
    for i in range(9000):
        L = int(rng.integers(25, 200))
        r = seqs[int(rng.integers(0, len(seqs)))][-L:] if i % 3 else gc.rand_seq(rng, L)
        reads.append(gc.mutate(rng, r) if i % 2 else r)
    index = gn.build_index(seqs, gene, 21, local)
    return seqs, gene, local, reads, index, ic.rule(index, reads, 3, 1)


def test_more_reads_than_waves_and_nogene_between_assigned(ctx, many):
    seqs, gene, local, reads, index, want = many
    _build(ctx, seqs, gene, local, 21)
    got = _dev(ctx, reads, 3, 1)                                # (poisoned outputs: a read without a gene is written too)
    _same(reads, got[0], want[0], "9,000 reads (gene records)")
    _same(reads, got[1], want[1], "9,000 reads")
    flags = [w[5] for w in want[1]]
    assert flags.count(U) > 1000 and flags.count(M) > 1000 and flags.count(NG) > 3000
    assert sum(1 for a, b in zip(flags, flags[1:]) if (a == NG) != (b == NG)) > 3000
    # the same call twice gives the same bytes; a small call behind the large one reuses the staging buffers
    assert _host(ctx, reads[:2000], 3, 1) == (want[0][:2000], want[1][:2000])
    assert _host(ctx, reads[:3], 3, 1) == (want[0][:3], want[1][:3])


def test_host_entry_against_device_entry(ctx, many):
    seqs, gene, local, reads, index, want = many
    _build(ctx, seqs, gene, local, 21)
    part = reads[1000:2500] + ["", "A", seqs[0]]
    dev = _dev(ctx, part, 3, 1)
    assert dev == _host(ctx, part, 3, 1)
    assert dev[1][:1500] == want[1][1000:2500]
    assert _dev(ctx, [], 3, 1) == ([], []) and _host(ctx, [], 3, 1) == ([], [])
    for min_hits, margin in ((1, 1), (3, 2), (3, 3), (10, 1), (3, 0xFFFFFFFF)):
        _check(ctx, index, part[:300], min_hits, margin, "min_hits %d, margin %d" % (min_hits, margin), run=_dev)
    # the gene records of the iso entry are those of the gene entry
    assert gc.rec_tuples(ctx.genes_assign(*_flat(part), 3)) == dev[0]


def test_plain_build_after_iso_build_and_back(ctx, many):
    seqs, gene, local, reads, index, want = many
    _build(ctx, seqs, gene, local, 21)
    bases, off = _flat(reads[:50])
    d = [_native.DeviceArray.from_host(ctx, a) for a in (bases, off, np.zeros(50 * 6, np.uint32), np.zeros(50 * 8, np.uint32))]
    try:
        ctx.genes_index_build(*_flat(seqs), np.asarray(gene, dtype=np.uint32), 21)      # the plain build drops the masks
        ctx.genes_assign_dev(d[0], d[1], 50, 3, d[2])
        assert gc.rec_tuples(d[2].to_host().view(_native.GENE_DTYPE)) == want[0][:50]
        for call in (lambda: ctx.iso_assign_dev(d[0], d[1], 50, d[2], 1, d[3]), lambda: ctx.iso_assign(bases, off, 3, 1)):
            with pytest.raises(_native.BadgerHipError) as e:
                call()
            assert e.value.code == _native.E_ARG and "no index with masks" in str(e.value)
        assert gc.rec_tuples(ctx.genes_assign(bases, off, 3)) == want[0][:50]           # the gene calls go on
    finally:
        for a in d:
            a.free()
    _build(ctx, seqs[:900], gene[:900], local[:900], 15)        # an iso build behind the plain one, another k, smaller
    index15 = gn.build_index(seqs[:900], gene[:900], 15, local[:900])
    _check(ctx, index15, reads[:600], 2, 1, "k 15 after a plain build")
    _build(ctx, seqs, gene, local, 21)
    assert _host(ctx, reads[:600], 3, 1) == (want[0][:600], want[1][:600])


def test_behind_other_kernel_families_on_one_context(ctx, many):
    seqs, gene, local, reads, index, want = many
    _build(ctx, seqs, gene, local, 21)
    case = uc.case("dense", 12)
    d = [_native.DeviceArray.from_host(ctx, a) for a in (case.cells, case.rank, case.has, case.umi)]
    d_mol = _native.DeviceArray(ctx, max(case.n, 1), np.uint32)
    d_cnt = _native.DeviceArray(ctx, (max(len(case.cells), 1), 4), np.uint32)
    bases, off = _flat(reads[:500])
    g = [_native.DeviceArray.from_host(ctx, a) for a in (bases, off, np.full(500 * 6, 0xABABABAB, np.uint32),
                                                         np.full(500 * 8, 0xABABABAB, np.uint32))]
    try:
        # queued on the context's stream one behind the other, nothing waited for in between
        ctx.umi_dedup_dev(d[1], d[2], d[3], case.n, d[0], len(case.cells), 12, 1, d_mol, d_cnt)
        ctx.genes_assign_dev(g[0], g[1], 500, 3, g[2])
        ctx.iso_assign_dev(g[0], g[1], 500, g[2], 1, g[3])
        ctx.umi_dedup_dev(d[1], d[2], d[3], case.n, d[0], len(case.cells), 12, 1, d_mol, d_cnt)
        got = ic.iso_tuples(g[3].to_host().view(_native.ISO_DTYPE))
    finally:
        for a in d + g + [d_mol, d_cnt]:
            a.free()
    _same(reads[:500], got, want[1][:500], "between two bdg_umi_dedup_dev calls")
    assert _host(ctx, reads[500:900], 3, 1) == (want[0][500:900], want[1][500:900])


def test_argument_errors(ctx):
    bases, off = _flat(["ACGT" * 20, "TTGCA" * 10])
    feats, local = np.array([1, 1], dtype=np.uint32), np.array([0, 63], dtype=np.uint8)
    fresh = _native.Context(0)
    try:
        for call, word in ((lambda: fresh.iso_assign(bases, off, 3, 1), "no index"),
                           (lambda: fresh.iso_assign_dev(0, 0, 0, 0, 1, 0), "no index"),
                           (lambda: fresh.genes_index_build_iso(bases, off, feats, local, 10), "11 .. 31"),
                           (lambda: fresh.genes_index_build_iso(bases, off, feats, local, 32), "11 .. 31"),
                           (lambda: fresh.genes_index_build_iso(bases, off, feats, np.array([0, 64], np.uint8), 21), "above 63"),
                           (lambda: fresh.genes_index_build_iso(bases, off, feats, np.array([255, 0], np.uint8), 21), "above 63"),
                           (lambda: fresh.genes_index_build_iso(bases, off, np.array([1, gn.AMBIGUOUS], np.uint32), local, 21), "reserved"),
                           (lambda: fresh.genes_index_build_iso(bases, off[[0, 2, 1]], feats, local, 21), "non-decreasing"),
                           (lambda: fresh.iso_assign(bases, off, 3, 1), "no index")):           # (no failed build left one behind)
            with pytest.raises(_native.BadgerHipError) as e:
                call()
            assert e.value.code == _native.E_ARG and word in str(e.value), word
        fresh.genes_index_build_iso(bases, off, feats, local, 21)
        d = [_native.DeviceArray.from_host(fresh, a) for a in (bases, off, np.zeros(12, np.uint32), np.zeros(16, np.uint32))]
        try:
            fresh.genes_assign_dev(d[0], d[1], 2, 3, d[2])
            for call, word in ((lambda: fresh.iso_assign(bases, off, 3, 0), "margin"),
                               (lambda: fresh.iso_assign(bases, off, 0, 1), "min_hits"),
                               (lambda: fresh.iso_assign_dev(d[0], d[1], 2, d[2], 0, d[3]), "margin"),
                               (lambda: fresh.iso_assign(bases, off[[0, 2, 1]], 3, 1), "non-decreasing"),
                               (lambda: fresh.iso_assign_dev(d[0], 0, 2, d[2], 1, d[3]), "null"),
                               (lambda: fresh.iso_assign_dev(d[0], d[1], 2, 0, 1, d[3]), "null"),
                               (lambda: fresh.iso_assign_dev(d[0], d[1], 2, d[2], 1, 0), "null")):
                with pytest.raises(_native.BadgerHipError) as e:
                    call()
                assert e.value.code == _native.E_ARG and word in str(e.value), word
            # an argument error leaves the index and its masks as they were
            with pytest.raises(_native.BadgerHipError):
                fresh.genes_index_build_iso(bases, off, feats, local, 40)
            g, i = fresh.iso_assign(bases, off, 3, 1)
            assert gc.rec_tuples(g) == [(1, 60, 0, 60, 60, gn.ASSIGNED), (1, 30, 0, 30, 30, gn.ASSIGNED)]
            assert ic.iso_tuples(i) == [(1, 1, 60, 0, 60, U, 0), (1 << 63, 1, 30, 0, 30, U, 0)]
        finally:
            for a in d:
                a.free()
    finally:
        fresh.close()
    lib = _native.load()
    assert lib.bdg_genes_index_build_iso(None, None, None, 0, None, None, 21) == _native.E_ARG
    assert lib.bdg_iso_assign(None, None, None, 0, 3, 1, None, None) == _native.E_ARG
    assert lib.bdg_iso_assign_dev(None, None, None, 0, None, 1, None) == _native.E_ARG
