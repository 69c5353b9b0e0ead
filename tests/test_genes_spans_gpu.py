"""The span forms of the gene-call and isoform kernels (k_genes_assign_spans, k_iso_assign_spans, k_cdna_spans of
csrc/genes_kernels.hip) against the rule of badger_amd/genes.py and against the forward kernels on the materialised
sequences: every field of every record.  Span lengths around k, the wave's 64 windows and the four chunks a wave has in flight;
spans at the read's start, at its end, inside it between bases that would change the answer, and past both ends; N at the
span's ends and middle, homopolymers; no read, one read and more reads than resident waves; a table of 64 slots with a wrap and
one of thousands; reads without a gene, whose bytes are poison; k_cdna_spans on the hand-derived records; the same answer twice
and in another order; the argument errors over poisoned outputs; and bdg_extract_keep_genes through bdg_stage1_collect, with and
without every chunk rerun."""
import numpy as np
import pytest

import genes_cases as gc
import iso_cases as ic
from badger_amd import _native, synth
from badger_amd import genes as gn
from span_cases import hand_arrays

pytestmark = pytest.mark.gpu

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


def _revcomp(s):
    return gn.span_sequence(s, 0, len(s), 1).decode()


def _host(ctx, reads, spans, min_hits, margin):
    g, i = ctx.genes_assign_spans(*_flat(reads), spans, min_hits, margin)
    return gc.rec_tuples(g), ic.iso_tuples(i)


def _dev(ctx, reads, spans, min_hits, margin):
    """bdg_genes_assign_spans_dev, then bdg_iso_assign_spans_dev over its records, both outputs poisoned first"""
    bases, off = _flat(reads)
    n = len(reads)
    d = [_native.DeviceArray.from_host(ctx, a) for a in (bases, off, spans, np.full(max(n, 1) * 6, POISON, np.uint32),
                                                         np.full(max(n, 1) * 8, POISON, np.uint32))]
    try:
        ctx.genes_assign_spans_dev(d[0], d[1], n, d[2], min_hits, d[3])
        ctx.iso_assign_spans_dev(d[0], d[1], n, d[2], d[3], margin, d[4])
        return gc.rec_tuples(d[3].to_host().view(_native.GENE_DTYPE)[:n]), ic.iso_tuples(d[4].to_host().view(_native.ISO_DTYPE)[:n])
    finally:
        for a in d:
            a.free()


def _check(ctx, index, reads, spans, min_hits, margin, what, runs=(_host, _dev)):
    """the span kernels against the checker and against the forward kernels on the materialised sequences -> the records"""
    spans = np.asarray(spans, dtype=_native.SPAN_DTYPE)
    seqs = gn.span_sequences(reads, spans)
    rule = gn.assign_spans(index, reads, spans, min_hits, margin)
    want = gc.rec_tuples(rule[0]), ic.iso_tuples(rule[1])
    g, i = ctx.iso_assign(*_flat(seqs), min_hits, margin)
    assert (gc.rec_tuples(g), ic.iso_tuples(i)) == want, what + ": the forward kernels and the checker differ"
    for run in runs:
        got = run(ctx, reads, spans, min_hits, margin)
        for kind in (0, 1):
            for r, (a, b) in enumerate(zip(got[kind], want[kind])):
                assert a == b, "%s, %s, %s record of read %d, span %r (%d bases):\n  device  %r\n  checker %r" % (
                    what, run.__name__, ("gene", "isoform")[kind], r, tuple(spans[r].tolist()), len(seqs[r]), a, b)
    return want


def _place(window, d, length, rc):
    """a read that holds the sequence window[d:d + length] as a span, and that span: the window as it stands, or its reverse
    complement, in which the span lies mirrored"""
    if rc:
        return _revcomp(window), (len(window) - d - length, len(window) - d, 1)
    return window, (d, d + length, 0)


@pytest.fixture(scope="module")
def model():
    """a gene of two transcripts that differ in one base, a polyA transcript of its own gene, and a second gene"""
    rng = np.random.default_rng(17)
    text = gc.rand_seq(rng, 1300)
    other = text[:620] + ("A" if text[620] != "A" else "C") + text[621:]
    return dict(seqs=[text, other, "A" * 80, gc.rand_seq(rng, 500)], feats=[5, 5, 7, 9], local=[0, 1, 0, 0], text=text)


def _build(ctx, m, k):
    ctx.genes_index_build_iso(*_flat(m["seqs"]), np.asarray(m["feats"], np.uint32), np.asarray(m["local"], np.uint8), k)
    return gn.build_index(m["seqs"], m["feats"], k, m["local"])


def test_span_layout():
    assert _native.SPAN_DTYPE.itemsize == 12 and _native.SPAN_DTYPE.names == ("begin", "end", "rc")


@pytest.mark.parametrize("rc", (0, 1))
@pytest.mark.parametrize("k", (11, 21, 31))
def test_lengths_and_positions(ctx, model, k, rc):
    index = _build(ctx, model, k)
    text = model["text"]
    lengths = [0, k - 1, k, k + 1, 63, 64, 65, 64 + k - 1, 255, 256, 257, 1000]
    reads, spans = [], []
    for j, L in enumerate(lengths):
        p = 100 + 3 * j                                            # the span's sequence is text[p:p + L]
        for lo, hi in ((0, 40), (40, 0), (40, 40)):                # at the read's start, at its end, inside it: the bases on either
            r, sp = _place(text[p - lo:p + L + hi], lo, L, rc)     # side go on in the same transcript - read, they would add hits
            reads.append(r)
            spans.append(sp)
        r, sp = _place(text[p:p + L], 0, L, rc)                    # coordinates past both ends of the read
        reads.append(r)
        spans.append((sp[0] - 7, sp[1] + 9, rc))
        r, sp = _place("acgtgca" * 6 + text[p:p + L] + "ttgacca" * 6, 42, L, rc)     # lower case on either side
        reads.append(r)
        spans.append(sp)
    want = _check(ctx, index, reads, spans, 1, 1, "k %d rc %d" % (k, rc))
    for j, L in enumerate(lengths):
        n = max(L - k + 1, 0)
        for g, i in zip(want[0][5 * j:5 * j + 5], want[1][5 * j:5 * j + 5]):
            assert g[3] == g[4] == n and g[1] == n and (g[0] == 5) == (n > 0) and i[4] == n       # the span's windows and no other


@pytest.mark.parametrize("rc", (0, 1))
def test_content_and_reads_without_a_gene(ctx, model, rc):
    k = 21
    index = _build(ctx, model, k)
    text, second = model["text"], model["seqs"][3]
    reads, spans = [], []
    for L in (100, 300):
        for at in (0, L - 1, L // 2):                              # N at the span's first, last and a middle position
            x = text[200:200 + L]
            r, sp = _place(text[150:200] + x[:at] + "N" + x[at + 1:] + text[200 + L:260 + L], 50, L, rc)
            reads.append(r)
            spans.append(sp)
    for base, L in (("A", 64), ("A", 300), ("T", 100), ("C", 257)):   # homopolymers: polyA is a transcript, the others are in none
        r, sp = _place(text[:30] + base * L + text[30:60], 30, L, rc)
        reads.append(r)
        spans.append(sp)
    # reads without an assigned gene between assigned ones: a span over lower case, over random bases, too short a span,
    # a tie between two genes - and the whole read of each is poison
    rng = np.random.default_rng(3)
    nogene = [("acgtacgtgg" * 20, (0, 200)), (gc.rand_seq(rng, 150).lower(), (10, 140)), ("tgcatgcaac" * 8, (30, 30 + k - 1)),
              ("gattacagat" * 9, (-5, 400))]
    for r, (b, e) in nogene:
        reads += [r, text[700:900] if not rc else _revcomp(text[700:900])]
        spans += [(b, e, rc), (0, 200, rc)]
    tie, sp = _place("ttgacc" * 5 + text[40:40 + k + 3] + "N" + second[40:40 + k + 3] + "ccagtt" * 5, 30, 2 * k + 7, rc)
    reads.append(tie)
    spans.append(sp)
    want = _check(ctx, index, reads, spans, 3, 1, "content rc %d" % rc)
    assert [g[3] for g in want[0][:6]] == [100 - k, 100 - k, 100 - 2 * k + 1, 300 - k, 300 - k, 300 - 2 * k + 1]   # windows with a key
    assert [g[0] for g in want[0][6:10]] == [7, 7, gn.NONE, gn.NONE]
    assert all(i[5] == gn.ISO_NOGENE for i in want[1][10:18:2]) and all(i[5] != gn.ISO_NOGENE for i in want[1][11:18:2])
    assert want[0][18][5] == gn.TIE and want[1][18][5] == gn.ISO_NOGENE


def test_batch_sizes(ctx, model):
    k = 11
    index = _build(ctx, model, k)
    text = model["text"]
    empty = np.zeros(0, dtype=_native.SPAN_DTYPE)
    assert _host(ctx, [], empty, 1, 1) == ([], []) and _dev(ctx, [], empty, 1, 1) == ([], [])
    _check(ctx, index, [text[5:70]], [(3, 60, 0)], 1, 1, "one read")
    # more reads than waves are resident: every wave takes several
    n = 20000
    rng = np.random.default_rng(8)
    start = rng.integers(0, len(text) - 20, size=n)
    rcs = rng.integers(0, 2, size=n)
    reads = [text[s:s + 20] if not c else _revcomp(text[s:s + 20]) for s, c in zip(start.tolist(), rcs.tolist())]
    spans = np.zeros(n, dtype=_native.SPAN_DTYPE)
    spans["begin"], spans["end"], spans["rc"] = rng.integers(0, 4, size=n), 20 - rng.integers(0, 4, size=n), rcs
    # (the checker takes a read at a time: the forward kernels on the materialised spans are the reference here, and the checker
    # on a sample)
    seqs = gn.span_sequences(reads, spans)
    g, i = ctx.iso_assign(*_flat(seqs), 2, 1)
    for run in (_host, _dev):
        got = run(ctx, reads, spans, 2, 1)
        assert got[0] == gc.rec_tuples(g) and got[1] == ic.iso_tuples(i), run.__name__
    sample = list(range(0, n, 97))
    rule = gn.assign_spans(index, [reads[j] for j in sample], spans[sample], 2, 1)
    assert gc.rec_tuples(rule[0]) == gc.rec_tuples(g[sample]) and ic.iso_tuples(rule[1]) == ic.iso_tuples(i[sample])
    assert (g["flags"] & gn.ASSIGNED != 0).sum() > n // 2
    # the same answer twice, and with the reads in another order
    again = _dev(ctx, reads, spans, 2, 1)
    assert again == got
    order = rng.permutation(n)
    shuffled = _dev(ctx, [reads[j] for j in order.tolist()], spans[order], 2, 1)
    assert shuffled[0] == [got[0][j] for j in order.tolist()] and shuffled[1] == [got[1][j] for j in order.tolist()]


def test_a_table_of_64_slots_with_a_wrap(ctx):
    rng = np.random.default_rng(5)
    k, wraps = 11, 0
    for _ in range(60):
        seqs, feats = gc.tiny_index_case(rng, k, int(rng.integers(20, 33)))
        local = gn.local_indices(feats)[0]
        ctx.genes_index_build_iso(*_flat(seqs), np.asarray(feats, np.uint32), local, k)
        stats = ctx.genes_index_stats()
        if int(stats[3]) != 64 or int(stats[5]) == 0:
            continue
        wraps += 1
        index = gn.build_index(seqs, feats, k, local)
        reads, spans = [], []
        for s in seqs:
            for rc in (0, 1):
                r, sp = _place("ca" * 4 + s + "tg" * 4, 8, len(s), rc)
                reads.append(r)
                spans.append(sp)
        _check(ctx, index, reads, spans, 1, 1, "64 slots", runs=(_dev,))
        if wraps == 5:
            break
    assert wraps == 5


def test_cdna_spans_on_the_hand_derived_records(ctx):
    reads, recs, trim, chim = hand_arrays()
    _, off = _flat(reads)
    n = len(reads)
    for with_chim in (True, False):
        want = gn.spans_of_records([len(r) for r in reads], recs, trim, chim if with_chim else None)
        d = [_native.DeviceArray.from_host(ctx, a) for a in (off, recs, trim, chim, np.full(3 * n, POISON, np.uint32))]
        try:
            ctx.cdna_spans_dev(d[0], n, d[1], d[2], d[3] if with_chim else None, d[4])
            got = d[4].to_host().view(_native.SPAN_DTYPE)
        finally:
            for a in d:
                a.free()
        assert got.tolist() == want.tolist(), with_chim


def test_argument_errors_leave_the_outputs_alone(model):
    fresh = _native.Context(0)
    try:
        reads = [model["text"][:100]] * 3
        bases, off = _flat(reads)
        spans = np.array([(0, 100, 0)] * 3, dtype=_native.SPAN_DTYPE)
        d = [_native.DeviceArray.from_host(fresh, a) for a in (bases, off, spans, np.full(18, POISON, np.uint32), np.full(24, POISON, np.uint32))]

        def refused(call, *args):
            with pytest.raises(_native.BadgerHipError):
                call(*args)
            assert (d[3].to_host() == POISON).all() and (d[4].to_host() == POISON).all()

        refused(fresh.genes_assign_spans_dev, d[0], d[1], 3, d[2], 1, d[3])             # no index
        refused(fresh.iso_assign_spans_dev, d[0], d[1], 3, d[2], d[3], 1, d[4])
        refused(fresh.genes_assign_spans, bases, off, spans, 1, 0)
        refused(fresh.extract_keep_genes, True, 3, 0)
        fresh.genes_index_build(*_flat(model["seqs"]), np.asarray(model["feats"], np.uint32), 21)
        refused(fresh.genes_assign_spans_dev, d[0], d[1], 3, d[2], 0, d[3])             # min_hits 0
        refused(fresh.genes_assign_spans_dev, d[0], d[1], 3, 0, 1, d[3])                # null pointers
        refused(fresh.genes_assign_spans_dev, d[0], 0, 3, d[2], 1, d[3])
        refused(fresh.genes_assign_spans_dev, d[0], d[1], 3, d[2], 1, 0)
        refused(fresh.iso_assign_spans_dev, d[0], d[1], 3, d[2], d[3], 1, d[4])         # an index without masks
        refused(fresh.genes_assign_spans, bases, off, spans, 1, 1)
        refused(fresh.genes_assign_spans, bases, off[::-1].copy(), spans, 1, 0)         # offsets that decrease
        refused(fresh.extract_keep_genes, True, 3, 0)                                   # the trim is off
        fresh.extract_set_trim(True, 20)
        refused(fresh.extract_keep_genes, True, 0, 0)
        refused(fresh.extract_keep_genes, True, 3, 1)                                   # a margin without masks
        fresh.extract_keep_genes(True, 3, 0)
        fresh.extract_set_trim(False)
        fresh.genes_index_build_iso(*_flat(model["seqs"]), np.asarray(model["feats"], np.uint32), np.asarray(model["local"], np.uint8), 21)
        refused(fresh.iso_assign_spans_dev, d[0], d[1], 3, d[2], d[3], 0, d[4])         # margin 0
        refused(fresh.iso_assign_spans_dev, d[0], d[1], 3, 0, d[3], 1, d[4])
        refused(fresh.iso_assign_spans_dev, d[0], d[1], 3, d[2], 0, 1, d[4])
        refused(fresh.cdna_spans_dev, d[1], 3, 0, d[2], None, d[3])
        # n = 0 is no error and touches nothing
        fresh.genes_assign_spans_dev(0, 0, 0, 0, 1, 0)
        fresh.iso_assign_spans_dev(0, 0, 0, 0, 0, 1, 0)
        fresh.cdna_spans_dev(0, 0, 0, 0, None, 0)
        assert fresh.kept_genes() == (0, 0, 0)
        for a in d:
            a.free()
    finally:
        fresh.close()


# ---- bdg_extract_keep_genes --------------------------------------------------------------------------------------------
N_READS, TSO_MIN, CHIM_ED, K = 600, 20, 3, 21


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """synth reads with a TSO, a few of them chimeras, as a FASTA; their records from the one-shot wrappers; and transcripts made
    of the cDNA of every third read, two reads a gene, so that most reads have a gene and an isoform"""
    wl = synth.make_whitelist(500)
    b, o = synth.make_reads(N_READS, wl, seed=77, tso=True)
    reads = synth.reads_to_list(b, o)
    for j in range(30):
        reads.append(reads[2 * j] + reads[2 * j + 1])
    bases, off = synth.list_to_reads(reads)
    path = str(tmp_path_factory.mktemp("keep_genes") / "reads.fa")
    with open(path, "w") as f:
        f.write("".join(">r%d\n%s\n" % (i, s if isinstance(s, str) else s.decode()) for i, s in enumerate(reads)))
    c = _native.Context(0)
    try:
        recs = c.extract_batch(bases, off, 12)
        trim = c.trim_batch(bases, off, recs, TSO_MIN)
        chim = c.chimera_batch(bases, off, recs, trim, CHIM_ED)
    finally:
        c.close()
    lengths = np.diff(off.astype(np.int64))
    plain = gn.span_sequences(reads, gn.spans_of_records(lengths, recs, trim, None))
    tx = [s.decode() for s in plain[::3] if len(s) > 60]
    feats = np.arange(len(tx), dtype=np.uint32) // 2
    assert len(tx) > 100
    return dict(path=path, reads=reads, bases=bases, off=off, lengths=lengths, recs=recs, trim=trim, chim=chim, tx=tx, feats=feats,
                local=gn.local_indices(feats)[0])


@pytest.mark.parametrize("chimera_on, margin", ((True, 1), (False, 0)))
def test_kept_gene_records_through_stage1_collect(library, chimera_on, margin):
    S = library
    n = len(S["reads"])
    chim = S["chim"] if chimera_on else None
    spans = gn.spans_of_records(S["lengths"], S["recs"], S["trim"], chim)
    index = gn.build_index(S["tx"], S["feats"], K, S["local"])
    rule = gn.assign_spans(index, S["reads"], spans, 3, margin or None)
    want_gene, want_iso = (rule if margin else (rule, None))
    ctx = _native.Context(0)
    try:
        if margin:
            ctx.genes_index_build_iso(*_flat(S["tx"]), S["feats"], S["local"], K)
        else:
            ctx.genes_index_build(*_flat(S["tx"]), S["feats"], K)
        # the span kernels on the whole input
        whole = ctx.genes_assign_spans(S["bases"], S["off"], spans, 3, margin)
        assert gc.rec_tuples(whole[0] if margin else whole) == gc.rec_tuples(want_gene)
        if margin:
            assert ic.iso_tuples(whole[1]) == ic.iso_tuples(want_iso)
        # (a synth read's cDNA is its own: the reads the transcripts were made of have a gene, and a chimera's second half)
        assert (want_gene["flags"] & gn.ASSIGNED != 0).sum() > len(S["tx"]) * 3 // 4 and (want_gene["n_keys"] == 0).sum() > 0
        if chimera_on:
            assert ((S["chim"]["flags"] & _native.CHIMERA_HIT) != 0).sum() > 10
        for queue in (0, 16):                                      # 16: every chunk overflows and is run again by collect
            ctx.extract_keep_records(True)
            ctx.extract_set_trim(True, TSO_MIN)
            if chimera_on:
                ctx.extract_set_chimera(True, CHIM_ED)
            ctx.extract_keep_genes(True, 3, margin)
            ctx.extract_set_queue_capacity(queue)
            try:
                ids = _native.IdStore()
                res = _native.stage1_collect(ctx, S["path"], 12, ids, chunk_reads=256)
            finally:
                ctx.extract_set_queue_capacity(0)
                ctx.extract_set_trim(False)                         # (the chimera search and the keeping go off with it)
            assert res.reads == n and res.chunks >= 3 and len(ids) == n
            d_gene, d_iso, kept = ctx.kept_genes()
            assert kept == n == ctx.kept_records()[1] and (d_iso != 0) == bool(margin)
            assert (ctx.kept_records_to_host() == S["recs"]).all()
            got = ctx.device_to_host(d_gene, n, _native.GENE_DTYPE)
            assert gc.rec_tuples(got) == gc.rec_tuples(want_gene), queue
            if margin:
                assert ic.iso_tuples(ctx.device_to_host(d_iso, n, _native.ISO_DTYPE)) == ic.iso_tuples(want_iso), queue
        # the trim went off and the keeping with it: a further chunk adds records and no gene record
        o = np.ascontiguousarray(S["off"][:101], dtype=np.uint64)
        ctx.extract_submit(0, S["bases"].ctypes.data, o.ctypes.data, 100, 12)
        ctx.extract_collect(0, 100)
        assert ctx.kept_genes()[2] == n and ctx.kept_records()[1] == n + 100
        ctx.extract_keep_records(False)                             # frees
        assert ctx.kept_genes() == (0, 0, 0)
    finally:
        ctx.close()
