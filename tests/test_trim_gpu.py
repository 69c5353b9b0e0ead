"""Trimmed reads on the GPU: bdg_trim_batch and the device form against badger_amd/trim.py on every field of every read, the
pipelined path (submit / collect / collect_trim, with a forced queue overflow), and the command line end to end."""
import ctypes as C
import gzip
import logging
import os

import numpy as np
import pytest

from badger_amd import _native, common, extract_raw_barcodes as erb, synth, trim

pytestmark = pytest.mark.gpu

FIELDS = ("cdna_start", "cdna_end", "tail_len", "tso_score", "flags")


def _same(got, want, what):
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert not len(bad), (what, f, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def _adversarial(reads, seed, umi_len):
    """reads ending inside the tail, inside the TSO, with fewer than 64 bases behind the tail, of only T, with N, without a
    polyT, of 16 bases ..., each on both strands; plus reads of the error model cut anywhere"""
    rng = np.random.default_rng(seed)
    rs = lambda n, a="ACGT": "".join(a[c] for c in rng.integers(0, len(a), size=n))       # noqa: E731
    out = []
    for k in range(300):
        head = rs(int(rng.integers(0, 41))) + synth.R1 + rs(16) + rs(umi_len)
        cdna = rs(5, "ACG") + rs(int(rng.integers(0, 200)))
        kind = k % 10
        if kind == 0:
            s = head + "T" * int(rng.integers(1, 30))                                      # ends inside the tail
        elif kind == 1:
            s = head + "T" * 30 + cdna + trim.TSO[:int(rng.integers(1, 30))]               # ends inside the TSO
        elif kind == 2:
            s = head + "T" * 30 + cdna[:int(rng.integers(1, 34))] + trim.TSO               # fewer than 64 bases behind the tail
        elif kind == 3:
            s = "T" * int(rng.integers(16, 3000))
        elif kind == 4:
            s = list(head + "T" * 30 + cdna + trim.TSO)
            for _ in range(int(rng.integers(1, 8))):
                s[int(rng.integers(0, len(s)))] = "N"
            s = "".join(s)
        elif kind == 5:
            s = head + cdna + rs(300, "ACG") + trim.TSO                                    # no polyT
        elif kind == 6:
            s = head + "T" * 30 + cdna + rs(40, "T") + trim.TSO + rs(int(rng.integers(0, 12)))
        elif kind == 7:
            s = rs(int(rng.integers(16, 64)))
        elif kind == 8:
            s = head + "T" * 30 + "ATTTTTTT" + cdna + trim.TSO[3:]
        else:
            s = head + "T" * 12 + "N" + "T" * 17 + rs(int(rng.integers(6000, 7900))) + trim.TSO
        out.append(trim.revcomp(s) if k & 16 else s)
    for k in range(400):
        s = reads[k]
        out.append(s[:int(rng.integers(16, len(s)))] if k & 1 else s[int(rng.integers(0, len(s) - 16)):])
    out += [rs(16), head + "T" * 30 + rs(8000 - len(head) - 60) + trim.TSO]               # the shortest and the longest
    return out


_CACHE = {}


def _read_set(n, seed, umi_len):
    key = (n, seed, umi_len)
    if key not in _CACHE:
        wl = synth.make_whitelist(3000)
        b, o = synth.make_reads(n, wl, seed=seed, umi_len=umi_len, device="cuda", tso=True, tso_tail=(seed % 3) * 5)
        reads = synth.reads_to_list(b.cpu(), o.cpu())
        reads += _adversarial(reads, seed, umi_len)
        bases, off = synth.list_to_reads(reads)
        _CACHE[key] = (reads, bases, off)
    return _CACHE[key]


# ---- 1. parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("umi_len,seed", [(12, 71), (10, 72)])
def test_trim_batch_equals_the_rule(umi_len, seed):
    """2 x 52,700 reads (error model 3 % / 2 % / 3 %, both strands, 16 .. 8000 bases, the adversarial sets, invalid and
    placeholder records) at tso_min_score 8, 20 and 30: every field of every read"""
    reads, bases, off = _read_set(52000, seed, umi_len)
    lens = np.diff(off.astype(np.int64))
    assert lens.min() == 16 and lens.max() >= 8000 and len(reads) >= 52700
    ctx = _native.Context(0)
    recs = ctx.extract_batch(bases, off, umi_len)
    recs[5]["valid"] = 0
    recs[6]["flags"] |= _native.FLAG_INCOMPLETE
    recs[7]["polyT"] = -1
    n_tso = 0
    for score in (8, 20, 30):
        want = trim.trim_batch(bases, off, recs, score)
        got = ctx.trim_batch(bases, off, recs, score)
        _same(got, want, "trim_batch umi %d score %d" % (umi_len, score))
        n_tso += int(((want["flags"] & trim.TRIM_TSO) != 0).sum())
    # the one-read form of the rule on a sample (tests/test_trim.py holds the two forms equal)
    pick = np.random.default_rng(seed).choice(len(reads), 1500, replace=False)
    one = trim.trim_reads([reads[i] for i in pick], recs[pick], 30)
    _same(got[pick], one, "one-read form")
    assert n_tso > 60000 and (want["cdna_start"] == -1).sum() > 100 and ((want["flags"] & trim.TRIM_EMIT) != 0).sum() > 40000
    for bad in (7, 31):
        with pytest.raises(_native.BadgerHipError):
            ctx.trim_batch(bases[:int(off[4])], off[:5], recs[:4], bad)
    ctx.close()


def test_trim_batch_dev_behind_the_extraction():
    import torch
    reads, bases, off = _read_set(52000, 71, 12)
    n = len(reads)
    dev = torch.device("cuda", 0)
    total = int(off[-1])
    d_bases = torch.zeros((total + 15) // 16 * 16 + 64, dtype=torch.uint8, device=dev)
    d_bases[:total] = torch.from_numpy(bases).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_recs = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_out = torch.full((n * 12,), 0xAB, dtype=torch.uint8, device=dev)
    ctx = _native.Context(0)
    ctx.set_stream(0)
    for _ in range(8):
        ctx.extract_batch_dev(d_bases, d_off, n, total, 12, d_recs)
        ctx.trim_batch_dev(d_bases, d_off, n, d_recs, 20, d_out)
        rc, _, _ = ctx.extract_status()
        if rc != _native.E_CAPACITY:
            break
    assert rc == 0
    torch.cuda.synchronize()
    recs = d_recs.cpu().numpy().view(_native.REC_DTYPE)
    got = d_out.cpu().numpy().view(_native.TRIM_DTYPE)
    assert (recs == ctx.extract_batch(bases, off, 12)).all()
    _same(got, trim.trim_batch(bases, off, recs, 20), "trim_batch_dev")
    with pytest.raises(_native.BadgerHipError):
        ctx.trim_batch_dev(d_bases, d_off, n, d_recs, 31, d_out)
    ctx.close()


# ---- 2. the pipelined path ----------------------------------------------------------------------------------------------
def _pipeline(ctx, bases, off, n, step, umi_len):
    """the reads in chunks of `step` through the four slots, two in flight -> records, trim results, slots that were rerun"""
    recs, trims, flying = [], [], []

    def collect():
        slot, a, b, _ = flying.pop(0)
        recs.append(ctx.extract_collect(slot, b - a))
        trims.append(ctx.extract_collect_trim(slot, b - a))

    for k, a in enumerate(range(0, n, step)):
        b = min(a + step, n)
        if len(flying) >= 3:
            collect()
        o = np.ascontiguousarray(off[a:b + 1], dtype=np.uint64)       # (stays alive until the chunk is collected)
        ctx.extract_submit(k % _native.SLOTS, bases.ctypes.data, o.ctypes.data, b - a, umi_len)
        flying.append((k % _native.SLOTS, a, b, o))
    while flying:
        collect()
    return np.concatenate(recs), np.concatenate(trims)


def test_submit_collect_trim_and_overflow_rerun():
    reads, bases, off = _read_set(52000, 72, 10)
    n = 20000
    ctx = _native.Context(0)
    recs = ctx.extract_batch(bases[:int(off[n])], off[:n + 1], 10)
    want = ctx.trim_batch(bases[:int(off[n])], off[:n + 1], recs, 20)
    _same(want, trim.trim_batch(bases, off[:n + 1], recs, 20), "batch")
    ctx.extract_set_trim(True, 20)
    got_recs, got = _pipeline(ctx, bases, off, n, 1777, 10)
    assert (got_recs == recs).all()
    _same(got, want, "pipelined")
    # a queue far too small: every chunk overflows, is run again by collect, and its trim with it
    ctx.extract_set_queue_capacity(16)
    got_recs, got = _pipeline(ctx, bases, off, n, 2500, 10)
    ctx.extract_set_queue_capacity(0)
    assert (got_recs == recs).all() and not (got_recs["flags"] & _native.FLAG_INCOMPLETE).any()
    _same(got, want, "pipelined after the rerun")
    # off again: a chunk submitted without it has no trim to hand over
    ctx.extract_set_trim(False)
    o = np.ascontiguousarray(off[:101], dtype=np.uint64)
    ctx.extract_submit(0, bases.ctypes.data, o.ctypes.data, 100, 10)
    assert (ctx.extract_collect(0, 100) == recs[:100]).all()
    with pytest.raises(_native.BadgerHipError):
        ctx.extract_collect_trim(0, 100)
    with pytest.raises(_native.BadgerHipError):
        ctx.extract_set_trim(True, 7)
    ctx.close()


# ---- 3. the command line ------------------------------------------------------------------------------------------------
def _write_inputs(tmp_path, ids, reads):
    import bamio
    paths = {}
    paths["fa"] = str(tmp_path / "reads.fasta")
    with open(paths["fa"], "w") as f:
        f.write("".join(">%s some description\n%s\n" % (i, "\n".join(s[a:a + 70] for a in range(0, len(s), 70))) for i, s in zip(ids, reads)))
    paths["fq.gz"] = str(tmp_path / "reads.fastq.gz")
    with gzip.open(paths["fq.gz"], "wt") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in zip(ids, reads)))
    paths["bam"] = str(tmp_path / "reads.bam")
    open(paths["bam"], "wb").write(bamio.bgzf(bamio.bam_raw([(i, 4, s) for i, s in zip(ids, reads)]), block=30000))
    return paths


def _expected(ids, reads, recs, tr, tsv_rows, with_wl):
    from test_trim import _expected_fasta
    wl_col = [r.split("\t")[8] for r in tsv_rows] if with_wl else None
    return _expected_fasta(ids, reads, recs, tr, tsv_rows, wl_col)


@pytest.fixture(scope="module")
def cli_set(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("trim_cli")
    reads, _, _ = _read_set(52000, 71, 12)
    reads = reads[:2600] + reads[52000:52700:2]                  # error-model reads and adversarial ones
    ids = ["read_%d" % i for i in range(len(reads))]
    bases, off = synth.list_to_reads(reads)
    ctx = _native.Context(0)
    recs = ctx.extract_batch(bases, off, 12)
    ctx.close()
    wl = synth.make_whitelist(3000)
    wl = wl[np.random.default_rng(2).permutation(len(wl))]
    wl_path = str(tmp / "wl.txt")
    open(wl_path, "w").write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    return dict(tmp=tmp, ids=ids, reads=reads, bases=bases, off=off, recs=recs, wl=wl_path, paths=_write_inputs(tmp, ids, reads))


@pytest.mark.parametrize("fmt", ["fa", "fq.gz", "bam"])
@pytest.mark.parametrize("with_wl", [False, True])
def test_cli_end_to_end(cli_set, fmt, with_wl, monkeypatch, caplog, tmp_path):
    S = cli_set
    monkeypatch.setenv("BADGER_AMD_CONTEXTS_ON_ONE_DEVICE", "1")
    monkeypatch.setenv("BADGER_AMD_SEGMENT_MB", "1")
    base = ["--mode", "tenX_v3", "-i", S["paths"][fmt], "-t", "1"] + (["-b", S["wl"], "--bc_candidates", "3"] if with_wl else [])
    plain = str(tmp_path / "plain.tsv")
    erb.main(base + ["-o", plain])
    rows = open(plain).read().split("\n")[1:-1]
    assert [r.split("\t")[0] for r in rows] == S["ids"]
    for gpus, score in (("1", None), ("2", 12)):
        tr = trim.trim_batch(S["bases"], S["off"], S["recs"], 20 if score is None else score)
        want = _expected(S["ids"], S["reads"], S["recs"], tr, rows, with_wl)
        out, fa = str(tmp_path / ("t%s.tsv" % gpus)), str(tmp_path / ("t%s.fa" % gpus))
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="BarcodeGraph"):
            erb.main(base + ["-o", out, "--gpus", gpus, "--trimmed_reads", fa] + ([] if score is None else ["--tso_min_score", str(score)]))
        got = open(fa, "rb").read()
        assert got == want, (fmt, with_wl, gpus)
        assert open(out, "rb").read() == open(plain, "rb").read()
        assert open(out + ".stats", "rb").read() == open(plain + ".stats", "rb").read()
        emit = (tr["flags"] & trim.TRIM_EMIT) != 0
        line = "Trimmed reads: %d written to %s, %d with the TSO cut off, %d bases" % (
            int(emit.sum()), fa, int((emit & ((tr["flags"] & trim.TRIM_TSO) != 0)).sum()),
            int((tr["cdna_end"][emit] - tr["cdna_start"][emit]).sum()))
        assert any(line in r.getMessage() for r in caplog.records), [r.getMessage() for r in caplog.records][-4:]
        assert got.count(b"\n") == 2 * int(emit.sum()) and (b"\tCB:Z:" in got) == with_wl
        assert not os.path.exists(plain + ".trimmed") and sorted(os.listdir(str(tmp_path))).count("t%s.fa" % gpus) == 1


def test_small_chunks_many_contexts_and_the_correction(cli_set, tmp_path):
    """bdg_stage1_run directly: chunks of 257 reads over three contexts, several reader and formatter threads, a header every
    1000 reads, with the whitelist correction: the trimmed file is the same, the other files are those of the run without"""
    S = cli_set
    wl = erb.load_barcodes(S["wl"])
    ctxs = [_native.Context(0) for _ in range(3)]
    for c in ctxs:
        c.whitelist_load(wl)
    header = "#read_id\tbarcode\tUMI\tBC_score\tvalid_UMI\tstrand\tpolyT_start\tR1_end\twhitelist_barcode\twhitelist_dist\twhitelist_ties"
    kw = dict(threads=3, header_every=1000, chunk_reads=257, format_threads=3, whitelist=True, max_bc_dist=2)
    a, b, fa = str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv"), str(tmp_path / "b.fa")
    ra = _native.stage1_run(ctxs[:1], S["paths"]["fq.gz"], a, header, 12, corrected_path=a + ".corr", **kw)
    rb = _native.stage1_run(ctxs, S["paths"]["fq.gz"], b, header, 12, corrected_path=b + ".corr", trimmed_path=fa, tso_min_score=25, **kw)
    assert open(a, "rb").read() == open(b, "rb").read() and open(a + ".corr", "rb").read() == open(b + ".corr", "rb").read()
    assert (ra.reads, ra.whitelist_barcodes, ra.whitelist_corrected) == (rb.reads, rb.whitelist_barcodes, rb.whitelist_corrected)
    rows = [r for r in open(a).read().split("\n")[:-1] if not r.startswith("#")]
    tr = trim.trim_batch(S["bases"], S["off"], S["recs"], 25)
    want = _expected(S["ids"], S["reads"], S["recs"], tr, rows, True)
    assert open(fa, "rb").read() == want
    emit = (tr["flags"] & trim.TRIM_EMIT) != 0
    assert (rb.trimmed_reads, rb.trimmed_bases) == (int(emit.sum()), int((tr["cdna_end"][emit] - tr["cdna_start"][emit]).sum()))
    assert rb.chunks >= len(S["reads"]) // 257
    # without a whitelist, and a caller that sets the fields but not the bit: they are not read
    c = str(tmp_path / "c.tsv")
    plain_header = header.split("\twhitelist_barcode")[0]
    rc0 = _native.stage1_run(ctxs[:2], S["paths"]["bam"], c, plain_header, 12, chunk_reads=300, trimmed_path=fa + "2")
    rows_c = open(c).read().split("\n")[1:-1]
    assert open(fa + "2", "rb").read() == _expected(S["ids"], S["reads"], S["recs"], trim.trim_batch(S["bases"], S["off"], S["recs"]), rows_c, False)
    assert rc0.trimmed_reads > 2000
    L = _native.load()
    o = _native.Stage1OptsTrim(12, 1, 0, 0, 300, 0, 0, 0, 0, 0, 0, 0, None, b"/nonexistent/dir/x.fa", 999, 0)
    res = _native.Stage1ResultTrim()
    res.trimmed_reads = 12345
    d = str(tmp_path / "d.tsv")
    arr = (C.c_void_p * 1)(ctxs[0].h)
    rc = L.bdg_stage1_run(arr, 1, os.fsencode(S["paths"]["bam"]), os.fsencode(d), plain_header.encode(),
                          C.cast(C.pointer(o), C.POINTER(_native.Stage1Opts)), C.cast(C.pointer(res), C.POINTER(_native.Stage1Result)))
    assert rc == 0 and open(d, "rb").read() == open(c, "rb").read() and res.trimmed_reads == 12345
    # with the bit the fields are checked
    for path, score in ((None, 20), (b"/nonexistent/dir/x.fa", 20), (os.fsencode(fa + "3"), 31)):
        o = _native.Stage1OptsTrim(12, 1, 0, 0, 300, 0, 0, _native.STAGE1_TRIM, 0, 0, 0, 0, None, path, score, 0)
        rc = L.bdg_stage1_run(arr, 1, os.fsencode(S["paths"]["bam"]), os.fsencode(d), plain_header.encode(),
                              C.cast(C.pointer(o), C.POINTER(_native.Stage1Opts)), C.cast(C.pointer(res), C.POINTER(_native.Stage1Result)))
        assert rc == _native.E_ARG
    for c_ in ctxs:
        c_.close()
