"""Chimeric reads on the GPU: bdg_chimera_batch and the device form against badger_amd/chimera.py on every field of every read,
the pipelined path (with a forced queue overflow), the command line end to end, and bdg_stage1_run directly."""
import ctypes as C
import logging
import os

import numpy as np
import pytest

import chimera_cases as cc
from badger_amd import _native, chimera, common, extract_raw_barcodes as erb, synth, trim

pytestmark = pytest.mark.gpu

FIELDS = ("cut", "hit_pos", "hit_ed", "hit_kind", "flags", "reserved")
E = chimera.MAX_ED_DEFAULT


def _same(got, want, what):
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert not len(bad), (what, f, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


_CACHE = {}


def _read_set(umi_len, seed):
    """10,000 reads of the error model, 300 chimeras made of pairs of them (head to tail and head to head, either strand), and
    the case set -> reads, bases, off, records (extraction's for the first two, hand-made for the cases), trim results, and
    the rule's records at max_ed 0, the default and 6 (one scan, shared by the tests)"""
    key = (umi_len, seed)
    if key in _CACHE:
        return _CACHE[key]
    wl = synth.make_whitelist(3000)
    b, o = synth.make_reads(10000, wl, seed=seed, umi_len=umi_len, device="cuda", tso=True)
    reads = synth.reads_to_list(b.cpu(), o.cpu())
    for k in range(300):
        x, y = reads[2 * k], reads[2 * k + 1]
        reads.append(x + (y if k & 1 else trim.revcomp(y)) if k & 2 else (trim.revcomp(y) if k & 1 else y) + x)
    n_real = len(reads)
    S = cc.case_set()
    reads = reads + S["reads"]
    bases, off = synth.list_to_reads(reads)
    ctx = _native.Context(0)
    recs = ctx.extract_batch(bases, off, umi_len)
    tr = ctx.trim_batch(bases, off, recs)
    ctx.close()
    recs[n_real:], tr[n_real:] = S["recs"], S["trim"]
    want = dict(zip((0, E, 6), chimera.chimera_batch_multi(bases, off, recs, tr, [0, E, 6])))
    _CACHE[key] = dict(reads=reads, bases=bases, off=off, recs=recs, trim=tr, want=want, n_real=n_real)
    return _CACHE[key]


# ---- 1. parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("umi_len,seed", [(12, 81), (10, 82)])
def test_chimera_batch_equals_the_rule(umi_len, seed):
    R = _read_set(umi_len, seed)
    ctx = _native.Context(0)
    for e in (0, E, 6):
        got = ctx.chimera_batch(R["bases"], R["off"], R["recs"], R["trim"], e)
        _same(got, R["want"][e], "chimera_batch umi %d max_ed %d" % (umi_len, e))
        again = ctx.chimera_batch(R["bases"], R["off"], R["recs"], R["trim"], e)
        assert got.tobytes() == again.tobytes()
    w = R["want"][E]
    hit = w["flags"] != 0
    # (the pairs are joined as sequenced: the molecule extraction picks lies in front of the junction in about three of four)
    assert hit[10000:10300].sum() > 150 and hit[:10000].sum() < 10 and set(w["hit_kind"][hit].tolist()) == {0, 1, 2, 3}
    assert (R["want"][6]["flags"] != 0).sum() > hit.sum() > (R["want"][0]["flags"] != 0).sum() > 200
    with pytest.raises(_native.BadgerHipError):
        ctx.chimera_batch(R["bases"][:int(R["off"][4])], R["off"][:5], R["recs"][:4], R["trim"][:4], 7)
    assert len(ctx.chimera_batch(R["bases"][:0], R["off"][:1], R["recs"][:0], R["trim"][:0], E)) == 0
    ctx.close()


def test_chimera_batch_dev_behind_extraction_and_trim():
    import torch
    R = _read_set(12, 81)
    n = R["n_real"]
    bases, off = R["bases"], R["off"][:n + 1]
    dev = torch.device("cuda", 0)
    total = int(off[-1])
    d_bases = torch.zeros((total + 15) // 16 * 16 + 64, dtype=torch.uint8, device=dev)
    d_bases[:total] = torch.from_numpy(bases[:total]).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_recs = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_trim = torch.zeros(n * 12, dtype=torch.uint8, device=dev)
    d_out = torch.full((n * 12,), 0xAB, dtype=torch.uint8, device=dev)
    ctx = _native.Context(0)
    ctx.set_stream(0)
    for _ in range(8):
        ctx.extract_batch_dev(d_bases, d_off, n, total, 12, d_recs)
        ctx.trim_batch_dev(d_bases, d_off, n, d_recs, 20, d_trim)
        ctx.chimera_batch_dev(d_bases, d_off, n, d_recs, d_trim, E, d_out)
        rc, _, _ = ctx.extract_status()
        if rc != _native.E_CAPACITY:
            break
    assert rc == 0
    torch.cuda.synchronize()
    assert (d_recs.cpu().numpy().view(_native.REC_DTYPE) == R["recs"][:n]).all()
    assert (d_trim.cpu().numpy().view(_native.TRIM_DTYPE) == R["trim"][:n]).all()
    _same(d_out.cpu().numpy().view(_native.CHIMERA_DTYPE), R["want"][E][:n], "chimera_batch_dev")
    with pytest.raises(_native.BadgerHipError):
        ctx.chimera_batch_dev(d_bases, d_off, n, d_recs, d_trim, 7, d_out)
    ctx.close()


def test_every_byte_alignment_of_a_unit():
    """the walk over a unit's words masks other bytes at every address mod 4 of the unit's first byte: the boundary cases (an
    exact occurrence at every scan step from -(m + k) to +1 around a segment border, both strands) behind one more read of
    0 .. 3 bases that takes no part, against the one-read rule"""
    S = cc.case_set()
    idx = [i for i, label in enumerate(S["labels"]) if label[0] == "boundary"]
    assert 200 < len(idx) < 600
    reads, recs, tr = [S["reads"][i] for i in idx], S["recs"][idx], S["trim"][idx]
    kinds = np.array([S["labels"][i][1] for i in idx])
    seen = {}

    def distances(pat, text):                                          # (the rule's scan once for both bounds)
        if (pat, text) not in seen:
            seen[pat, text] = chimera.start_distances(pat, text)
        return seen[pat, text]

    want = {e: chimera.chimera_reads(reads, recs, tr, e, distances) for e in (E, 6)}
    ctx = _native.Context(0)
    for shift in range(4):
        bases, off = synth.list_to_reads(["ACG"[:shift]] + reads)
        assert int(off[1]) == shift
        r = np.concatenate([np.zeros(1, recs.dtype), recs])
        t = np.concatenate([np.zeros(1, tr.dtype), tr])                # (no TRIM_EMIT: the leading read is not searched)
        for e in (E, 6):
            w = np.concatenate([np.array([chimera.NONE], dtype=chimera.CHIMERA_DTYPE), want[e]])
            planted = tr["cdna_start"] + 60                            # (the column of the occurrence's first base: chimera_cases)
            assert (w["flags"][1:] == chimera.CHIMERA_HIT).all() and (w["hit_ed"][1:] == 0).all()
            assert (w["hit_pos"][1:] == planted).all() and (w["hit_kind"][1:] == kinds).all() and (w["cut"][1:] <= planted).all()
            _same(ctx.chimera_batch(bases, off, r, t, e), w, "shift %d max_ed %d" % (shift, e))
    ctx.close()


# ---- 2. the pipelined path ----------------------------------------------------------------------------------------------
def _pipeline(ctx, bases, off, n, step, umi_len):
    recs, trims, chims, flying = [], [], [], []

    def collect():
        slot, a, b, _ = flying.pop(0)
        recs.append(ctx.extract_collect(slot, b - a))
        trims.append(ctx.extract_collect_trim(slot, b - a))
        chims.append(ctx.extract_collect_chimera(slot, b - a))

    for k, a in enumerate(range(0, n, step)):
        b = min(a + step, n)
        if len(flying) >= 3:
            collect()
        o = np.ascontiguousarray(off[a:b + 1], dtype=np.uint64)       # (stays alive until the chunk is collected)
        ctx.extract_submit(k % _native.SLOTS, bases.ctypes.data, o.ctypes.data, b - a, umi_len)
        flying.append((k % _native.SLOTS, a, b, o))
    while flying:
        collect()
    return np.concatenate(recs), np.concatenate(trims), np.concatenate(chims)


def test_submit_collect_chimera_and_overflow_rerun():
    R = _read_set(10, 82)
    bases, off = R["bases"], R["off"]
    n = len(R["reads"])                                                # the case reads too, under the records extraction gives them
    ctx = _native.Context(0)
    recs = ctx.extract_batch(bases, off, 10)
    tr = ctx.trim_batch(bases, off, recs)
    want = ctx.chimera_batch(bases, off, recs, tr, E)
    _same(want[:R["n_real"]], R["want"][E][:R["n_real"]], "batch")
    with pytest.raises(_native.BadgerHipError):
        ctx.extract_set_chimera(True, E)                               # the trim is off
    ctx.extract_set_trim(True, 20)
    with pytest.raises(_native.BadgerHipError):
        ctx.extract_set_chimera(True, 7)
    ctx.extract_set_chimera(True, E)
    got_recs, got_tr, got = _pipeline(ctx, bases, off, n, 1777, 10)
    assert (got_recs == recs).all() and (got_tr == tr).all()
    _same(got, want, "pipelined")
    ctx.extract_set_queue_capacity(16)                                 # every chunk overflows and is run again by collect
    got_recs, got_tr, got = _pipeline(ctx, bases, off, n, 2500, 10)
    ctx.extract_set_queue_capacity(0)
    assert (got_recs == recs).all() and (got_tr == tr).all()
    _same(got, want, "pipelined after the rerun")
    ctx.extract_set_chimera(False)                                     # off: the trim is still handed over, no search
    o = np.ascontiguousarray(off[:101], dtype=np.uint64)
    ctx.extract_submit(0, bases.ctypes.data, o.ctypes.data, 100, 10)
    assert (ctx.extract_collect(0, 100) == recs[:100]).all() and (ctx.extract_collect_trim(0, 100) == tr[:100]).all()
    with pytest.raises(_native.BadgerHipError):
        ctx.extract_collect_chimera(0, 100)
    ctx.close()


# ---- 3. the command line ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_set(tmp_path_factory):
    from test_trim_gpu import _write_inputs
    tmp = tmp_path_factory.mktemp("chimera_cli")
    R = _read_set(12, 81)
    reads = R["reads"][:1200] + R["reads"][10000:10300] + R["reads"][R["n_real"]::3]
    ids = ["read_%d" % i for i in range(len(reads))]
    bases, off = synth.list_to_reads(reads)
    ctx = _native.Context(0)
    recs = ctx.extract_batch(bases, off, 12)
    tr = ctx.trim_batch(bases, off, recs)
    ctx.close()
    wl = synth.make_whitelist(3000)
    wl = wl[np.random.default_rng(2).permutation(len(wl))]
    wl_path = str(tmp / "wl.txt")
    open(wl_path, "w").write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    return dict(ids=ids, reads=reads, bases=bases, off=off, recs=recs, trim=tr, wl=wl_path, paths=_write_inputs(tmp, ids, reads))


def _expected(S, ch, rows, with_wl):
    fields = [r.split("\t") for r in rows]
    return chimera.fasta_text(S["ids"], S["reads"], S["recs"], S["trim"], ch, rows=fields,
                              wl_barcodes=[f[8] for f in fields] if with_wl else None).encode()


@pytest.mark.parametrize("fmt", ["fa", "fq.gz", "bam"])
@pytest.mark.parametrize("with_wl", [False, True])
def test_cli_end_to_end(cli_set, fmt, with_wl, monkeypatch, caplog, tmp_path):
    S = cli_set
    monkeypatch.setenv("BADGER_AMD_CONTEXTS_ON_ONE_DEVICE", "1")
    monkeypatch.setenv("BADGER_AMD_SEGMENT_MB", "1")
    base = ["--mode", "tenX_v3", "-i", S["paths"][fmt], "-t", "1"] + (["-b", S["wl"]] if with_wl else [])
    plain, plain_fa = str(tmp_path / "plain.tsv"), str(tmp_path / "plain.fa")
    erb.main(base + ["-o", plain, "--trimmed_reads", plain_fa])
    rows = open(plain).read().split("\n")[1:-1]
    assert [r.split("\t")[0] for r in rows] == S["ids"]
    none = np.zeros(len(rows), dtype=chimera.CHIMERA_DTYPE)
    assert open(plain_fa, "rb").read() == _expected(S, none, rows, with_wl)          # --trimmed_reads alone: the file it gives today
    for gpus, ed in (("1", None), ("2", 5)):
        ch = chimera.chimera_batch(S["bases"], S["off"], S["recs"], S["trim"], E if ed is None else ed)
        out, fa = str(tmp_path / ("t%s.tsv" % gpus)), str(tmp_path / ("t%s.fa" % gpus))
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="BarcodeGraph"):
            erb.main(base + ["-o", out, "--gpus", gpus, "--trimmed_reads", fa, "--chimera_cut"] + ([] if ed is None else ["--chimera_max_ed", str(ed)]))
        got = open(fa, "rb").read()
        assert got == _expected(S, ch, rows, with_wl), (fmt, with_wl, gpus)
        assert open(out, "rb").read() == open(plain, "rb").read()
        assert open(out + ".stats", "rb").read() == open(plain + ".stats", "rb").read()
        cut, left_out, nb = chimera.counts(S["trim"], ch)
        line = "Chimeric reads: %d cut, %d left out, %d bases cut off" % (cut, left_out, nb)
        assert any(line in r.getMessage() for r in caplog.records), [r.getMessage() for r in caplog.records][-4:]
        assert cut > 150 and left_out > 0 and got.count(b"\tCH:Z:") == cut


def test_stage1_run_small_chunks_many_contexts(cli_set, tmp_path):
    """bdg_stage1_run directly: chunks of 257 reads over three contexts with the whitelist correction give the same trimmed
    file and counts; the bit without BDG_STAGE1_TRIM is E_ARG; without the bit the trailing fields are not touched"""
    S = cli_set
    wl = erb.load_barcodes(S["wl"])
    ctxs = [_native.Context(0) for _ in range(3)]
    for c in ctxs:
        c.whitelist_load(wl)
    header = "#read_id\tbarcode\tUMI\tBC_score\tvalid_UMI\tstrand\tpolyT_start\tR1_end\twhitelist_barcode\twhitelist_dist\twhitelist_ties"
    kw = dict(threads=3, header_every=1000, chunk_reads=257, format_threads=3, whitelist=True, max_bc_dist=2)
    a, b = str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv")
    ra = _native.stage1_run(ctxs[:1], S["paths"]["fq.gz"], a, header, 12, corrected_path=a + ".corr", trimmed_path=a + ".fa", **kw)
    rb = _native.stage1_run(ctxs, S["paths"]["fq.gz"], b, header, 12, corrected_path=b + ".corr", trimmed_path=b + ".fa", chimera_max_ed=4, **kw)
    assert open(a, "rb").read() == open(b, "rb").read() and open(a + ".corr", "rb").read() == open(b + ".corr", "rb").read()
    rows = [r for r in open(a).read().split("\n")[:-1] if not r.startswith("#")]
    ch = chimera.chimera_batch(S["bases"], S["off"], S["recs"], S["trim"], 4)
    assert open(b + ".fa", "rb").read() == _expected(S, ch, rows, True)
    assert open(a + ".fa", "rb").read() == _expected(S, np.zeros(len(rows), dtype=chimera.CHIMERA_DTYPE), rows, True)
    cut, left_out, nb = chimera.counts(S["trim"], ch)
    assert (rb.chimera_cut, rb.chimera_dropped, rb.chimera_bases) == (cut, left_out, nb)
    assert rb.trimmed_reads == ra.trimmed_reads - left_out and rb.chunks >= len(S["reads"]) // 257
    L = _native.load()
    plain_header = header.split("\twhitelist_barcode")[0]
    arr = (C.c_void_p * 1)(ctxs[0].h)

    def run(o, res, out):
        return L.bdg_stage1_run(arr, 1, os.fsencode(S["paths"]["bam"]), os.fsencode(out), plain_header.encode(),
                                C.cast(C.pointer(o), C.POINTER(_native.Stage1Opts)), C.cast(C.pointer(res), C.POINTER(_native.Stage1Result)))
    res = _native.Stage1ResultChimera()
    d, fa = str(tmp_path / "d.tsv"), os.fsencode(str(tmp_path / "d.fa"))
    # the bit without the trim's
    o = _native.Stage1OptsChimera(12, 1, 0, 0, 300, 0, 0, _native.STAGE1_CHIMERA, 0, 0, 0, 0, None, fa, 20, 0, 3, 0)
    assert run(o, res, d) == _native.E_ARG
    o = _native.Stage1OptsChimera(12, 1, 0, 0, 300, 0, 0, _native.STAGE1_CHIMERA | _native.STAGE1_TRIM, 0, 0, 0, 0, None, fa, 20, 0, 7, 0)
    assert run(o, res, d) == _native.E_ARG
    # the trim's bit alone: chimera_max_ed is not read (999 would be rejected), the three counts are not written
    o = _native.Stage1OptsChimera(12, 1, 0, 0, 300, 0, 0, _native.STAGE1_TRIM, 0, 0, 0, 0, None, fa, 20, 0, 999, 0)
    res.chimera_cut, res.chimera_dropped, res.chimera_bases = 11, 22, 33
    assert run(o, res, d) == 0 and (res.chimera_cut, res.chimera_dropped, res.chimera_bases) == (11, 22, 33)
    rows_d = open(d).read().split("\n")[1:-1]
    assert open(fa, "rb").read() == _expected(S, np.zeros(len(rows_d), dtype=chimera.CHIMERA_DTYPE), rows_d, False)
    assert res.trimmed_reads == ra.trimmed_reads
    for c_ in ctxs:
        c_.close()
