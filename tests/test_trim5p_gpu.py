"""The 5' layout on the GPU: k_layout5p_records against the record rule over the CPU oracle's records on every extraction path,
k_trim_reads_5p against badger_amd/trim5p.py on every field of every generated case, a 3' batch behind a 5' batch on the same
context, and the two command lines end to end against the models."""
import logging

import numpy as np
import pytest

from badger_amd import _native, chimera, common, extract_raw_barcodes as erb, synth, trim, trim5p
from oracle import pyoracle as orc

import fivep_cases as fc

pytestmark = pytest.mark.gpu

FIELDS = ("cdna_start", "cdna_end", "tail_len", "tso_score", "flags")
BATCHES = (1, 63, 64, 65, 257, 4097)


def _same(got, want, what, names=None):
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert not len(bad), (what, f, [names[i] for i in bad[:5]] if names else bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


_MODEL = {}


def _model(umi_len):
    """the read set, the oracle's 3' records of it and the record rule over them: computed once, shared, never changed"""
    if umi_len not in _MODEL:
        S = fc.read_set(umi_len)
        r3 = orc.extract_batch(S["bases"], S["off"], umi_len, threads=8)
        r5 = trim5p.fixup_records(r3, np.diff(S["off"].astype(np.int64)), umi_len)
        r3.setflags(write=False)
        r5.setflags(write=False)
        _MODEL[umi_len] = dict(S, r3=r3, r5=r5)
    return _MODEL[umi_len]


@pytest.fixture()
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


# ---- 1. the record rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("umi_len", [10, 12])
def test_records_extract_batch(ctx, umi_len):
    M = _model(umi_len)
    lens = np.diff(M["off"].astype(np.int64))
    assert lens.min() == 40 and lens.max() == 3000 and (M["r5"]["valid"] == 0).sum() > 50 and (M["r5"]["strand"] == -1).sum() > 1000
    assert ((M["r3"]["polyT"] >= 0) & (M["r3"]["valid"] == 1)).sum() > 100                  # the 3' rule's false polyT columns
    ctx.extract_set_layout(_native.LAYOUT_5P)
    for n in BATCHES:
        got = ctx.extract_batch(M["bases"][:int(M["off"][n])], M["off"][:n + 1], umi_len)
        assert (got == M["r5"][:n]).all(), (n, np.nonzero(got != M["r5"][:n])[0][:5])
    with pytest.raises(_native.BadgerHipError):
        ctx.extract_set_layout(2)
    ctx.extract_set_layout(_native.LAYOUT_3P)
    assert (ctx.extract_batch(M["bases"][:int(M["off"][257])], M["off"][:258], umi_len) == M["r3"][:257]).all()


@pytest.mark.parametrize("umi_len", [10, 12])
def test_records_extract_batch_dev(ctx, umi_len):
    import torch
    M = _model(umi_len)
    dev = torch.device("cuda", 0)
    ctx.set_stream(0)
    ctx.extract_set_layout(_native.LAYOUT_5P)
    for n in BATCHES:
        total = int(M["off"][n])
        d_bases = torch.zeros((total + 15) // 16 * 16 + 64, dtype=torch.uint8, device=dev)
        d_bases[:total] = torch.from_numpy(M["bases"][:total]).to(dev)
        d_off = torch.from_numpy(M["off"][:n + 1].astype(np.int64)).to(dev)
        d_recs = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        for _ in range(8):
            ctx.extract_batch_dev(d_bases, d_off, n, total, umi_len, d_recs)
            rc, _, _ = ctx.extract_status()
            if rc != _native.E_CAPACITY:
                break
        assert rc == 0
        torch.cuda.synchronize()
        assert (d_recs.cpu().numpy().view(_native.REC_DTYPE) == M["r5"][:n]).all(), n


def _pipeline(ctx, bases, off, n, step, umi_len, with_trim=False):
    recs, trims, flying = [], [], []

    def collect():
        slot, a, b, _ = flying.pop(0)
        recs.append(ctx.extract_collect(slot, b - a))
        if with_trim:
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
    return np.concatenate(recs), (np.concatenate(trims) if with_trim else None)


@pytest.mark.parametrize("umi_len", [10, 12])
def test_records_and_trim_submit_collect_with_forced_rerun(ctx, umi_len):
    M = _model(umi_len)
    n = 4097
    want_trim = trim5p.trim_batch(M["bases"], M["off"], M["r5"], umi_len)
    assert ((want_trim["flags"] & trim.TRIM_EMIT) != 0).sum() > 2000 and (want_trim["flags"] == trim5p.TRIM_NO_ANCHOR).sum() > 20
    ctx.extract_set_layout(_native.LAYOUT_5P)
    ctx.trim_set_5p(umi_len, trim5p.TSO5_MAX_ED_DEFAULT)
    ctx.extract_set_trim(True, trim5p.MIN_SCORE_DEFAULT)
    for step in (257, 1500):
        got, got_trim = _pipeline(ctx, M["bases"], M["off"], n, step, umi_len, True)
        assert (got == M["r5"]).all(), step
        _same(got_trim, want_trim, "pipelined trim, chunks of %d" % step)
    # a queue far too small: every chunk overflows and collect runs it again, in the layout it was submitted with - even when
    # the context has been put back in between
    ctx.extract_set_queue_capacity(16)
    recs, trims, held = [], [], []
    for k, a in enumerate(range(0, n, 1100)):
        b = min(a + 1100, n)
        o = np.ascontiguousarray(M["off"][a:b + 1], dtype=np.uint64)
        held.append(o)
        ctx.extract_submit(k, M["bases"].ctypes.data, o.ctypes.data, b - a, umi_len)
    ctx.extract_set_layout(_native.LAYOUT_3P)
    for k, a in enumerate(range(0, n, 1100)):
        b = min(a + 1100, n)
        recs.append(ctx.extract_collect(k, b - a))
        trims.append(ctx.extract_collect_trim(k, b - a))
    ctx.extract_set_queue_capacity(0)
    got = np.concatenate(recs)
    assert not (got["flags"] & _native.FLAG_INCOMPLETE).any() and (got == M["r5"]).all()
    _same(np.concatenate(trims), want_trim, "pipelined trim after the rerun")
    ctx.extract_set_trim(False)


# ---- 2. the trimming rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("umi_len,max_ed,score", [(10, 2, 16), (12, 2, 16), (12, 0, 8), (10, 4, 25), (12, 1, 20), (10, 3, 12)])
def test_trim_cases_equal_the_rule(ctx, umi_len, max_ed, score):
    S = fc.trim_cases(umi_len, max_ed)
    want = trim5p.trim_batch(S["bases"], S["off"], S["recs"], umi_len, max_ed, score)
    ctx.extract_set_layout(_native.LAYOUT_5P)
    ctx.trim_set_5p(umi_len, max_ed)
    got = ctx.trim_batch(S["bases"], S["off"], S["recs"], score)
    _same(got, want, "trim cases", S["names"])
    assert len(S["reads"]) > 256 and ((want["flags"] & trim.TRIM_EMIT) != 0).sum() > 100
    for bad in (7, 26):
        with pytest.raises(_native.BadgerHipError):
            ctx.trim_batch(S["bases"], S["off"], S["recs"], bad)
    with pytest.raises(_native.BadgerHipError):
        ctx.trim_set_5p(umi_len, 5)


def test_trim_batch_on_the_read_set_and_dev_form(ctx):
    import torch
    M = _model(12)
    n, total = 4097, int(M["off"][4097])
    want = trim5p.trim_batch(M["bases"], M["off"], M["r5"], 12, 2, 16)
    ctx.extract_set_layout(_native.LAYOUT_5P)
    ctx.trim_set_5p(12, 2)
    _same(ctx.trim_batch(M["bases"], M["off"], M["r5"], 16), want, "read set")
    pick = np.random.default_rng(1).choice(n, 300, replace=False)
    _same(want[pick], trim5p.trim_reads([M["reads"][i] for i in pick], M["r5"][pick], 12, 2, 16), "one-read form")
    dev = torch.device("cuda", 0)
    ctx.set_stream(0)
    d_bases = torch.zeros((total + 15) // 16 * 16 + 64, dtype=torch.uint8, device=dev)
    d_bases[:total] = torch.from_numpy(M["bases"][:total]).to(dev)
    d_off = torch.from_numpy(M["off"].astype(np.int64)).to(dev)
    d_recs = torch.from_numpy(np.ascontiguousarray(M["r5"]).view(np.uint8).copy()).to(dev)
    d_out = torch.full((n * 12,), 0xAB, dtype=torch.uint8, device=dev)
    ctx.trim_batch_dev(d_bases, d_off, n, d_recs, 16, d_out)
    torch.cuda.synchronize()
    _same(d_out.cpu().numpy().view(_native.TRIM_DTYPE), want, "device form")


# ---- 3. no state leaks into the 3' layout ---------------------------------------------------------------------------------
def test_3p_batch_behind_a_5p_batch(ctx):
    M = _model(12)
    n = 1200
    bases, off = M["bases"][:int(M["off"][n])], M["off"][:n + 1]
    wl = synth.make_whitelist(300)
    b3, o3 = synth.make_reads(n, wl, seed=5, umi_len=12, tso=True)
    b3, o3 = b3.numpy(), o3.numpy().astype(np.uint64)
    want3 = orc.extract_batch(b3, o3, 12, threads=8)
    ctx.extract_set_layout(_native.LAYOUT_5P)
    ctx.trim_set_5p(12, 2)
    r5 = ctx.extract_batch(bases, off, 12)
    assert (r5 == M["r5"][:n]).all()
    ctx.trim_batch(bases, off, r5, 16)
    ctx.extract_set_layout(_native.LAYOUT_3P)
    got3 = ctx.extract_batch(b3, o3, 12)
    assert (got3 == want3).all() and (got3["polyT"] >= 0).sum() > 1000
    _same(ctx.trim_batch(b3, o3, got3, 20), trim.trim_batch(b3, o3, got3, 20), "3' trim behind a 5' batch")
    _same(ctx.trim_batch(b3, o3, got3, 30), trim.trim_batch(b3, o3, got3, 30), "3' trim, score 30 again in range")


# ---- 4. the command lines ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_set(tmp_path_factory):
    """about 2,000 reads of the read set (UMI 10), every fourth with another molecule ligated into its cDNA (an R1 junction)"""
    tmp = tmp_path_factory.mktemp("trim5p_cli")
    S = fc.read_set(10)
    rng = np.random.default_rng(8)
    reads = list(S["reads"][:2000])
    for i in range(0, 2000, 4):
        y = S["reads"][2000 + i // 4]
        if len(reads[i]) > 300 and len(y) > 150:
            cut = int(rng.integers(150, len(reads[i]) - 100))
            reads[i] = (reads[i][:cut] + y[:150] + reads[i][cut:])[:3000]
    ids = ["read_%d" % i for i in range(len(reads))]
    bases, off = synth.list_to_reads(reads)
    r5 = trim5p.fixup_records(orc.extract_batch(bases, off, 10, threads=8), np.diff(off.astype(np.int64)), 10)
    fq = str(tmp / "reads.fastq")
    with open(fq, "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in zip(ids, reads)))
    wl_path = str(tmp / "wl.txt")
    open(wl_path, "w").write("".join(common.unrank(int(r), 16) + "\n" for r in S["wl"]))
    return dict(tmp=tmp, ids=ids, reads=reads, bases=bases, off=off, r5=r5, fq=fq, wl=wl_path)


def test_stage1_cli(cli_set, caplog):
    from test_trim import _Chunk
    S = cli_set
    tmp, n = S["tmp"], len(S["reads"])
    ck = _Chunk(S["ids"], S["reads"])
    rows_text, counts = _native.format_rows(ck.ch, S["r5"])
    header = erb.BARCODE_CALLING_MODES["tenX_5p_v2"].result_type().header()
    rows = rows_text.decode().split("\n")[:-1]
    out, fa, fa_cut = str(tmp / "s1.tsv"), str(tmp / "s1.fa"), str(tmp / "s1_cut.fa")
    with caplog.at_level(logging.INFO, logger="BarcodeGraph"):
        erb.main(["--mode", "tenX_5p_v2", "-i", S["fq"], "-o", out, "-t", "1", "--trimmed_reads", fa])
    assert open(out).read() == header + "\n" + rows_text.decode()
    valid = int((S["r5"]["valid"] == 1).sum())
    r1 = int(((S["r5"]["valid"] == 1) & (S["r5"]["r1_end"] != -1)).sum())
    assert open(out + ".stats").read() == "Total reads:\t%d\nBarcode detected:\t%d\nReliable UMI:\t0\nR1 detected:\t%d\n" % (n, valid, r1)
    assert valid > 1500 and all(r.split("\t")[6] == "-1" for r in rows) and {r.split("\t")[5] for r in rows} == {"+", "-", "."}
    tr = trim5p.trim_batch(S["bases"], S["off"], S["r5"], 10)
    assert open(fa).read() == trim.fasta_text(S["ids"], S["reads"], S["r5"], tr, rows=[r.split("\t") for r in rows])
    emit = (tr["flags"] & trim.TRIM_EMIT) != 0
    line = "Trimmed reads: %d written to %s, %d with the RT primer cut off, %d bases, %d left out without the switch oligo" % (
        int(emit.sum()), fa, int((emit & ((tr["flags"] & trim.TRIM_TSO) != 0)).sum()),
        int((tr["cdna_end"][emit] - tr["cdna_start"][emit]).sum()), int((tr["flags"] == trim5p.TRIM_NO_ANCHOR).sum()))
    assert any(line in r.getMessage() for r in caplog.records), [r.getMessage() for r in caplog.records][-4:]
    assert emit.sum() > 1500 and (tr["flags"] == trim5p.TRIM_NO_ANCHOR).sum() > 5
    # --chimera_cut over the 5' spans, other values of the two bounds, two contexts and several reader threads
    tr2 = trim5p.trim_batch(S["bases"], S["off"], S["r5"], 10, 3, 12)
    chim = chimera.chimera_batch(S["bases"], S["off"], S["r5"], tr2, 2)
    import os
    os.environ["BADGER_AMD_CONTEXTS_ON_ONE_DEVICE"] = "1"
    try:
        erb.main(["--mode", "tenX_5p_v2", "-i", S["fq"], "-o", str(tmp / "s1c.tsv"), "-t", "3", "--gpus", "2", "--trimmed_reads", fa_cut,
                  "--tso5_max_ed", "3", "--tso_min_score", "12", "--chimera_cut", "--chimera_max_ed", "2"])
    finally:
        del os.environ["BADGER_AMD_CONTEXTS_ON_ONE_DEVICE"]
    assert open(fa_cut).read() == chimera.fasta_text(S["ids"], S["reads"], S["r5"], tr2, chim, rows=[r.split("\t") for r in rows])
    assert chimera.counts(tr2, chim)[0] > 200
    # the shared context is back in the 3' layout
    assert (_native.default_context(0).extract_batch(S["bases"][:int(S["off"][50])], S["off"][:51], 10)["polyT"] >= 0).any()


def test_stage2_tagged_reads(cli_set):
    from test_tagged_reads_gpu import _expected, _stage2
    S = cli_set
    tmp = S["tmp"]
    fasta = {}
    for cut in (False, True):
        fasta[cut] = str(tmp / ("st1_%d.fa" % cut))
        erb.main(["--mode", "tenX_5p_v2", "-i", S["fq"], "-o", str(tmp / ("st1_%d.tsv" % cut)), "-t", "1", "--trimmed_reads", fasta[cut]]
                 + (["--chimera_cut"] if cut else []))
    T = dict(ids=S["ids"], fasta=fasta)
    base = ["-r", S["fq"], "-d", "tenX_5p_v2", "-l", S["wl"], "-c", "40"]
    prefix = str(tmp / "st2")
    _stage2(base + ["-o", prefix, "--tagged_reads", prefix + ".fa", "--umi_dedup"])
    want, lengths, counts = _expected(T, prefix, False, True, False)
    got = open(prefix + ".fa", "rb").read()
    assert got == want and counts[0] > 300 and got.count(b"\tUB:Z:") > 300
    prefix = str(tmp / "st2m")
    _stage2(base + ["-o", prefix, "--tagged_reads", prefix + ".fa", "--umi_dedup", "--molecule_reads", "--chimera_cut"])
    want, lengths, counts = _expected(T, prefix, True, True, True)
    got = open(prefix + ".fa", "rb").read()
    assert got == want and counts[0] > 300 and got.count(b"\tCH:Z:") > 10
    # the UMIs stage 2 deduplicates are the fixed-length ones
    mol = [l.split("\t") for l in open(prefix + "_molecules.tsv").read().split("\n")[1:-1]]
    lens = [len(f[2]) for f in mol if f[2] != "*"]
    assert max(lens) == 10 and lens.count(10) > 0.97 * len(lens) > 300        # (shorter: a read that ends inside its UMI)
