"""--tagged_reads on the GPU: stage 2's tagged file equals what the existing outputs say when joined by read id - the records
of stage 1's --trimmed_reads [--chimera_cut] FASTA on the same input, the cells of <out>_output_file.tsv, the molecules of
<out>_molecules.tsv - and, with --molecule_reads, filtered by the rule of badger_amd/molecule_reads.py over those files.  About
3,000 synthetic reads of a few dozen cells with planted chimeras and verbatim copies under new ids, so that molecules hold several
reads and share their longest cDNA.  Nothing stage 2 wrote before moves."""
import io
import logging
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

from badger_amd import badger, common, extract_raw_barcodes as erb, molecule_reads as mr, synth, trim
from badger_amd.umi_dedup import umi_code

pytestmark = pytest.mark.gpu

N_CELLS = 48


def _stage2(argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        badger.main(argv)
    return buf.getvalue()


def _build(tmp, umi_len, seed):
    """reads.fastq, the whitelist file, and stage 1's trimmed FASTA with and without --chimera_cut"""
    wl = synth.make_whitelist(400)
    b, o = synth.make_reads(1500, wl, seed=seed, umi_len=umi_len, n_cells=N_CELLS, tso=True)
    base = synth.reads_to_list(b, o)
    rng = np.random.default_rng(seed)
    reads = list(base)
    for i in rng.choice(1500, size=700, replace=False).tolist():      # verbatim copies: the same molecule, the same cDNA length
        reads.append(base[i])
        if i % 3 == 0:
            reads.append(base[i])
    for k in range(500):                                              # chimeras: a read of the set joined with another one
        x, y = base[int(rng.integers(0, 1500))], base[int(rng.integers(0, 1500))]
        reads.append(x + (y if k & 1 else trim.revcomp(y)) if k & 2 else (trim.revcomp(y) if k & 1 else y) + x)
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    ids = ["read_%d" % i for i in range(len(reads))]
    fq = str(tmp / "reads.fastq")
    with open(fq, "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in zip(ids, reads)))
    wl_path = str(tmp / "wl.txt")
    open(wl_path, "w").write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    mode = "tenX_v3" if umi_len == 12 else "tenX_v2"
    fasta = {}
    for cut in (False, True):
        fa = str(tmp / ("stage1_%d.fa" % cut))
        erb.main(["--mode", mode, "-i", fq, "-o", str(tmp / ("stage1_%d.tsv" % cut)), "-t", "1", "--trimmed_reads", fa] + (["--chimera_cut"] if cut else []))
        fasta[cut] = fa
    return dict(tmp=tmp, fq=fq, wl=wl_path, ids=ids, fasta=fasta, mode=mode,
                base=["-r", fq, "-d", mode, "-l", wl_path, "-c", str(N_CELLS)])


@pytest.fixture(scope="module")
def v3(tmp_path_factory):
    S = _build(tmp_path_factory.mktemp("tagged"), 12, 7)
    # the three outputs stage 2 has without the new flags
    S["plain"] = {}
    for dedup in (False, True):
        prefix = str(S["tmp"] / ("plain_%d" % dedup))
        out = _stage2(S["base"] + ["-o", prefix] + (["--umi_dedup"] if dedup else []))
        S["plain"][dedup] = (prefix, out.strip().split("\n")[-1])
    return S


def _records(fa):
    """stage 1's FASTA -> {read id: (header fields behind the id, sequence)} and the ids in file order"""
    lines = open(fa).read().split("\n")[:-1]
    out, order = {}, []
    for h, s in zip(lines[::2], lines[1::2]):
        f = h[1:].split("\t")
        out[f[0]] = (f[1:], s)
        order.append(f[0])
    return out, order


def _expected(S, prefix, cut, dedup, molecule_reads):
    """the tagged file from the existing outputs alone -> (bytes, per-molecule lists of cDNA lengths, counts)"""
    recs, order = _records(S["fasta"][cut])
    cell = dict(l.split("\t") for l in open(prefix + "_output_file.tsv").read().split("\n")[1:-1])
    ids = S["ids"]
    assert list(cell) == ids
    mol, size = {}, {}
    if dedup:
        for l in open(prefix + "_molecules.tsv").read().split("\n")[1:-1]:
            rid, bc, _, m = l.split("\t")
            assert bc == cell[rid]
            if m != "*":
                mol[rid] = m
                size[(bc, m)] = size.get((bc, m), 0) + 1
    keep = None
    lengths = {}
    if dedup:
        has = np.array([cell[r] != "*" for r in ids], dtype=np.uint8)
        rank = np.array([common.rank(cell[r], 16) if cell[r] != "*" else 0 for r in ids], dtype=np.uint32)
        code = np.array([umi_code(mol[r]) if r in mol else mr.NONE for r in ids], dtype=np.uint32)
        length = np.array([len(recs[r][1]) if r in recs else 0 for r in ids], dtype=np.uint32)
        rep, cnt = mr.molecule_reps(rank, has, code, length, np.unique(rank[has != 0]))
        assert all(int(cnt[i]) == size.get((cell[r], mol.get(r)), 0) for i, r in enumerate(ids))
        for i, r in enumerate(ids):
            if r in mol and length[i]:
                lengths.setdefault((cell[r], mol[r]), []).append(int(length[i]))
        if molecule_reads:
            keep = {r for i, r in enumerate(ids) if rep[i]}
    out, counts = [], [0, 0, 0, 0]
    for rid in order:
        fields, seq = recs[rid]
        if cell[rid] == "*":
            counts[2] += 1
            continue
        if keep is not None and rid not in keep:
            counts[3] += 1
            continue
        ch = [f for f in fields if f.startswith("CH:Z:")]
        assert [f[:5] for f in fields] == ["CR:Z:", "UR:Z:", "ST:A:"] + ["CH:Z:"] * len(ch)
        tags = ["CB:Z:" + cell[rid]] + (["UB:Z:" + mol[rid], "RN:i:%d" % size[(cell[rid], mol[rid])]] if rid in mol else [])
        out.append(">" + "\t".join([rid] + fields[:3] + tags + ch) + "\n" + seq + "\n")
        counts[0] += 1
        counts[1] += len(seq)
    return "".join(out).encode(), lengths, counts


def _unchanged(S, prefix, dedup, stdout):
    plain, last = S["plain"][dedup]
    for suffix in ("_output_file.tsv",) + (("_molecules.tsv", "_cells.tsv") if dedup else ()):
        assert open(prefix + suffix, "rb").read() == open(plain + suffix, "rb").read(), suffix
    assert stdout.strip().split("\n")[-1] == last


@pytest.mark.parametrize("dedup", (False, True))
@pytest.mark.parametrize("cut", (False, True))
def test_tagged_file_is_the_join_of_the_existing_outputs(v3, cut, dedup, caplog):
    S = v3
    prefix = str(S["tmp"] / ("t_%d_%d" % (cut, dedup)))
    fa = prefix + ".fa"
    flags = (["--chimera_cut"] if cut else []) + (["--umi_dedup"] if dedup else [])
    with caplog.at_level(logging.INFO, logger="BarcodeGraph"):
        out = _stage2(S["base"] + ["-o", prefix, "--tagged_reads", fa] + flags)
    want, lengths, counts = _expected(S, prefix, cut, dedup, False)
    got = open(fa, "rb").read()
    assert got == want, (cut, dedup)
    _unchanged(S, prefix, dedup, out)
    line = "Tagged reads: %d to %s, %d bases; left out: %d without a cell, %d not their molecule's read" % (counts[0], fa, counts[1], counts[2], 0)
    assert any(line in r.getMessage() for r in caplog.records), [r.getMessage() for r in caplog.records][-3:]
    assert counts[0] > 1000 and counts[2] > 20 and got.count(b"\tCB:Z:") == counts[0]
    assert (got.count(b"\tCH:Z:") > 50) == cut and (got.count(b"\tUB:Z:") > 500) == dedup and got.count(b"\tUB:Z:") == got.count(b"\tRN:i:")
    if dedup:
        # the input holds what it is for: molecules of several reads with cDNA, and molecules that share their longest one
        several = [v for v in lengths.values() if len(v) >= 2]
        assert len(several) >= 100 and sum(1 for v in several if v.count(max(v)) >= 2) >= 10
        assert sum(1 for v in several if v.count(max(v)) == 1) >= 10
        # one read per molecule
        caplog.clear()
        fa1 = prefix + ".mol.fa"
        with caplog.at_level(logging.INFO, logger="BarcodeGraph"):
            out = _stage2(S["base"] + ["-o", prefix + "_m", "--tagged_reads", fa1, "--molecule_reads"] + flags)
        want1, _, counts1 = _expected(S, prefix + "_m", cut, True, True)
        got1 = open(fa1, "rb").read()
        assert got1 == want1
        _unchanged(S, prefix + "_m", True, out)
        assert counts1[3] > 100 and counts1[0] + counts1[3] == counts[0] and counts1[2] == counts[2]
        line = "left out: %d without a cell, %d not their molecule's read" % (counts1[2], counts1[3])
        assert any(line in r.getMessage() for r in caplog.records)
        # every molecule with cDNA once, and nothing else (a read with a cell and no molecule is nobody's representative)
        heads = [l for l in got1.decode().split("\n") if l.startswith(">")]
        keys = [tuple(f[5:] for f in h.split("\t") if f[:5] in ("CB:Z:", "UB:Z:")) for h in heads]
        assert len(keys) == len(set(keys)) == len(lengths) and all(len(k) == 2 for k in keys)


def test_reader_threads_give_the_same_file(v3):
    S = v3
    outs = []
    for tr in ("1", "4"):
        prefix = str(S["tmp"] / ("tr%s" % tr))
        _stage2(S["base"] + ["-o", prefix, "-tr", tr, "--tagged_reads", prefix + ".fa", "--chimera_cut", "--umi_dedup", "--molecule_reads"])
        outs.append(open(prefix + ".fa", "rb").read())
    assert outs[0] == outs[1] and len(outs[0]) > 100000


def test_tenx_v2(tmp_path):
    S = _build(tmp_path, 10, 9)
    prefix = str(tmp_path / "v2")
    _stage2(S["base"] + ["-o", prefix, "--tagged_reads", prefix + ".fa", "--chimera_cut", "--umi_dedup"])
    want, lengths, counts = _expected(S, prefix, True, True, False)
    assert open(prefix + ".fa", "rb").read() == want and counts[0] > 1000 and len(lengths) > 300


def test_read_count_mismatch_is_an_error(v3, tmp_path):
    """bdg_stage1_run with BDG_STAGE1_TAGS: tag arrays shorter or longer than the input fail with E_ARG and say why"""
    from badger_amd import _native
    S = v3
    n = len(S["ids"])
    ctx = _native.Context(0)
    try:
        for m in (n - 1, n + 1, 10):
            tags = dict(cell_rank=np.zeros(m, np.uint32), cell_has=np.ones(m, np.uint8))
            with pytest.raises(_native.BadgerHipError) as e:
                _native.stage1_run([ctx], S["fq"], None, "", 12, threads=1, trimmed_path=str(tmp_path / "x.fa"), tags=tags)
            assert e.value.code == _native.E_ARG and "reads" in str(e.value) and str(m) in str(e.value)
        tags = dict(cell_rank=np.zeros(n, np.uint32), cell_has=np.ones(n, np.uint8))
        with pytest.raises(_native.BadgerHipError):                  # the bit without the trim's
            _native.stage1_run([ctx], S["fq"], None, "", 12, threads=1, tags=tags)
        res = _native.stage1_run([ctx], S["fq"], None, "", 12, threads=1, trimmed_path=str(tmp_path / "y.fa"), tags=tags)
        assert res.reads == n and res.tags_no_cell == 0 and res.trimmed_reads == open(str(tmp_path / "y.fa"), "rb").read().count(b">") > 1500
    finally:
        ctx.close()
