"""--chimera_split end to end: equivalence with a pre-split file.  A FASTQ of synthetic reads, some of them planted two- and
three-molecule chimeras, and a second FASTQ in which the checker's pieces (badger_amd/chimera_split.py) stand as reads of their
own under the suffixed ids: every command with the flag on the first file must write the bytes it writes without the flag on
the second."""
import ctypes as C
import io
import logging
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

from badger_amd import _native, badger, chimera_split as cs, common, extract_raw_barcodes as erb, synth
from badger_amd.trim import revcomp

pytestmark = pytest.mark.gpu

N_CELLS = 40
E = cs.MAX_ED_DEFAULT


def _fastq(path, ids, reads):
    with open(path, "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in zip(ids, reads)))


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("split_cli")
    wl = synth.make_whitelist(400)
    b, o = synth.make_reads(460, wl, seed=31, n_cells=N_CELLS, tso=True)
    base = synth.reads_to_list(b, o)
    rng = np.random.default_rng(31)
    reads = list(base[:340])
    for k in range(60):                                                 # chimeras of two and of three reads, either strand
        parts = [base[340 + 2 * k], base[341 + 2 * k]] + ([base[int(rng.integers(0, 340))]] if k % 3 == 0 else [])
        reads.append("".join(revcomp(x) if rng.integers(0, 2) else x for x in parts))
    reads = [reads[i] for i in rng.permutation(len(reads))]
    ids = ["read_%d%s" % (i, " ch=%d start=x" % i if i % 7 == 0 else "") for i in range(len(reads))]
    bases, off = synth.list_to_reads(reads)
    off_out, rows = cs.split_batch(bases, off, E)
    text = bases.tobytes().decode()
    pieces = [text[int(a):int(z)] for a, z in zip(off_out[:-1], off_out[1:])]
    n_cut, n_pieces = cs.counts(rows, len(reads))
    assert 50 <= n_cut <= 64 and n_pieces >= 2 * n_cut + 15
    clean = [r for r, c in zip(reads, np.bincount(rows["read"])) if c == 1]
    paths = dict(a=str(tmp / "reads.fastq"), b=str(tmp / "pieces.fastq"), clean=str(tmp / "clean.fastq"), wl=str(tmp / "wl.txt"))
    _fastq(paths["a"], ids, reads)
    _fastq(paths["b"], cs.piece_ids(ids, rows), pieces)
    _fastq(paths["clean"], ["c%d" % i for i in range(len(clean))], clean)
    open(paths["wl"], "w").write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    return dict(tmp=tmp, paths=paths, reads=reads, ids=ids, rows=rows, counts=(n_cut, n_pieces), n_pieces=len(rows))


def _same_files(da, db):
    names = sorted(os.listdir(da))
    assert names == sorted(os.listdir(db)) and names
    for n in names:
        assert open(os.path.join(da, n), "rb").read() == open(os.path.join(db, n), "rb").read(), n
    return names


VARIANTS = {
    "plain": [],
    "trim": ["--trimmed_reads", "{d}/t.fa"],
    "trim_cut": ["--trimmed_reads", "{d}/t.fa", "--chimera_cut"],
    "rescue": ["-b", "{wl}", "--bc_correct", "--bc_rescue", "--trimmed_reads", "{d}/t.fa"],
}


@pytest.mark.parametrize("threads,gpus", [("1", "1"), ("4", "1"), ("4", "2")])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_stage1_cli_equals_the_presplit_file(S, variant, threads, gpus, tmp_path, monkeypatch, caplog):
    """the command line as users run it, in its one-thread and its parallel file shape and with two contexts opened.  (The command
    line has no option for the chunk size and these files are one chunk of its 100,000 reads: many chunks over many contexts, with
    the correction and the rescue, are test_many_chunks_many_contexts_with_correction_and_rescue's, through bdg_stage1_run)"""
    monkeypatch.setenv("BADGER_AMD_CONTEXTS_ON_ONE_DEVICE", "1")
    dirs = {}
    for which, extra in (("a", ["--chimera_split"]), ("b", [])):
        d = tmp_path / which
        d.mkdir()
        args = [x.format(d=d, wl=S["paths"]["wl"]) for x in VARIANTS[variant]]
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="BarcodeGraph"):
            erb.main(["--mode", "tenX_v3", "-i", S["paths"][which], "-o", str(d / "o.tsv"), "-t", threads, "--gpus", gpus] + args + extra)
        if which == "a":
            line = "Split reads: %d reads cut into %d pieces" % S["counts"]
            assert any(line in r.getMessage() for r in caplog.records), [r.getMessage() for r in caplog.records][-4:]
        dirs[which] = str(d)
    names = _same_files(dirs["a"], dirs["b"])
    assert "o.tsv.stats" in names and ("t.fa" in names) == (variant != "plain")
    rows = [r for r in open(os.path.join(dirs["a"], "o.tsv")).read().split("\n")[:-1] if not r.startswith("#")]
    assert len(rows) == S["n_pieces"] and sum("/2" in r.split("\t")[0] for r in rows) == S["counts"][0]


def test_stage1_run_small_chunks_and_the_bit_alone(S, tmp_path):
    """bdg_stage1_run directly: chunks of 37 reads over three contexts (a chimera's pieces straddle nothing: chunk borders fall
    between reads) and --split_max_ed; without the bit the trailing fields are neither read nor written"""
    header = "#read_id\tbarcode\tUMI\tBC_score\tvalid_UMI\tstrand\tpolyT_start\tR1_end"
    ctxs = [_native.Context(0) for _ in range(3)]
    kw = dict(threads=3, header_every=100, chunk_reads=37, format_threads=3)
    for ed in (E, 1):
        bases, off = synth.list_to_reads(S["reads"])
        off_out, rows = cs.split_batch(bases, off, ed)
        text = bases.tobytes().decode()
        b_fq = str(tmp_path / ("b%d.fastq" % ed))
        _fastq(b_fq, cs.piece_ids(S["ids"], rows), [text[int(a):int(z)] for a, z in zip(off_out[:-1], off_out[1:])])
        a, b = str(tmp_path / ("a%d.tsv" % ed)), str(tmp_path / ("b%d.tsv" % ed))
        ra = _native.stage1_run(ctxs, S["paths"]["a"], a, header, 12, trimmed_path=a + ".fa", split_max_ed=ed, **kw)
        rb = _native.stage1_run(ctxs[:1], b_fq, b, header, 12, trimmed_path=b + ".fa", **kw)
        assert open(a, "rb").read() == open(b, "rb").read() and open(a + ".fa", "rb").read() == open(b + ".fa", "rb").read()
        assert (ra.split_reads, ra.split_pieces) == cs.counts(rows, len(S["reads"])) and ra.reads == rb.reads == len(rows)
        assert ra.chunks >= len(S["reads"]) // 37 and ra.trimmed_reads == rb.trimmed_reads
    # the bit off: split_max_ed is not read (99 would be rejected), the two counts are not written
    L = _native.load()
    arr = (C.c_void_p * 1)(ctxs[0].h)
    o = _native.Stage1OptsSplit(12, 1, 0, 0, 300)
    o.split_max_ed = 99
    res = _native.Stage1ResultSplit()
    res.split_reads, res.split_pieces = 11, 22
    run = lambda: L.bdg_stage1_run(arr, 1, os.fsencode(S["paths"]["a"]), os.fsencode(str(tmp_path / "c.tsv")), header.encode(),   # noqa: E731
                                   C.cast(C.pointer(o), C.POINTER(_native.Stage1Opts)), C.cast(C.pointer(res), C.POINTER(_native.Stage1Result)))
    assert run() == 0 and (res.split_reads, res.split_pieces, res.reads) == (11, 22, len(S["reads"]))
    o.whitelist = _native.STAGE1_SPLIT
    assert run() == _native.E_ARG and "split max_ed" in L.bdg_last_error(ctxs[0].h).decode()
    o.split_max_ed = E
    assert run() == 0 and (res.split_reads, res.split_pieces, res.reads) == S["counts"] + (S["n_pieces"],)
    ctxs[0].extract_set_layout(_native.LAYOUT_5P)                        # the 5' layout: an error with a message
    assert run() == _native.E_ARG and "3'" in L.bdg_last_error(ctxs[0].h).decode()
    ctxs[0].extract_set_layout(_native.LAYOUT_3P)
    for c in ctxs:
        c.close()


WL_HEADER = "#read_id\tbarcode\tUMI\tBC_score\tvalid_UMI\tstrand\tpolyT_start\tR1_end\twhitelist_barcode\twhitelist_dist\twhitelist_ties"


def _presplit(tmp_path, name, ids, reads, max_ed=E):
    """the two inputs of an equivalence: the reads, and the checker's pieces as reads -> paths a, b, the piece records"""
    bases, off = synth.list_to_reads(reads)
    off_out, rows = cs.split_batch(bases, off, max_ed)
    text = bases.tobytes().decode()
    a, b = str(tmp_path / (name + "_a.fastq")), str(tmp_path / (name + "_b.fastq"))
    _fastq(a, ids, reads)
    _fastq(b, cs.piece_ids(ids, rows), [text[int(x):int(z)] for x, z in zip(off_out[:-1], off_out[1:])])
    return a, b, rows


def test_many_chunks_many_contexts_with_correction_and_rescue(S, tmp_path):
    """bdg_stage1_run with the whitelist match, the correction, the rescue and the trimmed file, chunks of 37 reads over three
    contexts: the rescue store's ordinals, the kept candidate lists, the map from chunks to contexts in the correction's and the
    rescue's last step and the id store all count pieces over many chunks.  Some reads have lost their adapter (both ends cut
    off), so that the rescue has work."""
    bare = [r[45:-45] for r, c in zip(S["reads"], np.bincount(S["rows"]["read"])) if c == 1 and len(r) > 400][:90]
    rng = np.random.default_rng(5)
    reads = S["reads"] + bare
    reads = [reads[i] for i in rng.permutation(len(reads))]
    ids = ["m%d" % i for i in range(len(reads))]
    a_fq, b_fq, rows = _presplit(tmp_path, "many", ids, reads)
    assert cs.counts(rows, len(reads))[0] >= 50
    wl = erb.load_barcodes(S["paths"]["wl"])
    ctxs = [_native.Context(0) for _ in range(3)]
    for c in ctxs:
        c.whitelist_load(wl)
    res = {}
    for which, fq, n_ctx, extra in (("a", a_fq, 3, dict(split_max_ed=E)), ("b", b_fq, 2, {})):
        out = str(tmp_path / (which + ".tsv"))
        res[which] = _native.stage1_run(ctxs[:n_ctx], fq, out, WL_HEADER, 12, threads=3, header_every=100, chunk_reads=37, format_threads=3,
                                        whitelist=True, max_bc_dist=2, corrected_path=out + ".corr", rescued_path=out + ".resc",
                                        trimmed_path=out + ".fa", **extra)
    for suffix in ("", ".corr", ".resc", ".fa"):
        assert open(str(tmp_path / "a.tsv") + suffix, "rb").read() == open(str(tmp_path / "b.tsv") + suffix, "rb").read(), suffix
    ra, rb = res["a"], res["b"]
    for f in ("reads", "barcodes", "whitelist_barcodes", "whitelist_corrected", "trimmed_reads", "trimmed_bases", "rescue_eligible", "rescue_rescued",
              "rescue_ambiguous", "rescue_truncated"):
        assert getattr(ra, f) == getattr(rb, f), f
    assert ra.reads == len(rows) and ra.chunks >= len(reads) // 37 and (ra.split_reads, ra.split_pieces) == cs.counts(rows, len(reads))
    assert ra.whitelist_corrected > 200 and ra.rescue_eligible >= 50 and ra.rescue_rescued > 0
    for c in ctxs:
        c.close()


def test_a_chunk_of_concatemers_only(tmp_path):
    """one chunk whose boundaries outnumber what the submit fetches with the count (n / 8 + 1024): the rest of the piece records
    is fetched before the chunk's kernels are queued"""
    import split_cases as sc
    rng = np.random.default_rng(12)
    mols = [sc.molecule(rng) for _ in range(40)]
    reads = ["".join(revcomp(mols[i]) if flip else mols[i] for i, flip in zip(rng.integers(0, 40, size=6), rng.integers(0, 2, size=6)))
             for _ in range(300)]
    a_fq, b_fq, rows = _presplit(tmp_path, "conc", ["c%d" % i for i in range(300)], reads)
    assert len(rows) - 300 > 300 // 8 + 1024 and (np.bincount(rows["read"]) == 6).all()
    header = WL_HEADER.split("\twhitelist_barcode")[0]
    ctx = _native.Context(0)
    ra = _native.stage1_run([ctx], a_fq, str(tmp_path / "a.tsv"), header, 12, threads=1, trimmed_path=str(tmp_path / "a.fa"), split_max_ed=E)
    rb = _native.stage1_run([ctx], b_fq, str(tmp_path / "b.tsv"), header, 12, threads=1, trimmed_path=str(tmp_path / "b.fa"))
    ctx.close()
    assert ra.chunks == 1 and (ra.split_reads, ra.split_pieces, ra.reads) == (300, 1800, 1800) and rb.reads == 1800
    for name in ("tsv", "fa"):
        assert open(str(tmp_path / ("a." + name)), "rb").read() == open(str(tmp_path / ("b." + name)), "rb").read(), name


def test_a_chimera_free_file_is_left_alone(S, tmp_path):
    dirs = []
    for extra in (["--chimera_split"], []):
        d = tmp_path / str(len(dirs))
        d.mkdir()
        erb.main(["--mode", "tenX_v3", "-i", S["paths"]["clean"], "-o", str(d / "o.tsv"), "-t", "1", "--trimmed_reads", str(d / "t.fa"), "--chimera_cut"] + extra)
        dirs.append(str(d))
    _same_files(*dirs)


def test_a_bad_base_behind_a_boundary_names_the_input_read(S, tmp_path):
    """(the library knows the bad read of the chunk it queued last: the read is put into the input's last chunk, behind other chunks
    and behind pieces of its own chunk, so that neither the piece's number nor the number inside the chunk is the answer)"""
    n = len(S["reads"])
    victim = int(np.nonzero(np.bincount(S["rows"]["read"]) > 1)[0][-1])  # the last read with several pieces
    R = S["rows"]["read"]
    chunk = next(c for c in range(20, 200) if victim // c == (n - 1) // c and victim >= c and ((R >= victim // c * c) & (R < victim)).sum() > victim % c)
    reads = list(S["reads"])
    reads[victim] = reads[victim][:-30] + "X" + reads[victim][-29:]     # in its last piece
    fq = str(tmp_path / "bad.fastq")
    _fastq(fq, S["ids"], reads)
    ctx = _native.Context(0)
    L = _native.load()
    arr = (C.c_void_p * 1)(ctx.h)
    o = _native.Stage1OptsSplit(12, 1, 0, 0, chunk, 0, 0, _native.STAGE1_SPLIT)
    o.split_max_ed = E
    res = _native.Stage1ResultSplit()
    rc = L.bdg_stage1_run(arr, 1, os.fsencode(fq), os.fsencode(str(tmp_path / "bad.tsv")), b"#read_id",
                          C.cast(C.pointer(o), C.POINTER(_native.Stage1Opts)), C.cast(C.pointer(res), C.POINTER(_native.Stage1Result)))
    assert rc == _native.E_BADBASE and res.bad_read == victim, (res.bad_read, victim, chunk)
    assert "read %d of the chunk" % (victim % chunk) in L.bdg_last_error(ctx.h).decode()
    ctx.close()
    with pytest.raises(KeyError):
        erb.main(["--mode", "tenX_v3", "-i", fq, "-o", str(tmp_path / "bad2.tsv"), "-t", "1", "--chimera_split"])


def test_stage2_equals_the_presplit_file(S, tmp_path, caplog):
    """badger.py on reads with --chimera_split: every output file, both passes"""
    dirs = []
    for which, extra in (("a", ["--chimera_split"]), ("b", [])):
        d = tmp_path / which
        d.mkdir()
        caplog.clear()
        with redirect_stdout(io.StringIO()), caplog.at_level(logging.INFO, logger="BarcodeGraph"):
            badger.main(["-r", S["paths"][which], "-d", "tenX_v3", "-l", S["paths"]["wl"], "-c", str(N_CELLS), "-o", str(d / "s2"), "--umi_dedup",
                         "--tagged_reads", str(d / "tagged.fa"), "--molecule_consensus", str(d / "consensus.fa")] + extra)
        if which == "a":
            assert any("Split reads: %d reads cut into %d pieces" % S["counts"] in r.getMessage() for r in caplog.records)
        dirs.append(str(d))
    names = _same_files(*dirs)
    assert {"tagged.fa", "consensus.fa"} <= set(names) and len(names) >= 5
    assert open(os.path.join(dirs[0], "tagged.fa")).read().count("/2\t") > 20
