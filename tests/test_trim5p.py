"""The 5' layout without a GPU: the two forms of badger_amd/trim5p.py against each other and against hand-derived answers, the
record rule on the false-polyT reads of the 3' rule (records from the CPU oracle), the native FASTA formatters with
BDG_TRIM_SENSE against the Python writers, the command lines' argument checks, and the header / binding bookkeeping."""
import numpy as np
import pytest

from badger_amd import _native, badger, chimera, common, extract_raw_barcodes as erb, molecule_reads as mr, synth, trim, trim5p
from badger_amd.umi_dedup import UMI_LEN, umi_code
from oracle import pyoracle as orc

import fivep_cases as fc

FIELDS = ("cdna_start", "cdna_end", "tail_len", "tso_score", "flags")


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__
    __graft_entry__.build()


def _same(got, want, what, names=None):
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert not len(bad), (what, f, [names[i] for i in bad[:5]] if names else bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


# ---- 1. the rule --------------------------------------------------------------------------------------------------------
def test_anchor_and_tail_by_hand():
    A = trim5p.TSO5
    assert trim5p.anchor_search(A) == (0, 12) and trim5p.anchor_search("") == (13, -1)
    assert trim5p.anchor_search("GGC" + A + "CAT") == (0, 15)
    assert trim5p.anchor_search("GGC" + A[:5] + A[6:] + "CAT") == (1, 14)                    # one deletion
    assert trim5p.anchor_search("GGC" + A[:5] + "N" + A[6:] + "CAT")[0] == 1                  # N equals nothing
    assert trim5p.anchor_search(A + "G")[1] == 12                                             # a fourth G stays in the cDNA
    assert trim5p.anchor_search(A[:-1]) == (1, 11)                                            # the text ends inside the oligo
    s = "CGT" * 10 + "A" * 30
    assert trim5p.tail_begin(s, 0, len(s)) == 30 and trim5p.tail_begin(s, 40, len(s)) == 40   # (stops at cdna_start)
    assert trim5p.tail_begin("CGTCGT", 0, 6) == 6
    assert trim5p.tail_begin("CCC" + "A" * 12 + "C" + "A" * 17, 0, 33) == 3                   # one non-A inside: -2 + 12 > 0
    assert trim5p.tail_begin("CCC" + "A" * 30 + "CGTCG" + "A" * 3, 0, 41) == 38               # five non-A end the walk: the last three A only
    # a whole strand: cuts behind the oligo, in front of the tail; the primer's cut at its first base
    umi, cdna = "ACGTACGTAC", "GCTGCATCGGCTACGGCTTCAGCGGCATCGTCGCATGCTG"
    s = "AC" + synth.R1 + "A" * 16 + umi + A + cdna + "A" * 30 + trim5p.PRIMER
    us = 2 + 22 + 16
    st, en, tl, sc, fl = trim5p.trim_strand(s, us, us + 10)
    assert (st, en, tl, sc) == (us + 10 + 13, us + 10 + 13 + len(cdna), 30, 25)
    assert fl == trim5p.TRIM_ANCHOR | trim.TRIM_TSO | trim.TRIM_EMIT | trim.TRIM_SENSE and trim5p.anchor_ed(fl) == 0
    assert trim5p.trim_strand(s.replace(A, "CACACACACACAC"), us, us + 10) == (-1, -1, 0, 0, trim5p.TRIM_NO_ANCHOR)
    assert trim5p.trim_strand(s, us, us + 10, tso_min_score=25)[3] == 25 and trim5p.trim_strand(s[:-1], us, us + 10, tso_min_score=25)[1:3] == (len(s) - 1, 0)


@pytest.mark.parametrize("umi_len,max_ed,score", [(10, 2, 16), (12, 0, 8), (12, 4, 25), (10, 1, 16)])
def test_batch_form_equals_one_read_form(umi_len, max_ed, score):
    S = fc.trim_cases(umi_len, max_ed)
    one = trim5p.trim_reads(S["reads"], S["recs"], umi_len, max_ed, score)
    many = trim5p.trim_batch(S["bases"], S["off"], S["recs"], umi_len, max_ed, score)
    _same(many, one, "batch form", S["names"])


def test_cases_deliver_what_they_promise():
    S = fc.trim_cases(10, 2)
    t = trim5p.trim_batch(S["bases"], S["off"], S["recs"], 10, 2, 16)
    by = {}
    for name, r in zip(S["names"], t):
        by.setdefault(name.replace(" (rev)", ""), []).append(r)
    fl = lambda name: [int(r["flags"]) for r in by[name]]                                  # noqa: E731
    for offs in range(-3, 4):
        assert all(f & trim5p.TRIM_ANCHOR for f in fl("anchor off %d edits 0" % offs)), offs
    assert {trim5p.anchor_ed(f) for k in range(3) for o in range(-3, 4) for f in fl("anchor off %d edits %d" % (o, k)) if f & trim5p.TRIM_ANCHOR} == {0, 1, 2}
    assert any(f == trim5p.TRIM_NO_ANCHOR for o in range(-3, 4) for f in fl("anchor off %d edits 3" % o))
    assert all(f == 0 for name in ("ends inside the UMI", "invalid", "incomplete") for f in fl(name))
    assert all(not f & trim.TRIM_EMIT for f in fl("ends behind the anchor") + fl("ends inside the anchor"))
    assert all(int(r["tail_len"]) == 32767 for r in by["tail of 33000"])
    assert all(int(r["cdna_end"]) == int(r["cdna_start"]) and not r["flags"] & trim.TRIM_EMIT for r in by["cdna of A"])
    assert all(f & trim.TRIM_TSO for f in fl("primer without tail")) and not any(f & trim.TRIM_TSO for f in fl("tail without primer"))
    assert all(int(r["tail_len"]) == 0 for r in by["primer without tail"] + by["no tail no primer"])
    assert all(int(r["tail_len"]) == 36 for r in by["tail with 4 non-A"]) and any(int(r["tail_len"]) < 36 for r in by["tail with 5 non-A"])
    assert {int(r["cdna_end"]) - int(r["cdna_start"]) for r in by["cdna 8 with far end"]} == {8}


# ---- 2. the record rule -------------------------------------------------------------------------------------------------
def _false_polyt_reads(umi_len, n=60, seed=3):
    """error-free 5' reads whose UMI ends in TT: with the oligo's TTT behind it the 3' rule's local polyT re-search succeeds"""
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n):
        s = (fc._rs(rng, int(rng.integers(0, 30))) + synth.R1 + fc._rs(rng, 16) + fc._rs(rng, umi_len - 2) + "TT" + trim5p.TSO5
             + "C" + fc._rs(rng, 294, "ACG") + "CGCGC" + "A" * 30 + trim5p.PRIMER)     # (five non-A: the tail's walk ends there)
        reads.append(trim.revcomp(s) if i & 1 else s)
    return reads


@pytest.mark.parametrize("umi_len", [10, 12])
def test_record_rule_on_false_polyt_reads(umi_len):
    reads = _false_polyt_reads(umi_len)
    bases, off = synth.list_to_reads(reads)
    r3 = orc.extract_batch(bases, off, umi_len, threads=2)
    assert (r3["valid"] == 1).all()
    short = (r3["polyT"] >= 0) & (r3["umi_end"] - r3["umi_start"] < umi_len)
    assert short.sum() >= len(reads) // 2                 # the false polyT of the 3' rule: a UMI column two or more bases short
    r5 = trim5p.fixup_records(r3, np.diff(off.astype(np.int64)), umi_len)
    assert (r5["polyT"] == -1).all() and (r5["umi_end"] - r5["umi_start"] == umi_len).all()
    assert (r5["umi_start"] == r3["bc_start"] + 16).all()
    assert (r5["strand"] == np.where(np.arange(len(reads)) & 1, -1, 1)).all()
    for f in ("r1_end", "bc_start", "bc_rank", "r1_score", "valid", "flags", "reserved"):
        assert (r5[f] == r3[f]).all(), f
    # the one-record form says the same; invalid and placeholder records
    r3[3]["valid"] = 0
    r3[4]["flags"] |= _native.FLAG_INCOMPLETE
    r5 = trim5p.fixup_records(r3, np.diff(off.astype(np.int64)), umi_len)
    one = np.array([trim5p.fixup_record(r, int(off[i + 1] - off[i]), umi_len) for i, r in enumerate(r3)], dtype=_native.REC_DTYPE)
    assert (one == r5).all()
    assert r5[3]["polyT"] == -1 and r5[3]["strand"] == 0 and r5[3]["umi_end"] == r3[3]["umi_end"] and r5[4] == r3[4]
    # ... and the trimming rule then finds every planted cDNA
    t = trim5p.trim_batch(bases, off, r5, umi_len)
    ok = np.ones(len(reads), bool)
    ok[[3, 4]] = False
    assert ((t["flags"][ok] & trim.TRIM_EMIT) != 0).all() and (t["cdna_end"][ok] - t["cdna_start"][ok] == 300).all()


# ---- 3. the formatters ---------------------------------------------------------------------------------------------------
def _format_inputs():
    """5' reads with and without a planted R1 junction in the cDNA, both strands; SENSE, the TSO flag, a cell and a keep bit dealt
    out so that every combination occurs among the reads the chimera form writes"""
    rng = np.random.default_rng(21)
    strands = []
    for i in range(160):
        body = fc._rs(rng, int(rng.integers(60, 200)), "CGT")
        if i & 2:
            body += synth.R1 + fc._rs(rng, 16) + fc._rs(rng, 60, "CGT")                      # a second molecule ligated behind
        strands.append(fc._rs(rng, int(rng.integers(0, 20))) + synth.R1 + fc._rs(rng, 16) + fc._rs(rng, 12) + trim5p.TSO5 + body
                       + "A" * 25 + trim5p.PRIMER)
    reads = [trim.revcomp(s) if i & 1 else s for i, s in enumerate(strands)]
    bases, off = synth.list_to_reads(reads)
    recs = trim5p.fixup_records(orc.extract_batch(bases, off, 12, threads=2), np.diff(off.astype(np.int64)), 12)
    tr = trim5p.trim_batch(bases, off, recs, 12)
    n = len(reads)
    turn, sense, tso, has, keep = {}, np.ones(n, bool), np.zeros(n, bool), np.ones(n, np.uint8), np.ones(n, np.uint8)
    chim = chimera.chimera_batch(bases, off, recs, tr)
    for i in np.flatnonzero(mr.cdna_len(tr, chim) > 0).tolist():
        cls = (int(recs[i]["flags"]) & _native.FLAG_REV, int(chim[i]["flags"]) & chimera.CHIMERA_HIT)
        k = turn[cls] = turn.get(cls, -1) + 1
        sense[i], tso[i], has[i], keep[i] = k & 1, (k >> 1) & 1, (k >> 2) & 1, (k >> 3) & 1
    fl = tr["flags"] & ~np.uint8(trim.TRIM_TSO | trim.TRIM_SENSE)
    emit = (tr["flags"] & trim.TRIM_EMIT) != 0
    tr["flags"] = fl | np.where(emit & sense, trim.TRIM_SENSE, 0).astype(np.uint8) | np.where(emit & tso, trim.TRIM_TSO, 0).astype(np.uint8)
    return reads, bases, off, recs, tr, chim, has, keep


def test_native_formatters_with_sense_against_python():
    from test_trim import _Chunk
    reads, bases, off, recs, tr, chim, has, keep = _format_inputs()
    n = len(reads)
    ids = ["r%d" % i for i in range(n)]
    ck = _Chunk(ids, reads)
    rev, hit = (recs["flags"] & _native.FLAG_REV) != 0, (chim["flags"] & chimera.CHIMERA_HIT) != 0
    written = mr.cdna_len(tr, chim) > 0
    combos = {(bool(rev[i]), bool(tr[i]["flags"] & trim.TRIM_SENSE), bool(tr[i]["flags"] & trim.TRIM_TSO), bool(hit[i]), bool(has[i]), bool(keep[i]))
              for i in range(n) if written[i]}
    assert len(combos) == 64
    # the sequences by hand: with SENSE the strand's text as it stands, without it its reverse complement
    text, counts = _native.format_trimmed(ck.ch, recs, tr)
    assert text == trim.fasta_text(ids, reads, recs, tr).encode() and counts[0] == int(((tr["flags"] & trim.TRIM_EMIT) != 0).sum()) > 100
    seqs = dict(zip([l[1:].split("\t")[0] for l in text.decode().split("\n")[:-1:2]], text.decode().split("\n")[1::2]))
    for i in range(n):
        if tr[i]["flags"] & trim.TRIM_EMIT:
            s = trim.revcomp(reads[i]) if rev[i] else reads[i]
            piece = s[int(tr[i]["cdna_start"]):int(tr[i]["cdna_end"])]
            assert seqs[ids[i]] == (piece if tr[i]["flags"] & trim.TRIM_SENSE else trim.revcomp(piece)), i
    text_c, counts_c = _native.format_trimmed_chimera(ck.ch, recs, tr, chim)
    assert text_c == chimera.fasta_text(ids, reads, recs, tr, chim).encode() and counts_c[3:] == chimera.counts(tr, chim)
    assert counts_c[3] > 20 and text_c.count(b"\tCH:Z:") == counts_c[3]
    cell = np.random.default_rng(4).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    mol = np.full(n, umi_code("ACGTACGTACGT"), dtype=np.uint32)
    mol_reads = np.arange(1, n + 1, dtype=np.uint32)
    for cm, kp, m in ((chim, keep, mol), (chim, None, None), (None, keep, mol)):
        text_t, counts_t = _native.format_trimmed_tags(ck.ch, recs, tr, cm, cell, has, m, mol_reads if m is not None else None, kp)
        want, want_counts = mr.fasta_text(ids, reads, recs, tr, cm, cell, has, m, mol_reads if m is not None else None, kp)
        assert text_t == want.encode() and counts_t == want_counts and counts_t[0] > 10


# ---- 4. the command lines ------------------------------------------------------------------------------------------------
def _erb(*extra, mode="tenX_5p_v2"):
    return erb.parse_args(["--mode", mode, "-i", "reads.fastq", "-o", "out.tsv"] + list(extra))


def _bdg(*extra, dtype="tenX_5p_v2"):
    return badger.parse_args(["-r", "reads.fastq", "-d", dtype] + list(extra))


def test_new_modes_parse():
    for mode, umi in (("tenX_5p_v2", 10), ("tenX_5p_v3", 12)):
        a = _erb(mode=mode)
        det = erb.BARCODE_CALLING_MODES[a.mode]
        assert det.LAYOUT == _native.LAYOUT_5P and det(device=0).UMI_LEN_10X == umi == UMI_LEN[mode] and erb.is_5p_mode(mode)
        assert _bdg(dtype=mode).data_type == mode
    assert not erb.is_5p_mode("tenX_v3") and erb.BARCODE_CALLING_MODES["tenX_v3"].LAYOUT == _native.LAYOUT_3P
    a = _erb("--trimmed_reads", "t.fa", "--tso5_max_ed", "3", "--tso_min_score", "25", "--chimera_cut")
    assert erb._trim_kwargs(a) == dict(trimmed_path="t.fa", tso_min_score=25, tso5_max_ed=3, chimera_max_ed=_native.CHIMERA_MAX_ED_DEFAULT)
    assert erb._trim_kwargs(_erb("--trimmed_reads", "t.fa")) == dict(trimmed_path="t.fa", tso_min_score=16, tso5_max_ed=2)
    assert erb._trim_kwargs(_erb("--trimmed_reads", "t.fa", mode="tenX_v3")) == dict(trimmed_path="t.fa", tso_min_score=20)
    b = _bdg("--tagged_reads", "t.fa", "--tso5_max_ed", "0")
    assert (b.tso5_max_ed, b.tso_min_score) == (0, 16) and _bdg("--tagged_reads", "t.fa", dtype="tenX_v2").tso5_max_ed is None
    assert _bdg(dtype="tenX_v2").tso_min_score == 20


@pytest.mark.parametrize("extra,mode", [(("--tso5_max_ed", "2"), "tenX_5p_v2"),                       # without --trimmed_reads
                                        (("--trimmed_reads", "t.fa", "--tso5_max_ed", "2"), "tenX_v3"),  # without a 5' mode
                                        (("--trimmed_reads", "t.fa", "--tso5_max_ed", "5"), "tenX_5p_v3"),
                                        (("--trimmed_reads", "t.fa", "--tso5_max_ed", "-1"), "tenX_5p_v3"),
                                        (("--trimmed_reads", "t.fa", "--tso5_max_ed", "x"), "tenX_5p_v3"),
                                        (("--trimmed_reads", "t.fa", "--tso_min_score", "26"), "tenX_5p_v2")])
def test_tso5_max_ed_prerequisites(extra, mode, capsys):
    with pytest.raises(SystemExit) as e:
        _erb(*extra, mode=mode)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "tso5_max_ed" in err or "tso_min_score" in err
    with pytest.raises(SystemExit) as e:
        _bdg(*[x.replace("--trimmed_reads", "--tagged_reads") for x in extra], dtype=mode)
    assert e.value.code == 2


def test_help_texts_format(capsys):
    for parse in (erb.parse_args, badger.parse_args):
        with pytest.raises(SystemExit) as e:
            parse(["--help"])
        assert e.value.code == 0
        out = " ".join(capsys.readouterr().out.split())
        assert "--tso5_max_ed" in out and "tenX_5p_v2" in out
    with pytest.raises(SystemExit):
        erb.parse_args(["--help"])
    out = " ".join(capsys.readouterr().out.split())
    assert "default 16" in out and "4 of 100,000" in out and "99.1 %" in out and "27 of 100,000" in out


def test_layouts_and_symbols():
    import ctypes as C
    L = _native.load()
    assert {"bdg_extract_set_layout", "bdg_trim_set_5p"} <= set(_native.EXPORTS)
    assert L.bdg_extract_set_layout(None, 0) == _native.E_ARG and L.bdg_trim_set_5p(None, 10, 2) == _native.E_ARG
    assert C.sizeof(_native.Stage1Result5p) == C.sizeof(_native.Stage1ResultTags) + 8
    hdr = open(common.__file__.replace("badger_amd/common.py", "include/badger_hip.h")).read()
    for name, v in (("BDG_LAYOUT_5P", _native.LAYOUT_5P), ("BDG_TRIM5P_MAX_ED_DEFAULT", _native.TSO5_MAX_ED_DEFAULT),
                    ("BDG_TRIM5P_MAX_ED_MAX", _native.TSO5_MAX_ED_MAX), ("BDG_TRIM5P_MIN_SCORE_DEFAULT", _native.TSO5_MIN_SCORE_DEFAULT),
                    ("BDG_TRIM5P_PRIMER_LEN", len(trim5p.PRIMER))):
        assert ("#define %s %d" % (name, v)) in " ".join(hdr.split()), name
    assert '"%s"' % trim5p.TSO5 in hdr and trim.TSO.endswith(trim5p.PRIMER)
    assert (trim.TRIM_SENSE, trim5p.TRIM_ANCHOR, trim5p.TRIM_NO_ANCHOR) == (_native.TRIM_SENSE, _native.TRIM_ANCHOR, _native.TRIM_NO_ANCHOR) == (4, 8, 128)
    assert trim5p.MIN_SCORE_DEFAULT == _native.TSO5_MIN_SCORE_DEFAULT and trim5p.MIN_SCORE_RANGE[1] == _native.TSO5_MIN_SCORE_MAX


def test_make_reads_5p():
    wl = synth.make_whitelist(100)
    b1, o1, t = synth.make_reads_5p(50, wl, seed=2, umi_len=12, clean_every=2, with_truth=True)
    b2, o2 = synth.make_reads_5p(50, wl, seed=2, umi_len=12, clean_every=2)
    assert (b1 == b2).all() and (o1 == o2).all() and set(bytes(b1)) <= set(b"ACGT")
    raw = b1.tobytes()
    for i in range(0, 50, 2):                              # the error-free ones hold their layout verbatim
        s = raw[int(o1[i]):int(o1[i + 1])].decode()
        s = trim.revcomp(s) if t["revcomp"][i] else s
        core = synth.R1 + common.unrank(int(t["barcode"][i]), 16) + t["umi"][i] + trim5p.TSO5 + t["cdna"][i] + "A" * 30 + trim5p.PRIMER
        assert s.endswith(core) and len(s) - len(core) <= 40
    assert t["revcomp"].sum() not in (0, 50)
