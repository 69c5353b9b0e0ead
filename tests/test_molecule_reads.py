"""Tagged reads without a GPU: the rule of badger_amd/molecule_reads.py against a literal dictionary form, the generators of
tests/molecule_cases.py against what they promise, the native formatter bdg_format_trimmed_tags against a Python text builder,
the command line's argument checks, and the layouts."""
import ctypes as C
import os

import numpy as np
import pytest

import chimera_cases as cc
import molecule_cases as mc
from badger_amd import _native, badger, chimera, common, molecule_reads as mr, trim
from badger_amd.umi_dedup import umi_code, umi_str

NONE = mr.NONE


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__
    __graft_entry__.build()


# ---- 1. the rule ----------------------------------------------------------------------------------------------------------
def _dict_rule(case):
    """the rule, read off its text: a dictionary of molecules, a count and a maximum each"""
    rep, cnt = [0] * case.n, [0] * case.n
    for members in case.groups().values():
        for i in members:
            cnt[i] = len(members)
        bidders = [i for i in members if int(case.length[i]) > 0]
        if bidders:
            rep[max(bidders, key=lambda i: (int(case.length[i]), -i))] = 1
    return np.array(rep, dtype=np.uint8), np.array(cnt, dtype=np.uint32)


def _all_cases():
    return [mc.case(name) for name in sorted(mc.GENERATORS)] + [mc.one_molecule(3000), mc.distinct_keys(512, 1), mc.distinct_keys(1024, 2)]


def test_checker_equals_the_dictionary_form():
    for case in _all_cases():
        got, want = case.rule(), _dict_rule(case)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), case
        assert got[0].dtype == np.uint8 and got[1].dtype == np.uint32
        # one representative per molecule with cDNA, none elsewhere
        groups = case.groups()
        assert int(got[0].sum()) == sum(1 for g in groups.values() if any(case.length[i] > 0 for i in g))
    # by hand: cell 7 holds molecule A (reads 0, 2, 3: lengths 5, 9, 9 -> read 2) and B (read 4, no cDNA); read 1 has no cell,
    # read 5 a rank that is no cell, read 6 no molecule
    a, b = umi_code("ACGTACGTACGT"), umi_code("ACGTACGTACGA")
    rep, cnt = mr.molecule_reps([7, 7, 7, 7, 7, 8, 7], [1, 0, 1, 1, 1, 1, 1], [a, a, a, a, b, a, NONE], [5, 50, 9, 9, 0, 9, 9], [7])
    assert rep.tolist() == [0, 0, 1, 0, 0, 0, 0] and cnt.tolist() == [3, 0, 3, 3, 1, 0, 0]
    # nothing at all
    rep, cnt = mr.molecule_reps([], [], [], [], [])
    assert len(rep) == 0 and len(cnt) == 0
    rep, cnt = mr.molecule_reps([3], [1], [a], [4], [])
    assert rep.tolist() == [0] and cnt.tolist() == [0]


def test_cdna_len():
    tr = np.zeros(6, dtype=_native.TRIM_DTYPE)
    ch = np.zeros(6, dtype=_native.CHIMERA_DTYPE)
    tr["cdna_start"], tr["cdna_end"], tr["flags"] = [10, 10, 10, 10, -1, 10], [50, 50, 50, 50, -1, 10], [1, 3, 1, 1, 0, 2]
    ch["cut"], ch["flags"] = [-1, 30, 10, 49, -1, -1], [0, 1, 1, 1, 0, 0]
    assert mr.cdna_len(tr).tolist() == [40, 40, 40, 40, 0, 0]
    assert mr.cdna_len(tr, ch).tolist() == [40, 20, 0, 39, 0, 0]
    # what the formatter writes: the same numbers
    S = cc.case_set()
    chim = chimera.chimera_batch(S["bases"], S["off"], S["recs"], S["trim"])
    ids = ["r%d" % i for i in range(len(S["reads"]))]
    want = [0] * len(ids)
    for i in range(len(ids)):
        text = chimera.fasta_text(ids[i:i + 1], S["reads"][i:i + 1], S["recs"][i:i + 1], S["trim"][i:i + 1], chim[i:i + 1])
        want[i] = len(text.split("\n")[1]) if text else 0
    assert mr.cdna_len(S["trim"], chim).tolist() == want and sum(1 for w in want if w == 0) > 10


# ---- 2. the generators ----------------------------------------------------------------------------------------------------
def _tied(case):
    """molecules whose longest cDNA is shared: list of the tied read indices"""
    out = []
    for members in case.groups().values():
        top = max(int(case.length[i]) for i in members)
        if top:
            t = [i for i in members if int(case.length[i]) == top]
            if len(t) > 1:
                out.append(t)
    return out


def test_generators_deliver_what_they_promise():
    assert [mc.case("mixed_%d" % n).n for n in (1, 63, 64, 65, 4097)] == [1, 63, 64, 65, 4097]
    big = mc.case("mixed_4097")
    inside = np.isin(big.rank, big.cells)
    assert (big.has == 0).sum() > 200 and (~inside).sum() > 200 and (big.mol == NONE).sum() > 200 and (big.length == 0).sum() > 400
    assert (big.length >= 1 << 16).sum() > 100 and len(_tied(big)) > 50
    groups = big.groups()
    assert max(len(g) for g in groups.values()) >= 4 and len(groups) > 500
    by_code = {}
    for c, u in groups:
        by_code.setdefault(u, set()).add(c)
    assert sum(1 for cs in by_code.values() if len(cs) > 1) > 50          # one code in several cells
    # one molecule
    one = mc.one_molecule(200000)
    g = one.groups()
    assert len(g) == 1 and len(next(iter(g.values()))) == 200000 and len(_tied(one)[0]) > 10000 and (one.length == 0).sum() > 50000
    # ties: inside a wave, across a wave boundary, across a block boundary; the earliest index wins
    wt = mc.case("wave_ties")
    tied = _tied(wt)
    assert len(tied) == len(wt.planted) >= 10
    assert sum(1 for t in tied if t[0] // 64 == t[1] // 64) >= 2 and sum(1 for t in tied if t[0] // 64 != t[1] // 64) >= 5
    assert any(t[0] % 64 == 63 and t[1] == t[0] + 1 for t in tied) and any(t[0] // 256 != t[-1] // 256 for t in tied)
    assert any(len(t) == 3 for t in tied)
    rep = wt.rule()[0]
    for t, extra in wt.planted:
        assert rep[t[0]] == 1 and not rep[t[1:]].any() and not rep[extra].any()
    assert any(len(e) == 2 and wt.length[e[0]] == 0 and e[0] < t[0] for t, e in wt.planted)
    # molecules without cDNA
    nc = mc.case("no_cdna")
    empty = [m for m in nc.groups().values() if not any(nc.length[i] for i in m)]
    assert len(empty) > 30 and sum(1 for m in empty if len(m) > 1) > 20
    rep, cnt = nc.rule()
    assert all(not rep[m].any() and (cnt[m] == len(m)).all() for m in empty)
    # long lengths: every special value is some molecule's longest, and ties among them exist
    ll = mc.case("long_lengths")
    tops = {max(int(ll.length[i]) for i in m) for m in ll.groups().values()}
    assert {65535, 65536, 65537, 1 << 31, 0xFFFFFFFF} <= set(ll.length.tolist()) and 0xFFFFFFFF in tops and len(_tied(ll)) > 5
    # one code, two cells
    tc = mc.case("two_cells_one_code")
    assert len(set(tc.mol.tolist())) == 1 and len(tc.groups()) == 2
    rep, cnt = tc.rule()
    assert rep.tolist() == [0, 0, 1, 0, 1, 0, 0, 0] and cnt.tolist() == [3, 4, 3, 4, 4, 0, 3, 4]
    # distinct keys: half-full tables
    for n, P in ((512, 1024), (1024, 2048)):
        d = mc.distinct_keys(n, seed=n)
        assert len(d.groups()) == n and mc.occupied(d, P)[0].sum() == n


# ---- 3. the formatter -----------------------------------------------------------------------------------------------------
def _tag_inputs():
    """the chimera cases (both strands, with and without a hit) with a TSO flag, a cell, a molecule and a keep bit dealt out
    so that every combination of the six occurs among the reads format_trimmed_chimera writes"""
    S = cc.case_set()
    n = len(S["reads"])
    recs, tr = S["recs"].copy(), S["trim"].copy()
    recs["bc_start"], recs["umi_start"], recs["umi_end"] = 30, 46, 58
    chim = chimera.chimera_batch(S["bases"], S["off"], recs, tr)
    rng = np.random.default_rng(12)
    cell = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    mol = np.array([umi_code("".join("ACGT"[c] for c in rng.integers(0, 4, size=int(rng.integers(10, 15))))) for _ in range(n)], dtype=np.uint32)
    mol_reads = rng.integers(1, 100000, size=n).astype(np.uint32)
    mol_reads[:4] = [1, 9, 10, 0xFFFFFFFF]
    # the four bits go round inside each (strand, hit) class of the reads that are written
    tso, has, keep = np.zeros(n, bool), np.ones(n, np.uint8), np.ones(n, np.uint8)
    turn = {}
    for i in np.flatnonzero(mr.cdna_len(tr, chim) > 0).tolist():
        cls = (int(recs[i]["flags"]) & _native.FLAG_REV, int(chim[i]["flags"]) & chimera.CHIMERA_HIT)
        k = turn[cls] = turn.get(cls, -1) + 1
        tso[i], has[i], keep[i] = k & 1, (k >> 1) & 1, (k >> 2) & 1
        if (k >> 3) & 1:
            mol[i] = NONE
    tr["flags"] = np.where(tso & ((tr["flags"] & trim.TRIM_EMIT) != 0), tr["flags"] | trim.TRIM_TSO, tr["flags"])
    return S, recs, tr, chim, cell, has, mol, mol_reads, keep


def test_format_trimmed_tags_against_python():
    from test_trim import _Chunk
    S, recs, tr, chim, cell, has, mol, mol_reads, keep = _tag_inputs()
    reads, n = S["reads"], len(S["reads"])
    ids = ["t%d" % i for i in range(n)]
    ids[5] = "t5 runid=9"
    ck = _Chunk(ids, reads)
    written = np.array([bool(chimera.fasta_text(ids[i:i + 1], reads[i:i + 1], recs[i:i + 1], tr[i:i + 1], chim[i:i + 1])) for i in range(n)])
    rev, hit = (recs["flags"] & _native.FLAG_REV) != 0, (chim["flags"] & chimera.CHIMERA_HIT) != 0
    combos = {(bool(rev[i]), bool(tr[i]["flags"] & trim.TRIM_TSO), bool(hit[i]), bool(has[i]), bool(mol[i] != NONE), bool(keep[i]))
              for i in range(n) if written[i]}
    assert len(combos) == 64
    for m, mrd, kp, cm in ((mol, mol_reads, keep, chim), (mol, mol_reads, None, chim), (None, None, keep, chim), (None, None, None, chim),
                           (mol, mol_reads, keep, None), (None, None, None, None)):
        text, counts = _native.format_trimmed_tags(ck.ch, recs, tr, cm, cell, has, m, mrd, kp)
        want, want_counts = mr.fasta_text(ids, reads, recs, tr, cm, cell, has, m, mrd, kp)
        assert text == want.encode() and counts == want_counts, (m is None, kp is None, cm is None)
        ok = written if cm is not None else (tr["flags"] & trim.TRIM_EMIT) != 0
        assert counts[2] == int((ok & (has == 0)).sum()) and counts[3] == (0 if kp is None else int((ok & (has != 0) & (kp == 0)).sum()))
        assert counts[0] == text.count(b">") == int(ok.sum()) - counts[2] - counts[3] and counts[0] > 50
        assert text.count(b"\tCB:Z:") == counts[0] and text.count(b"\tUB:Z:") == text.count(b"\tRN:i:")
        assert (text.count(b"\tUB:Z:") > 0) == (m is not None)
    # the fields by hand: CB, UB, RN in front of CH; a molecule of 2^32 - 1 reads
    text = _native.format_trimmed_tags(ck.ch, recs, tr, chim, cell, np.ones(n, np.uint8), mol, mol_reads)[0].decode()
    lines = {l.split("\t")[0][1:]: l.split("\t")[1:] for l in text.split("\n") if l.startswith(">")}
    i = next(i for i in range(n) if written[i] and hit[i] and mol[i] != NONE)
    f = lines["t%d" % i]
    assert [x[:5] for x in f] == ["CR:Z:", "UR:Z:", "ST:A:", "CB:Z:", "UB:Z:", "RN:i:", "CH:Z:"]
    assert f[3][5:] == common.unrank(int(cell[i]), 16) and f[4][5:] == umi_str(int(mol[i])) and f[5][5:] == str(int(mol_reads[i]))
    i = next(i for i in range(n) if written[i] and mol[i] == NONE and not hit[i])
    assert [x[:5] for x in lines["t%d" % i]] == ["CR:Z:", "UR:Z:", "ST:A:", "CB:Z:"]
    assert "t5" in lines or not written[5]
    if written[3] and mol[3] != NONE:
        assert lines["t3"][5] == "RN:i:4294967295"
    # the records and sequences are those of format_trimmed_chimera, in its order
    plain = _native.format_trimmed_chimera(ck.ch, recs, tr, chim)[0].decode().split("\n")
    tagged = text.split("\n")
    assert plain[1::2] == tagged[1::2] and [l.split("\t")[0] for l in plain[::2]] == [l.split("\t")[0] for l in tagged[::2]]


def test_format_trimmed_tags_sizing_and_errors():
    from test_trim import _Chunk
    S, recs, tr, chim, cell, has, mol, mol_reads, keep = _tag_inputs()
    ck = _Chunk(["q%d" % i for i in range(len(S["reads"]))], S["reads"])
    L = _native.load()
    p = lambda a: None if a is None else a.ctypes.data                    # noqa: E731
    counts = (C.c_uint64 * 4)(7, 7, 7, 7)

    def call(recs_=recs, tr_=tr, cell_=cell, has_=has, mol_=mol, mrd_=mol_reads, out=None, cap=0, counts_=counts):
        return L.bdg_format_trimmed_tags(C.byref(ck.ch), p(recs_), p(tr_), p(chim), p(cell_), p(has_), p(mol_), p(mrd_), p(keep), out, cap, counts_)

    need = call()
    text = _native.format_trimmed_tags(ck.ch, recs, tr, chim, cell, np.ones(len(cell), np.uint8), mol, mol_reads)[0]
    assert need >= len(text) > 0 and list(counts) == [7, 7, 7, 7]         # out == NULL: the size, nothing counted
    buf = C.create_string_buffer(b"\xAA" * 64, 64)
    assert call(out=buf, cap=64) == need and buf.raw == b"\xAA" * 64 and list(counts) == [7, 7, 7, 7]
    for bad in (dict(recs_=None), dict(tr_=None), dict(cell_=None), dict(has_=None), dict(mrd_=None)):
        assert call(**bad) == _native.E_ARG, bad
    assert call(mol_=None, mrd_=None) > 0 and call(counts_=None) == need
    none = np.zeros(len(tr), dtype=_native.TRIM_DTYPE)
    assert _native.format_trimmed_tags(ck.ch, recs, none, chim, cell, has, mol, mol_reads, keep) == (b"", (0, 0, 0, 0))


# ---- 4. arguments, layouts, symbols ---------------------------------------------------------------------------------------
def _args(*extra, reads="reads.fastq"):
    return ["-r", reads, "-d", "tenX_v3", "-o", "out"] + list(extra)


def test_tagged_reads_needs_read_input(capsys):
    with pytest.raises(SystemExit):
        badger.parse_args(_args("--tagged_reads", "t.fa", reads="stage1.tsv"))
    err = capsys.readouterr().err
    assert "--tagged_reads" in err and "bases" in err and "TSV" in err
    for reads in ("r.fa", "r.fastq.gz", "r.sam", "r.bam"):
        assert badger.parse_args(_args("--tagged_reads", "t.fa", reads=reads)).tagged_reads == "t.fa"


def test_molecule_reads_needs_dedup_and_tagged_reads(capsys):
    for extra in (("--molecule_reads",), ("--molecule_reads", "--umi_dedup"), ("--molecule_reads", "--tagged_reads", "t.fa")):
        with pytest.raises(SystemExit):
            badger.parse_args(_args(*extra))
        assert "--molecule_reads needs --umi_dedup and --tagged_reads" in capsys.readouterr().err
    a = badger.parse_args(_args("--molecule_reads", "--umi_dedup", "--tagged_reads", "t.fa"))
    assert a.molecule_reads and a.tso_min_score == 20 and not a.chimera_cut and a.chimera_max_ed is None


@pytest.mark.parametrize("extra", [("--tso_min_score", "20"), ("--chimera_cut",), ("--tagged_reads", "t.fa", "--chimera_max_ed", "2"),
                                   ("--tagged_reads", "t.fa", "--tso_min_score", "7"), ("--tagged_reads", "t.fa", "--tso_min_score", "31"),
                                   ("--tagged_reads", "t.fa", "--chimera_cut", "--chimera_max_ed", "7"),
                                   ("--tagged_reads", "t.fa", "--chimera_cut", "--chimera_max_ed", "x")])
def test_trim_flags_need_tagged_reads_and_their_ranges(extra):
    with pytest.raises(SystemExit):
        badger.parse_args(_args(*extra))


def test_flags_parse():
    a = badger.parse_args(_args())
    assert a.tagged_reads is None and not a.molecule_reads and not a.chimera_cut
    a = badger.parse_args(_args("--tagged_reads", "t.fa", "--chimera_cut"))
    assert a.chimera_max_ed == chimera.MAX_ED_DEFAULT and a.tso_min_score == _native.TSO_MIN_SCORE_DEFAULT
    a = badger.parse_args(_args("--tagged_reads", "t.fa", "--chimera_cut", "--chimera_max_ed", "0", "--tso_min_score", "30"))
    assert (a.chimera_max_ed, a.tso_min_score) == (0, 30)


def test_layouts_and_symbols():
    assert _native.Stage1OptsTags.tag_cell_rank.offset == C.sizeof(_native.Stage1OptsChimera) == 80
    assert C.sizeof(_native.Stage1OptsTags) == 80 + 6 * 8 and _native.Stage1OptsTags.tag_reads.offset == 120
    assert _native.Stage1ResultTags.tags_no_cell.offset == C.sizeof(_native.Stage1ResultChimera)
    assert _native.STAGE1_TAGS == 0x1000
    assert _native.STAGE1_TAGS & (_native.STAGE1_TRIM | _native.STAGE1_CHIMERA | _native.STAGE1_WL_CANDIDATES | _native.STAGE1_WL_CORRECT | 0xFF) == 0
    hdr = open(os.path.join(os.path.dirname(_native._HERE), "include", "badger_hip.h")).read()
    L = _native.load()
    for name in ("bdg_extract_keep_cdna", "bdg_kept_cdna", "bdg_molecule_reps_dev", "bdg_molecule_reps_set_aggregate", "bdg_format_trimmed_tags"):
        assert name in _native.EXPORTS and hasattr(L, name) and ("%s(" % name) in hdr
    assert "BDG_STAGE1_TAGS          0x1000u" in hdr and "cdna_len << 32 | (0xFFFFFFFF - i)" in hdr
