"""The barcode rescue rule (badger_amd/rescue.py, the specification in include/badger_hip.h) on the hand-built reads of
tests/rescue_cases.py, its polyT against the oracle's, the record layout, and the command line's checks.  No GPU."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import rescue_cases as rc
from badger_amd import _native, extract_raw_barcodes as erb, rescue, synth
from badger_amd.trim import revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def S():
    s = rc.build()
    s["matcher"] = rescue.Matcher(s["wl"])
    return s


def _fields(t):
    return dict(zip(rescue.FIELDS[1:], t))


def test_every_case_gives_what_the_rule_says(S):
    names = [c[0] for c in S["cases"]]
    assert len(set(names)) == len(names) >= 26
    for name, read, rec, want in S["cases"]:
        got = rescue.rescue_read(read, rc.U, S["matcher"], S["support"]) if rescue.eligible(rec) else None
        if want is None:
            assert got is None, name
        else:
            assert got is not None and _fields(got) == {k: want[k] for k in rescue.FIELDS[1:]}, (name, got, want)


def test_batch_form_and_the_five_prime_layout(S):
    reads = [c[1] for c in S["cases"]]
    recs = np.array([c[2] for c in S["cases"]], dtype=_native.REC_DTYPE)
    bases, off = synth.list_to_reads(reads)
    got = rescue.rescue_batch(bases, off, recs, rc.U, S["wl"], S["support"], matcher=S["matcher"])
    want = [(i, c[3]) for i, c in enumerate(S["cases"]) if c[3] is not None]
    assert got["read"].tolist() == [i for i, _ in want]
    for g, (_, w) in zip(got, want):
        assert {k: g[k].item() if k != "umi" else bytes(g[k]) for k in rescue.FIELDS[1:]} == {k: w[k] for k in rescue.FIELDS[1:]}
    st = got["status"]
    assert {int(x) for x in st} == {rescue.NONE, rescue.RESCUED, rescue.AMBIGUOUS, rescue.TRUNCATED}
    assert rescue.counts(recs, got) == (len(reads) - 2, int((st == 1).sum()), int((st == 2).sum()), int((st == 3).sum()))
    assert len(rescue.rescue_batch(bases, off, recs, rc.U, S["wl"], S["support"], layout=1, matcher=S["matcher"])) == 0
    # a rescued UMI is s[b + 16 : p], U - d letters
    for g in got[st == rescue.RESCUED]:
        s = reads[g["read"]] if g["strand"] > 0 else revcomp(reads[g["read"]])
        assert g["umi"].decode() == s[g["bc_start"] + 16:g["polyT"]] and len(g["umi"]) == rc.U - g["offset"]
        assert g["bc_start"] == g["polyT"] - rc.U - 16 + g["offset"]
    for bad in ((0, 1), (15, 1), (12, 3)):
        with pytest.raises(ValueError):
            rescue.rescue_batch(bases, off, recs, bad[0], S["wl"], S["support"], max_ed=bad[1], matcher=S["matcher"])


def test_settings_move_the_cases_as_the_rule_says(S):
    by = {c[0]: c for c in S["cases"]}
    one = lambda name, D, M: rescue.rescue_read(by[name][1], rc.U, S["matcher"], S["support"], D, M)    # noqa: E731
    # min_support 1 lets the entry with one hit in; 3 shuts the one with two out
    assert _fields(one("support M - 1", 1, 1))["status"] == rescue.RESCUED
    assert _fields(one("support exactly M", 1, 3))["status"] == rescue.NONE
    # at min_support 1 the second neighbour counts again
    assert _fields(one("the same with one entry below M", 1, 1))["status"] == rescue.AMBIGUOUS
    # at distance 0 the two neighbours, and the ten, are out of reach
    assert _fields(one("two entries at the smallest distance", 0, 2))["status"] == rescue.NONE
    assert _fields(one("ten entries within distance 1 of the window", 0, 2))["status"] == rescue.NONE
    # at distance 2 a window one letter on reaches the entry too, but never nearer than the exact one
    for d in range(-2, 3):
        f = _fields(one("offset %+d alone" % d, 2, 2))
        assert (f["status"], f["dist"], f["offset"]) == (rescue.RESCUED, 0, d)


def test_the_answer_ignores_the_order_of_candidates(S):
    rng = random.Random(7)
    for name, read, rec, want in S["cases"]:
        cands = rescue.candidates(read, rc.U)
        if not cands:
            continue
        for D in (0, 1, 2):
            lists = [S["matcher"].topk(c[4], D) for c in cands]
            st, entry, e, i = rescue.resolve(cands, lists, S["support"], 2)
            for _ in range(5):
                perm = list(range(len(cands)))
                rng.shuffle(perm)
                st2, entry2, e2, i2 = rescue.resolve([cands[k] for k in perm], [lists[k] for k in perm], S["support"], 2)
                assert (st2, entry2, e2, None if i2 is None else perm[i2]) == (st, entry, e, i), name


def test_candidates_number_at_most_ten_and_rank_packs_like_the_records(S):
    for _, read, _, _ in S["cases"]:
        cands = rescue.candidates(read, rc.U)
        assert len(cands) <= 10
        for strand, p, d, b, w in cands:
            assert rescue.window_rank(w) == synth.str_to_rank(w) and -rescue.SLACK <= d <= rescue.SLACK and b == p - rc.U - 16 + d


def test_matcher_equals_a_plain_scan(S):
    """the deletion-variant lookup finds what comparing a window with every entry finds"""
    m = S["matcher"]
    rng = np.random.default_rng(3)
    windows = [rc.CENTRE, rc.W_AMB, rc.E_P, rc.E_S] + [synth.rank_to_str(r) for r in rng.choice(S["wl"], 6)]
    windows += [w[:5] + "T" + w[5:15] for w in windows[4:7]] + [w[1:] + "G" for w in windows[4:7]]
    for w in windows:
        want = sorted((d, i) for i, d in enumerate(rescue.lev(w, x) for x in m.wl) if d <= 2)
        assert m.near(w) == want, w
        for D in (0, 1, 2):
            top, n = m.topk(w, D)
            assert n == sum(1 for d, _ in want if d <= D) and top == [x for x in want if x[0] <= D][:8]


def test_find_polyt_start_equals_the_oracle_on_both_strands():
    from oracle import pyoracle as orc
    from test_trim_gpu import _adversarial
    wl = synth.make_whitelist(500)
    b, o = synth.make_reads(400, wl, seed=17)
    reads = synth.reads_to_list(b, o)
    reads += _adversarial(reads, 18, 12)
    reads += ["", "T", "T" * 15, "T" * 16, "T" * 17, "A" * 17, "ACGT" * 4, "TTTTTTTTTTTTACGTA", "ACGT" + "T" * 12 + "A", "N" * 40,
              "GCGC" + "TTATTATTATTATTATTATT" + "GC", "C" * 20 + "T" * 11 + "C" * 20, "C" * 20 + "T" * 12 + "C" * 20]
    seen = set()
    for s in reads:
        for t in (s, revcomp(s)):
            p = rescue.find_polyt_start(t)
            assert p == orc.find_polyt_start(t), t[:80]
            seen.add(p < 0)
    assert seen == {True, False}


def test_record_layout_is_as_declared():
    text = open(os.path.join(ROOT, "include", "badger_hip.h")).read()
    m = re.search(r"typedef struct bdg_rescue_rec \{(.*?)\} bdg_rescue_rec;\s*/\* (\d+) bytes \*/", text, re.S)
    assert m and int(m.group(2)) == 40 == _native.RESCUE_DTYPE.itemsize == rescue.RESCUE_DTYPE.itemsize
    names = re.findall(r"\b(\w+)(?:\[16\])?;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert tuple(names) == _native.RESCUE_DTYPE.names == rescue.RESCUE_DTYPE.names
    assert [_native.RESCUE_DTYPE.fields[n][1] for n in names] == [0, 4, 8, 12, 16, 20, 21, 22, 23, 24]
    consts = dict(re.findall(r"#define (BDG_RESCUE_\w+)\s+(\d+)", text))
    assert (consts["BDG_RESCUE_SLACK"], consts["BDG_RESCUE_MAX_ED_DEFAULT"], consts["BDG_RESCUE_MAX_ED_MAX"],
            consts["BDG_RESCUE_MIN_SUPPORT_DEFAULT"]) == ("2", "1", "2", "2")
    assert (rescue.SLACK, rescue.MAX_ED_DEFAULT, rescue.MAX_ED_MAX, rescue.MIN_SUPPORT_DEFAULT, rescue.UMI_MAX) == \
        (_native.RESCUE_SLACK, _native.RESCUE_MAX_ED_DEFAULT, _native.RESCUE_MAX_ED_MAX, _native.RESCUE_MIN_SUPPORT_DEFAULT, _native.RESCUE_UMI_MAX)
    assert [int(consts["BDG_RESCUE_" + s.upper()]) for s in rescue.STATUS] == [0, 1, 2, 3]
    # the trailing fields of the run's structs: the options behind the tags', the counts behind the 5' layout's
    assert C.sizeof(_native.Stage1OptsRescue) == C.sizeof(_native.Stage1OptsTags) + 16
    assert C.sizeof(_native.Stage1ResultRescue) == C.sizeof(_native.Stage1Result5p) + 32
    assert int(re.search(r"#define BDG_STAGE1_WL_RESCUE\s+0x([0-9a-f]+)u", text).group(1), 16) == _native.STAGE1_WL_RESCUE == 0x2000


def test_rows_of_the_rescued_file(S):
    reads = [c[1] for c in S["cases"]]
    recs = np.array([c[2] for c in S["cases"]], dtype=_native.REC_DTYPE)
    bases, off = synth.list_to_reads(reads)
    got = rescue.rescue_batch(bases, off, recs, rc.U, S["wl"], S["support"], matcher=S["matcher"])
    ids = ["r%d" % i for i in range(len(reads))]
    rows = rescue.rows(ids, got, S["wl"])
    assert rows[0] == rescue.HEADER and len(rows) == 1 + int((got["status"] != rescue.NONE).sum())
    assert rows[1] == "r0\t%s\t0\t5\t+\t%d\t0\t%s\trescued" % (rc.E_A, len(rc.PRE) + 28, rc.UMI)
    assert "r1\t%s\t0\t5\t-\t33\t0\t%s\trescued" % (rc.E_B, rc.UMI) in rows
    assert "r2\t*\t0\t0\t.\t-1\t0\t*\tambiguous" in rows
    assert any(r.endswith("\t*\t1\t0\t.\t-1\t0\t*\ttruncated") for r in rows)


@pytest.mark.parametrize("argv", [
    ["--bc_rescue"],                                                     # needs --bc_correct
    ["--bc_correct", "--rescue_max_ed", "1"],                            # needs --bc_rescue
    ["--bc_correct", "--rescue_min_support", "3"],
    ["--bc_correct", "--bc_rescue", "--rescue_max_ed", "3"],             # out of range
    ["--bc_correct", "--bc_rescue", "--rescue_max_ed", "x"],
    ["--bc_correct", "--bc_rescue", "--rescue_min_support", "-1"],
    ["--bc_correct", "--bc_rescue", "--mode", "tenX_5p_v2"],             # 3' modes only
    ["--bc_correct", "--bc_rescue", "--mode", "tenX_5p_v3"],
])
def test_argparse_errors(argv, tmp_path, capsys):
    wl = tmp_path / "wl.txt"
    wl.write_text("ACGTACGTACGTACGT\n")
    base = ["-i", "x.fq", "-o", str(tmp_path / "o"), "-b", str(wl)]
    with pytest.raises(SystemExit) as e:
        erb.parse_args(base + (argv if "--mode" in argv else ["--mode", "tenX_v3"] + argv))
    assert e.value.code == 2
    capsys.readouterr()


def test_argparse_accepts_the_flag(tmp_path):
    wl = tmp_path / "wl.txt"
    wl.write_text("ACGTACGTACGTACGT\n")
    base = ["-i", "x.fq", "-o", str(tmp_path / "o"), "-b", str(wl), "--mode", "tenX_v3", "--bc_correct"]
    a = erb.parse_args(base + ["--bc_rescue"])
    assert erb._rescue_kwargs(a, True) == dict(rescued_path=str(tmp_path / "o") + ".rescued.tsv", rescue_max_ed=1, rescue_min_support=2)
    a = erb.parse_args(base + ["--bc_rescue", "--rescue_max_ed", "0", "--rescue_min_support", "5"])
    assert erb._rescue_kwargs(a, True) == dict(rescued_path=str(tmp_path / "o") + ".rescued.tsv", rescue_max_ed=0, rescue_min_support=5)
    assert erb._rescue_kwargs(erb.parse_args(base), True) == {}
