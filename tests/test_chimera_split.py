"""The split rule of --chimera_split on the CPU: the three forms of badger_amd/chimera_split.py against each other, the checker
against boundaries derived by hand for every clause of the rule (tests/split_cases.py), the id rule, and what the rule does on
reads of the error model at the default bound."""
import numpy as np
import pytest

import chimera_cases as cc
import split_cases as sc
from badger_amd import chimera, chimera_split as cs, synth
from badger_amd.trim import revcomp

E = cs.MAX_ED_DEFAULT


def _random_texts(seed, count):
    """texts of 0 .. 300 bases (with an N now and then) holding up to three patterns with up to three edits each"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        L = int(rng.integers(0, 301))
        s = cc._rs(rng, L, "ACGTN" if rng.integers(0, 4) == 0 else "ACGT")
        for _ in range(int(rng.integers(0, 4))):
            p = chimera.PATTERNS[int(rng.integers(0, 4))]
            p = cc.mutate(rng, p, int(rng.integers(0, 4)), ("sub", "ins", "del")[int(rng.integers(0, 3))])
            if L > len(p):
                x = int(rng.integers(0, L - len(p)))
                s = s[:x] + p + s[x + len(p):]
        out.append(s)
    return out


def _same(a, b, what):
    assert len(a[0]) == len(b[0]) and (a[0] == b[0]).all(), what
    assert a[1].tobytes() == b[1].tobytes(), what


def test_distances_literal_and_myers():
    for s in _random_texts(3, 12):
        for kind, p in enumerate(chimera.PATTERNS):
            assert cs.end_distances_literal(p, s) == cs.end_distances(p, s), (kind, s)
    # the two directions are one search: T of a text forwards is S of the reversed text with the reversed pattern
    s = _random_texts(4, 3)[2]
    for p in chimera.PATTERNS:
        assert cs.end_distances(p, s) == chimera.start_distances(p[::-1], s[::-1])[::-1]


def test_literal_form_equals_myers_form():
    texts = [t for t in _random_texts(5, 60) if len(t) >= 2 * cs.MARGIN][:14]
    assert len(texts) == 14
    for e in (E, 6):
        _same(cs.split_reads(texts, e, literal=True), cs.split_reads(texts, e), e)


@pytest.mark.parametrize("segment", [None, 256, 64, 7])
def test_batch_form_equals_myers_form(segment):
    texts = _random_texts(6, 150)
    bases, off = synth.list_to_reads(texts)
    got = cs.split_batch_multi(bases, off, [0, E, 6], segment)
    total = 0
    for e, g in zip((0, E, 6), got):
        want = cs.split_reads(texts, e)
        _same(g, want, (segment, e))
        total += len(want[1]) - len(texts)
    assert total > 60                                                   # (the texts do hold boundaries)


@pytest.mark.parametrize("case", sc.cases(), ids=lambda c: "-".join(str(x) for x in c[0]))
def test_hand_derived_cases(case):
    label, read, e, bounds = case
    assert cs.select(cs.read_hits(read, e)) == bounds, label
    pieces = cs.split_read(read, e)
    assert pieces == [(0, 0, 0, 0)] + [(p, d, k, cs.SPLIT_CUT) for p, d, k in bounds]
    bases, off = synth.list_to_reads(["ACGT", read, ""])
    off_out, rows = cs.split_batch(bases, off, e)
    assert rows["read"].tolist() == [0] + [1] * len(pieces) + [2] and rows["start"].tolist() == [0] + [p[0] for p in pieces] + [0]
    assert off_out.tolist() == [0] + [4 + p[0] for p in pieces] + [4 + len(read)] * 2
    assert [(int(r["ed"]), int(r["kind"]), int(r["flags"])) for r in rows[1:-1]] == [p[1:] for p in pieces]


def test_consequences_of_the_rule():
    """boundaries of a read lie at least 65 columns apart, and the pieces tile the read"""
    rng = np.random.default_rng(8)
    reads = [sc.concatemer(rng, int(rng.integers(1, 5)))[0] for _ in range(40)]
    bases, off = synth.list_to_reads(reads)
    off_out, rows = cs.split_batch(bases, off, 6)
    assert off_out[0] == 0 and off_out[-1] == off[-1] and (np.diff(off_out.astype(np.int64)) >= 0).all()
    assert set(off.tolist()) <= set(off_out.tolist()) and len(rows) > len(reads) + 40
    inner = rows["flags"] != 0
    assert (inner == (rows["start"] != 0)).all()
    same = rows["read"][1:] == rows["read"][:-1]
    assert (np.diff(rows["start"].astype(np.int64))[same] >= 65).all()
    assert cs.counts(rows, len(reads)) == (int((np.bincount(rows["read"]) > 1).sum()), int(inner.sum() + (np.bincount(rows["read"]) > 1).sum()))


def test_piece_ids():
    rows = np.zeros(7, dtype=cs.SPLIT_DTYPE)
    rows["read"] = [0, 1, 1, 2, 3, 3, 3]
    ids = ["r0 comment stays", "r1 runid=7 ch=3", "", "a\tb c"]
    assert cs.piece_ids(ids, rows) == ["r0 comment stays", "r1/1 runid=7 ch=3", "r1/2 runid=7 ch=3", "", "a/1\tb c", "a/2\tb c", "a/3\tb c"]
    rows["read"] = [0, 0, 1, 2, 2, 2, 3]
    assert cs.piece_ids(["", "x", "", "y z"], rows) == ["/1", "/2", "x", "/1", "/2", "/3", "y z"]


def test_accuracy_at_the_default_bound():
    """Conditions, not measurements (seed 11; the rates behind the default are in DESIGN §4.18): of 2,000 chimera-free reads of
    the error model at most 2 are split; of 500 pairs of such reads at least 495 have a boundary within 64 columns of the
    junction and at most 5 a boundary anywhere else"""
    wl = synth.make_whitelist(3000)
    b, o = synth.make_reads(2000, wl, seed=11, tso=True)
    reads = synth.reads_to_list(b, o)
    bases, off = synth.list_to_reads(reads)
    _, rows = cs.split_batch(bases, off, E, segment=cs.SEGMENT)
    assert cs.counts(rows, len(reads))[0] <= 2
    pairs, junction = [], []
    for k in range(500):
        x, y = reads[2 * k], reads[2 * k + 1]
        pairs.append(x + (revcomp(y) if k & 1 else y))
        junction.append(len(x))
    bases, off = synth.list_to_reads(pairs)
    _, rows = cs.split_batch(bases, off, E, segment=cs.SEGMENT)
    inner = rows[rows["flags"] != 0]
    near = np.abs(inner["start"].astype(np.int64) - np.array(junction)[inner["read"]]) <= 64
    found = len(set(inner["read"][near].tolist()))
    extra = len(set(inner["read"][~near].tolist()))
    assert found >= 495 and extra <= 5, (found, extra)


@pytest.mark.parametrize("argv,message", [
    (["--split_max_ed", "2"], "--split_max_ed needs --chimera_split"),
    (["--chimera_split", "--split_max_ed", "7"], "7 is outside 0 .. 6"),
    (["--chimera_split", "--split_max_ed", "x"], "not an integer"),
    (["--chimera_split", "--mode", "tenX_5p_v2"], "--chimera_split serves the 3' modes only"),
    (["--chimera_split", "--mode", "tenX_5p_v3", "--split_max_ed", "2"], "--chimera_split serves the 3' modes only"),
    (["--chimera_max_ed", "2"], "--chimera_max_ed needs --chimera_cut"),                  # (as before)
])
def test_stage1_command_line_errors(argv, message, capsys):
    from badger_amd import extract_raw_barcodes as erb
    base = ["-i", "reads.fastq", "-o", "out.tsv"] + ([] if "--mode" in argv else ["--mode", "tenX_v3"])
    with pytest.raises(SystemExit) as e:
        erb.parse_args(base + argv)
    assert e.value.code == 2 and message in capsys.readouterr().err
    a = erb.parse_args(base[:4] + ["--mode", "tenX_v3", "--chimera_split"])
    assert a.chimera_split and a.split_max_ed is None and erb.split_kwargs(a) == {"split_max_ed": cs.MAX_ED_DEFAULT}
    assert erb.split_kwargs(erb.parse_args(base[:4] + ["--mode", "tenX_v3"])) == {}


@pytest.mark.parametrize("argv,message", [
    (["-r", "reads.fastq", "--split_max_ed", "2"], "--split_max_ed needs --chimera_split"),
    (["-r", "reads.fastq", "--chimera_split", "--split_max_ed", "9"], "9 is outside 0 .. 6"),
    (["-r", "stage1.tsv", "--chimera_split"], "--chimera_split needs read input"),
    (["-r", "reads.fastq", "-d", "tenX_5p_v2", "--chimera_split"], "--chimera_split serves the 3' modes only"),
])
def test_stage2_command_line_errors(argv, message, capsys):
    from badger_amd import badger
    base = ["-l", "wl.txt", "-c", "10"] + ([] if "-d" in argv else ["-d", "tenX_v3"])
    with pytest.raises(SystemExit) as e:
        badger.parse_args(base + argv)
    assert e.value.code == 2 and message in capsys.readouterr().err
    a = badger.parse_args(["-l", "wl.txt", "-c", "10", "-d", "tenX_v3", "-r", "reads.fastq", "--chimera_split", "--split_max_ed", "4"])
    assert a.chimera_split and a.split_max_ed == 4
