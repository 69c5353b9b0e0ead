"""The consensus rule on the CPU: badger_amd/consensus.py (the checker the device is held against) against the plain full-matrix
form of tests/consensus_cases.py, hand-derived answers for every tie rule, the grouping and election of a tagged file, the two
command lines' argument errors, and what the rule is for: fewer errors than the longest read has."""
import numpy as np
import pytest

import consensus_cases as cc
from badger_amd import consensus as cs


def _checker(group, anchor, pct=20):
    cons, voted, recs = cs.consensus_groups([group], anchor, pct)[0]
    return cons.decode(), voted, recs


@pytest.mark.parametrize("anchor", (cs.ANCHOR_START, cs.ANCHOR_END))
def test_checker_equals_the_plain_matrix(anchor):
    """random groups: related reads, and unrelated sequences of 0 .. 200 bases with N, at a distance bound that accepts some"""
    rng = np.random.default_rng(31 + anchor)
    groups = cc.random_groups(5 + anchor, 40, anchor=anchor)
    groups += [[cc.rand_seq(rng, int(rng.integers(0, 201)), 0.05) for _ in range(int(rng.integers(1, 5)))] for _ in range(40)]
    groups += [["", "ACGT"], ["ACGT", ""], [""], ["N" * 40, "N" * 38], ["ACGT" * 10] * 3]
    for pct in (20, 60):
        got = cs.consensus_groups(groups, anchor, pct)
        for g, (cons, voted, recs) in zip(groups, got):
            assert (cons.decode(), voted, recs) == cc.plain_consensus(g, anchor, pct), (g, pct)


def test_alignment_records_of_random_pairs():
    """the alignment alone, through the record: ed, span and the flag of pairs of 0 .. 200 bases, every one of them"""
    rng = np.random.default_rng(77)
    seen = set()
    for _ in range(150):
        b = cc.rand_seq(rng, int(rng.integers(0, 201)), 0.02)
        m = cc.mutate(rng, b[:int(rng.integers(0, len(b) + 1))], 0.1, 0.1, 0.1) if rng.random() < 0.7 else cc.rand_seq(rng, int(rng.integers(0, 201)))
        a = cc.plain_align(m, b)
        rec = _checker([b, m], cs.ANCHOR_START, 25)[2][1]
        if a is None:
            assert rec == (0, 0, cs.REJ_BAND) and len(m) > len(b) + 32
        else:
            assert rec == (a[0], a[1], cs.ACCEPTED if a[0] * 100 <= 25 * len(m) else cs.REJ_DIST)
        seen.add(rec[2])
    assert seen == {cs.ACCEPTED, cs.REJ_DIST, cs.REJ_BAND}


def test_band_edges():
    for k, ed, flag in ((31, 31, cs.ACCEPTED), (-32, 32, cs.ACCEPTED)):
        b, m = cc.band_pair(k)
        assert _checker([b, m], cs.ANCHOR_START, 40)[2][1] == (ed, len(b) - 10, flag)
    for k in (32, -33):                                   # one diagonal further: only paths full of mismatches are left
        b, m = cc.band_pair(k)
        rec = _checker([b, m], cs.ANCHOR_START, 40)[2][1]
        assert rec[2] == cs.REJ_DIST and rec[0] > abs(k) + 5 and rec == cc.plain_consensus([b, m], cs.ANCHOR_START, 40)[2][1]
    # without a band cell in the last row: Lm = Lb + 33; Lb + 32 still has one
    assert _checker(["ACGT" * 5, "A" * 53], cs.ANCHOR_START, 100)[2][1] == (0, 0, cs.REJ_BAND)
    assert _checker(["ACGT" * 5, "A" * 52], cs.ANCHOR_START, 100)[2][1][2] == cs.ACCEPTED


@pytest.mark.parametrize("case", cc.TIES, ids=[c[0] for c in cc.TIES])
def test_tie_rules(case):
    _, group, anchor, pct, want, voted, recs = case
    for got in (_checker(group, anchor, pct), cc.plain_consensus(group, anchor, pct)):
        assert got[0] == want and got[1] == voted
        assert recs is None or got[2][1:] == recs
        assert got[2][0] == (0, len(group[0]), cs.BACKBONE)


def test_acceptance_boundary():
    """ed * 100 == pct * Lm is accepted, one more is not; 0 accepts only identical, 100 everything the band holds"""
    b, m = "ACGTTGCAAC" * 2, "ACGTTGCAAC" + "ACGTAGCAAC"            # Lm 20, ed 1: 100 == 5 * 20
    assert _checker([b, m], 0, 5)[2][1] == (1, 20, cs.ACCEPTED)
    assert _checker([b, m], 0, 4)[2][1] == (1, 20, cs.REJ_DIST)
    assert _checker([b, m], 0, 0)[2][1][2] == cs.REJ_DIST and _checker([b, b], 0, 0)[2][1] == (0, 20, cs.ACCEPTED)
    assert _checker([b, "T" * 20], 0, 100)[2][1][2] == cs.ACCEPTED
    for bad in (-1, 101):
        with pytest.raises(ValueError):
            cs.consensus_groups([[b]], 0, bad)
    with pytest.raises(ValueError):
        cs.consensus_groups([[b] * 17], 0, 20)
    with pytest.raises(ValueError):
        cs.consensus_groups([[b]], 2, 20)
    assert _checker([b] * 16, 1, 20) == (b, 16, [(0, 20, cs.BACKBONE)] + [(0, 20, cs.ACCEPTED)] * 15)


def test_anchor_start_on_reversed_inputs_is_anchor_end_reversed():
    groups = cc.random_groups(3, 30, anchor=cs.ANCHOR_END)
    end = cs.consensus_groups(groups, cs.ANCHOR_END, 20)
    start = cs.consensus_groups([[s[::-1] for s in g] for g in groups], cs.ANCHOR_START, 20)
    assert [(c[::-1], v, r) for c, v, r in start] == end
    assert any(c.decode() != g[0] for (c, _, _), g in zip(end, groups))


def test_length_limit():
    rng = np.random.default_rng(5)
    long = cc.rand_seq(rng, 9000)
    assert _checker([long, long[:5000], long[:100]], 0, 20) == (long, 1, [(0, 9000, cs.BACKBONE), (0, 0, cs.REJ_LEN), (0, 0, cs.REJ_LEN)])
    b = cc.rand_seq(rng, 8192)
    assert _checker([b, b + "A"], 0, 20)[2][1] == (0, 0, cs.REJ_LEN)
    assert _checker([b, b], 1, 20) == (b, 2, [(0, 8192, cs.BACKBONE), (0, 8192, cs.ACCEPTED)])


# ---- the tagged file: groups, election, text ----
def _fa(recs):
    return "".join(">%s\n%s\n" % ("\t".join(h), s) for h, s in recs).encode()


def _rec(rid, seq, cb="AAAC", ub="GGGT", rn=1, ch=None):
    h = [rid, "CR:Z:x", "UR:Z:y", "ST:A:+"] + (["CB:Z:" + cb] if cb else []) + (["UB:Z:" + ub, "RN:i:%d" % rn] if ub else [])
    return (h + (["CH:Z:" + ch] if ch else []), seq)


def test_grouping_and_election():
    recs = [_rec("r0", "ACGTAC", ub="T"), _rec("r1", "ACGTACGG", ub="G"), _rec("r2", "ACGTACGT", ub="T"), _rec("r3", "ACGTACGT", ub="T"),
            _rec("r4", "ACG", ub=None), _rec("r5", "TTTT", cb="CCCC", ub="T"), _rec("r6", "ACGTACG", ub="G"), _rec("r7", "AC", cb=None, ub=None)]
    heads, seqs, cb, ub = cs.parse_tagged(_fa(recs))
    mols, left = cs.elect(seqs, cb, ub)
    # the file order of the backbones: r1 (molecule G), r2 (molecule T: r2 and r3 are equally long, the earlier wins), r5
    assert mols == [[1, 6], [2, 0, 3], [5]] and left == 2
    assert cs.with_cn(b"r\tCB:Z:A\tUB:Z:C\tRN:i:3", 2) == b"r\tCB:Z:A\tUB:Z:C\tRN:i:3\tCN:i:2"
    assert cs.with_cn(b"r\tCB:Z:A\tUB:Z:C\tRN:i:3\tCH:Z:tso,5,1", 3) == b"r\tCB:Z:A\tUB:Z:C\tRN:i:3\tCN:i:3\tCH:Z:tso,5,1"


def test_seventeen_reads_and_min_reads():
    rng = np.random.default_rng(9)
    truth = cc.rand_seq(rng, 60)
    reads = [cc.mutate(rng, truth) for _ in range(17)]
    reads[4] = truth + "ACGTACGT"                                    # the longest: the backbone
    recs = [_rec("m%d" % i, s, ub="TTTT", rn=17, ch="tso,1,2" if i == 4 else None) for i, s in enumerate(reads)]
    recs += [_rec("p0", "ACGTACGTAA", ub="CC", rn=2), _rec("p1", "ACGTACGTA", ub="CC", rn=2), _rec("q0", "GGGTTT", ub="AA")]
    text = _fa(recs)
    calls = []

    def run(groups, anchor, pct):
        calls.append([list(map(bytes, g)) for g in groups])
        return cs.consensus_groups(groups, anchor, pct)

    out3, counts3 = cs.consensus_text(text, cs.ANCHOR_END, 3, 20, run)
    # the 16th and 17th read: the backbone and the first 15 of the others in file order go, m16 stays out
    sent = calls[0]
    assert len(sent) == 1 and len(sent[0]) == 16
    assert sent[0] == [reads[4].encode()] + [r.encode() for i, r in enumerate(reads) if i not in (4, 16)]
    want = cs.consensus_groups(sent, cs.ANCHOR_END, 20)[0]
    lines = out3.decode().split("\n")
    assert lines[0] == ">" + "\t".join(recs[4][0][:-1]) + "\tCN:i:%d\tCH:Z:tso,1,2" % want[1] and lines[1] == want[0].decode()
    # a molecule below min_reads is its backbone with CN 1; at min_reads 2 the pair votes
    assert lines[2:6] == [">" + "\t".join(recs[17][0]) + "\tCN:i:1", "ACGTACGTAA", ">" + "\t".join(recs[19][0]) + "\tCN:i:1", "GGGTTT"]
    assert counts3["molecules"] == 3 and counts3["voted"] == 1 and counts3["accepted"] + counts3["rej_dist"] == 15 and counts3["no_molecule"] == 0
    out2, counts2 = cs.consensus_text(text, cs.ANCHOR_END, 2, 20, run)
    assert len(calls[1]) == 2 and out2.decode().split("\n")[2].endswith("\tCN:i:2") and counts2["voted"] == 2
    assert out2.decode().split("\n")[4:6] == lines[4:6]


def test_argparse_errors(capsys):
    from badger_amd import badger
    for argv, word in ((["-i", "a", "-o", "b", "--consensus_min_reads", "1"], "at least 2"),
                       (["-i", "a", "-o", "b", "--consensus_max_ed", "101"], "0 .. 100"),
                       (["-i", "a", "-o", "b", "--consensus_max_ed", "-1"], "0 .. 100"),
                       (["-i", "a", "-o", "b", "--anchor", "middle"], "invalid choice"),
                       (["-i", "a"], "required")):
        with pytest.raises(SystemExit):
            cs.parse_args(argv)
        assert word in capsys.readouterr().err, argv
    a = cs.parse_args(["-i", "a", "-o", "b"])
    assert (a.anchor, a.consensus_min_reads, a.consensus_max_ed) == ("end", 3, 20)
    base = ["-r", "reads.fastq", "-d", "tenX_v3"]
    for argv, word in ((["--molecule_consensus", "c.fa"], "needs --tagged_reads and --umi_dedup"),
                       (["--molecule_consensus", "c.fa", "--tagged_reads", "t.fa"], "needs --tagged_reads and --umi_dedup"),
                       (["--molecule_consensus", "c.fa", "--umi_dedup"], "needs --tagged_reads and --umi_dedup"),
                       (["--molecule_consensus", "c.fa", "--tagged_reads", "t.fa", "--umi_dedup", "--molecule_reads"], "leaves nothing to vote"),
                       (["--tagged_reads", "t.fa", "--umi_dedup", "--consensus_min_reads", "4"], "need --molecule_consensus"),
                       (["--molecule_consensus", "c.fa", "--tagged_reads", "t.fa", "--umi_dedup", "--consensus_min_reads", "1"], "at least 2")):
        with pytest.raises(SystemExit):
            badger.parse_args(base + argv)
        assert word in capsys.readouterr().err, argv
    a = badger.parse_args(base + ["--molecule_consensus", "c.fa", "--tagged_reads", "t.fa", "--umi_dedup", "--consensus_max_ed", "10"])
    assert (a.molecule_consensus, a.consensus_min_reads, a.consensus_max_ed) == ("c.fa", 3, 10)
    assert badger.consensus_anchor("tenX_v2") == badger.consensus_anchor("tenX_v3") == cs.ANCHOR_END
    assert badger.consensus_anchor("tenX_5p_v2") == badger.consensus_anchor("tenX_5p_v3") == cs.ANCHOR_START
    assert badger.parse_args(base).molecule_consensus is None


def test_consensus_is_closer_to_the_truth_than_the_backbone():
    """200 molecules of 300 bases, 5 reads each at synth's error rates (3 % substitutions, 2 % insertions, 3 % deletions), the
    members cut by up to a quarter at the end away from the anchor.  Measured here: see DESIGN 4.17."""
    rng = np.random.default_rng(2024)
    truths, groups = [], []
    for _ in range(200):
        t, r = cc.molecule(rng, 300, 5, cs.ANCHOR_END)
        truths.append(t)
        groups.append(cc.elected(r))
    res = cs.consensus_groups(groups, cs.ANCHOR_END, 20)
    backbone = sum(cc.edit_distance(g[0], t) for g, t in zip(groups, truths))
    cons = sum(cc.edit_distance(c.decode(), t) for (c, _, _), t in zip(res, truths))
    rejected = sum(1 for _, _, recs in res for r in recs[1:] if not r[2] & cs.ACCEPTED)
    print("backbone edits %d, consensus edits %d, ratio %.3f, rejected %d of 800" % (backbone, cons, cons / backbone, rejected))
    assert cons < 0.75 * backbone
    assert rejected <= 0.05 * 800
