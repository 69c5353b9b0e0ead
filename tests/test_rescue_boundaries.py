"""The boundary cases of the barcode rescue (tests/rescue_boundary_cases.py) on the host: every construction is what its family
claims (rescue.find_polyt_start and rescue.Matcher.near judge), the values said by hand equal the rule's, the set holds what it is
for, the plain restatement equals rescue.py with no knob and every knob moves a record of the family named for it, and the
rule's own strand text is total over bytes.  No GPU.

Not reached by any of this, nor by the GPU tier: the `w >= nw` padding of k_rescue_resolve (the top-k match pads no list that
n_within says is filled, so no public call gets there), and `b + 16 <= L` against `<` (see KNOBS in the cases module)."""
import numpy as np
import pytest

import rescue_boundary_cases as bc
from badger_amd import rescue, synth
from badger_amd.trim import revcomp

NAMES = list(bc.FAMILIES)


def _by_read(recs):
    return {int(r["read"]): bc.fields(r) for r in recs}


@pytest.mark.parametrize("fam", NAMES)
def test_constructions_and_hand_values(fam):
    said = 0
    for B in bc.family(fam):
        want = {s: _by_read(r) for s, r in bc.expected(B).items()}
        m = bc.matcher(B.whitelist)
        assert len(set(B.names)) == len(B.names) == len(B.reads) == len(B.records)
        for window, D, claim in B.near:
            assert {m.wl[i]: d for d, i in m.near(window) if d <= D} == claim, (B.name, window)
        for i, (name, read, hand) in enumerate(zip(B.names, B.reads, B.hand)):
            for s, h in (hand or {}).items():
                got = want[s].get(i)
                if h == bc.ABSENT:
                    assert got is None, (name, s, got)
                    continue
                assert got == h, (name, s, got, h)
                said += 1
                if h["status"] == rescue.RESCUED:
                    # p, b and the window by the judges: the walk on the strand's text, the neighbourhood of s[b : b + 16]
                    t = rescue.strand_text(read, h["strand"])
                    p, b = h["polyT"], h["bc_start"]
                    assert rescue.find_polyt_start(t) == p and b == p - B.U - 16 + h["offset"] and 0 <= b, name
                    assert (h["dist"], h["entry"]) in m.near(t[b:b + 16]) and h["umi"] == t[b + 16:p].encode(), name
                    assert len(h["umi"]) == max(B.U - h["offset"], 0), name
    assert said > 0, fam


def test_no_filler_entry_lies_within_two_of_a_case_window():
    n = 0
    for fam in NAMES:
        for B in bc.family(fam):
            m, filler = bc.matcher(B.whitelist), bc.filler_of(B.whitelist)
            for read in set(B.reads):
                for c in m.candidates(read, B.U):
                    n += 1
                    assert not [i for _, i in m.near(c[4]) if i in filler], (B.name, c)
    assert n > 5000 and len(bc._Main.wl) == bc.N_MAIN and len(bc._W5.wl) == bc.N_W5


def test_the_list_holds_what_it_is_for():
    st = set()
    for fam in NAMES:
        for B in bc.family(fam):
            for r in bc.expected(B).values():
                st |= {int(x) for x in r["status"]}
                # R6: a record that is not `rescued` is the header's empty one
                for x in r[r["status"] != rescue.RESCUED]:
                    f = bc.fields(x)
                    assert f == dict(f, entry=rescue.NONE_IDX, support=0, polyT=-1, bc_start=-1, offset=0, strand=0, umi=b"")
                    assert (f["dist"] == -1) == (f["status"] == rescue.NONE) and f["dist"] >= -1
    assert st == {rescue.NONE, rescue.RESCUED, rescue.AMBIGUOUS, rescue.TRUNCATED}
    # W1: every (U, d, strand) is rescued from its offset; UMIs of 0 .. 16 letters; 16 letters without a zero byte; b + 16 > p
    seen, lens = set(), set()
    for B in bc.family("W1"):
        for r in bc.expected(B)[(1, bc.M)]:
            assert r["status"] == rescue.RESCUED
            seen.add((B.U, int(r["offset"]), int(r["strand"])))
            lens.add(len(bytes(r["umi"])))
            if (B.U, int(r["offset"])) == (14, -2):
                raw = bytes(r["umi"])
                assert len(raw) == 16 and 0 not in raw
            if r["bc_start"] + 16 > r["polyT"]:
                assert (B.U, int(r["offset"])) == (1, 2) and bytes(r["umi"]) == b""
                seen.add("b + 16 > p")
    assert seen == {(U, d, s) for U in range(1, 15) for d in range(-2, 3) for s in (1, -1)} | {"b + 16 > p"}
    assert lens == set(range(17))
    # R2: n_within 8 and 9 both stand at the deciding distance
    m = bc.matcher(bc._Main.wl)
    assert [m.topk(c, 1)[1] for c in (bc.C1, bc.C7, bc.C8, bc.C9)] == [1, 7, 8, 9]
    assert [m.topk(c, 2)[1] for c in (bc.A7, bc.A8, bc.A9)] == [8, 9, 10] and (m.topk(bc.D0, 0)[1], m.topk(bc.D0, 1)[1]) == (1, 10)
    # R1: all 255 pairs of ranges, in every batch of it; every candidate of the ten reports somewhere
    assert len(bc.RANGES) == 16
    who = set()
    for B in bc.family("R1"):
        assert len(B.reads) == len(set(B.reads)) == 255
        who |= {(int(r["offset"]), int(r["strand"])) for r in bc.expected(B)[(1, bc.M)]}
    assert who == set(bc.PREF)
    # W5: eligible lanes that store nothing stand between storing ones
    assert any(h is not None and bc.ABSENT in h.values() for B in bc.family("W5") if "between" in B.name for h in B.hand)
    # the bytes outside ACGTN reach every strand and the UMI text
    w3 = [(n, r) for B in bc.family("W3") for n, r in zip(B.names, B.reads)]
    assert all(any(c in r for _, r in w3) for c in bc.BAD)
    assert any(b"N" in bytes(x["umi"]) for B in bc.family("W3") for x in bc.expected(B)[(1, bc.M)])


@pytest.mark.parametrize("fam", NAMES)
def test_restatement_without_a_knob_equals_the_rule(fam):
    for B in bc.family(fam):
        for s, want in bc.expected(B).items():
            got = bc.restated_batch(B, s)
            assert got == {int(r["read"]): tuple(bc.fields(r)[k] for k in rescue.FIELDS[1:]) for r in want}, (B.name, s)


def _moved(knob, fam):
    """the cases of a family whose expected record a knob moves"""
    out = []
    for B in bc.family(fam):
        for s in B.settings:
            a, b = bc.restated_batch(B, s), bc.restated_batch(B, s, knob)
            out += [(B.names[i], s) for i in sorted(set(a) | set(b)) if a.get(i) != b.get(i)]
    return out


@pytest.mark.parametrize("knob", list(bc.KNOBS))
def test_every_knob_moves_a_record_of_its_family(knob):
    fam = bc.KNOBS[knob]
    moved = _moved(knob, fam)
    print("%s: %s notices, %d records move, first %r" % (knob, fam, len(moved), moved[:1]))
    assert moved, (knob, fam)


def test_the_pipelined_set_stays_eligible_under_the_oracle():
    """what the GPU tier's pipelined test relies on: the extraction finds no usable adapter in these reads (the oracle's records
    say so here): at most 2 % of them may come out with a barcode, and none of R1"""
    from oracle import pyoracle as orc
    groups = bc.pipelined_set()
    assert sorted(groups) == list(range(1, 15))                            # every U of W1; W2's 1, 12, 14; W4 and R1 at 12
    total = lost = stored = n_r1 = 0
    for U, (reads, names, r1) in groups.items():
        bases, off = synth.list_to_reads(reads)
        recs = orc.extract_batch(bases, off, U, threads=4)
        elig = np.array([rescue.eligible(r) for r in recs])
        assert elig[r1].all(), (U, [names[i] for i in np.nonzero(~elig & r1)[0]][:5])
        want = rescue.rescue_batch(bases, off, recs, U, bc._Main.wl, bc._Main.support, matcher=bc.matcher(bc._Main.wl))
        total, lost, stored, n_r1 = total + len(reads), lost + int((~elig).sum()), stored + len(want), n_r1 + int(r1.sum())
    print("pipelined set: %d reads, %d of R1, %d not eligible, %d with a record" % (total, n_r1, lost, stored))
    assert total == 140 + 90 + 16 + 5 * 255 and n_r1 == 5 * 255
    assert lost <= 0.02 * total and stored > 0.9 * total


def test_strand_text_is_total_and_equals_revcomp_on_acgtn():
    rng = np.random.default_rng(4)
    for _ in range(300):
        s = "".join(rng.choice(list("ACGTN"), size=int(rng.integers(0, 120))))
        assert rescue.strand_text(s, 1) == s == revcomp(revcomp(s)) and rescue.strand_text(s, -1) == revcomp(s)
        assert rescue.strand_text(rescue.strand_text(s, -1), -1) == s
    for c in bc.BAD:
        assert rescue.strand_text("AC" + c + "GT", 1) == "ACNGT" and rescue.strand_text("AC" + c + "GT", -1) == "ACNGT"
    every = "".join(chr(c) for c in range(256))
    assert rescue.strand_text(every, 1) == "".join(c if c in "ACGT" else "N" for c in every)
    assert rescue.strand_text(every, -1) == "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(c, "N") for c in reversed(every))
    # the rule runs on such a read and treats the byte as N on both strands
    m = bc.matcher(bc._Main.wl)
    read = bc.pre(6) + bc.E0 + "CGaC" + bc.UMI16[4:12] + bc.TAIL + bc.CDNA
    for strand in (1, -1):
        r = rescue.rescue_read(bc.as_read(read.replace("a", "N"), strand).replace("N", "-"), 12, m, bc._Main.support)
        assert r[7] == rescue.RESCUED and r[6] == strand and r[8] == b"CGNC" + bc.UMI16[4:12].encode()
