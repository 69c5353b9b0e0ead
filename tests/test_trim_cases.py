"""tests/trim_cases.py holds what it is for.  No GPU.

The plain restatement of the 3' rule, trim.trim_reads and trim.trim_batch agree on every field of every 3' case at the three
thresholds; trim5p.trim_reads and trim5p.trim_batch agree on every 5' case; every answer a case carries by construction is the
rule's answer (a strand whose constructed answer the rule does not confirm is a generator error and fails here); no family is
empty and no case is left out; every switch of plain_trim changes the result of a case of the family it belongs to, which is
the proof that the cases can see a kernel that is wrong in that one decision; and the shapes the families promise are there."""
from collections import Counter

import numpy as np
import pytest

import trim_cases as tc
from badger_amd import _native, trim, trim5p

PARAMS_5P = [(10, 2, 16), (12, 2, 16), (12, 0, 8), (10, 4, 25), (12, 1, 20), (10, 3, 12), (1, 2, 16)]   # test_trim5p_gpu.py's, and the shortest UMI
_RULE = {}


def _tuples(a):
    return [tuple(int(a[f][i]) for f in tc.FIELDS) for i in range(len(a))]


def _rule_3p(score):
    if score not in _RULE:
        C = tc.cases_3p()
        _RULE[score] = _tuples(trim.trim_batch(C["bases"], C["off"], C["recs"], score))
    return _RULE[score]


def _strand(C, i):
    return tc.rc(C["reads"][i]) if int(C["recs"]["flags"][i]) & tc.FLAG_REV else C["reads"][i]


def _eligible_3p(C, i):
    r = C["recs"][i]
    return int(r["valid"]) == 1 and int(r["polyT"]) >= 0 and not int(r["flags"]) & tc.FLAG_INCOMPLETE


def test_constants_are_the_rules():
    assert (tc.TSO, tc.WINDOW, tc.XDROP) == (trim.TSO, trim.TSO_WINDOW, trim.TAIL_XDROP)
    assert (tc.TSO5, tc.PRIMER) == (trim5p.TSO5, trim5p.PRIMER)
    assert (tc.EMIT, tc.HAS_TSO, tc.SENSE, tc.ANCHOR, tc.NO_ANCHOR) == (
        trim.TRIM_EMIT, trim.TRIM_TSO, trim.TRIM_SENSE, trim5p.TRIM_ANCHOR, trim5p.TRIM_NO_ANCHOR)
    assert (tc.FLAG_REV, tc.FLAG_INCOMPLETE) == (_native.FLAG_REV, _native.FLAG_INCOMPLETE)
    assert (min(tc.SCORES_3P), max(tc.SCORES_3P)) == trim.TSO_MIN_SCORE_RANGE and (min(tc.SCORES_5P), max(tc.SCORES_5P)) == trim5p.MIN_SCORE_RANGE


@pytest.mark.parametrize("score", tc.SCORES_3P)
def test_three_forms_of_the_3p_rule_agree(score):
    C = tc.cases_3p()
    batch = _rule_3p(score)
    one = _tuples(trim.trim_reads(C["reads"], C["recs"], score))
    for i, name in enumerate(C["names"]):
        plain = tuple(tc.plain_trim_read(C["reads"][i], C["recs"][i], score))
        assert plain == batch[i] == one[i], (name, score, plain, batch[i], one[i])


def test_3p_cases_carry_the_rules_answers_and_every_family():
    C = tc.cases_3p()
    n = len(C["names"])
    assert all(len(C[k]) == n for k in ("family", "reads", "recs", "expect")) and len(C["off"]) == n + 1
    counts = Counter(C["family"])
    print(dict(counts), n)
    assert set(counts) == set(tc.FAMILIES_3P) and all(counts[f] >= 2 for f in tc.FAMILIES_3P)
    # both strands of every name
    names = Counter(C["names"])
    assert all(names[x + " (rev)"] == names[x] for x in names if not x.endswith(" (rev)"))
    assert sum(1 for x in names if x.endswith(" (rev)")) * 2 == len(names)
    rev = (C["recs"]["flags"] & tc.FLAG_REV) != 0
    assert all(x.endswith(" (rev)") == bool(r) for x, r in zip(C["names"], rev))
    with_answer = 0
    for score in tc.SCORES_3P:
        rule = _rule_3p(score)
        for i, exp in enumerate(C["expect"]):
            bad = tc.check_expect(exp, rule[i], len(C["reads"][i]), score)
            assert not bad, (C["names"][i], score, bad, exp, rule[i])
            with_answer += bool(exp)
    assert with_answer > 3 * 0.35 * n
    assert max(len(r) for r in C["reads"]) < 34000 and n < 2500


def test_3p_shapes():
    C = tc.cases_3p()
    rule = _rule_3p(20)
    by = {}
    for i, f in enumerate(C["family"]):
        by.setdefault(f, []).append(i)
    nws, offsets, to_end, tails, tied = set(), set(), set(), set(), Counter()
    for i in range(len(C["names"])):
        if not _eligible_3p(C, i):
            continue
        s, p, tr = _strand(C, i), int(C["recs"]["polyT"][i]), {}
        assert tuple(tc.plain_trim(s, p, 20, trace=tr)) == rule[i]
        nws.add(tr["nw"])
        tied[tr["tied"]] += 1
        if C["family"][i] == "eight-base step":
            if tr["stop_col"] is None:
                to_end.add(len(s) - p)
            else:
                offsets.add((tr["stop_col"] - p) % 8)
                assert s[tr["stop_col"] + 1:tr["stop_col"] + 8] == "T" * 7        # the T behind the stop, in the same step
        if C["family"][i] == "saturation":
            tails.add(rule[i][0] - p)
            assert rule[i][2] == min(rule[i][0] - p, 32767)
    assert nws >= set(range(65)) and max(nws) == 64
    assert offsets == set(range(8)) and to_end >= set(range(18))
    assert tails == {32766, 32767, 32768}
    # the window length family alone covers every window length and both sides of the clip
    wl = {}
    for i in by["window length"]:
        if "behind the tail" not in C["names"][i]:
            continue
        tr = {}
        tc.plain_trim(_strand(C, i), int(C["recs"]["polyT"][i]), 20, trace=tr)
        wl[len(C["reads"][i]) - rule[i][0]] = tr["nw"]
    assert wl == {nb: min(nb, 64) for nb in range(71)}
    # both sides of every threshold, as prefix, suffix and inner piece
    kinds = Counter()
    for i in by["TSO score at the threshold"]:
        what = C["names"][i].split(",")[0]
        kinds[("prefix" if what.startswith("TSO[:") else "suffix" if what.endswith(":]") else "inner", rule[i][3])] += 1
    for k in range(6, 31):
        assert kinds[("prefix", k)] and (kinds[("suffix", k)] or k == 30) and (kinds[("inner", k)] or k >= 29), k
    # the cut in front of, on and behind cdna_start
    where = Counter()
    for i in by["cut against cdna_start"]:
        e = C["expect"][i]
        where[(e["cut"] > e["cdna_start"]) - (e["cut"] < e["cdna_start"])] += 1
    assert min(where[-1], where[0], where[1]) >= 2
    assert tied[(2, 1)] and tied[(1, 2)]                               # rows tied in the end column, in the begin column
    print(sorted(tied.items()))


def _differs(C, idx, **switch):
    """the cases among idx whose result the switch changes, at any threshold"""
    out = []
    for i in idx:
        if not _eligible_3p(C, i):
            continue
        s, p = _strand(C, i), int(C["recs"]["polyT"][i])
        if any(tuple(tc.plain_trim(s, p, score, **switch)) != _rule_3p(score)[i] for score in tc.SCORES_3P):
            out.append(i)
    return out


@pytest.mark.parametrize("switch", sorted(tc.SWITCHES))
def test_every_switch_is_caught_by_its_family(switch):
    C = tc.cases_3p()
    values, family = tc.SWITCHES[switch]
    idx = [i for i, f in enumerate(C["family"]) if f == family]
    for v in values:
        hit = _differs(C, idx, **{switch: v})
        print("%s=%r: %d of %d cases of %r, first %s" % (switch, v, len(hit), len(idx), family, [C["names"][i] for i in hit[:3]]))
        assert hit, (switch, v, family)
        # on both strands
        assert {bool(int(C["recs"]["flags"][i]) & tc.FLAG_REV) for i in hit} == {False, True}


def test_every_tie_case_tells_a_tie_rule_from_its_near_miss():
    C = tc.cases_3p()
    idx = [i for i, f in enumerate(C["family"]) if f == "ties"]
    seen = {sw: set(_differs(C, idx, **{sw: True})) for sw in ("end_last_col", "begin_largest_row", "end_largest_row")}
    print({sw: len(v) for sw, v in seen.items()}, len(idx))
    for i in idx:
        assert any(i in v for v in seen.values()), C["names"][i]
    T = tc.tie_search()
    print("search: %d draws, last column %d, largest begin row %d, largest end row %d" % (
        T["draws"], len(T["last_col"]), len(T["largest_row"]), len(T["end_row"])))
    assert len(T["last_col"]) >= 48 and len(T["largest_row"]) >= 48 and len(T["end_row"]) >= 1
    # the two windows the rule was first checked on
    a = tc.plain_trim("T" * 20 + "CGGACTTGAGATTCGTACTCGGCGTTNCATACCAAGGTACTCTGCGTGATA", 0, 8)
    b = tc.plain_trim("T" * 20 + "CGGACTTGAGATTCGTACTCGGCGTTNCATACCAAGGTACTCTGCGTGATA", 0, 8, end_last_col=True)
    assert (a[1], b[1]) == (29, 50)                                   # cuts 9 and 30 behind the tail
    a = tc.plain_align(tc.TSO, "CCAACGACTCTGCGTTGATACCACTTGGGA")
    b = tc.plain_align(tc.TSO, "CCAACGACTCTGCGTTGATACCACTTGGGA", begin_largest_row=True)
    assert a[6] == 2 and a[2] != b[2]


# ---- the 5' cases -------------------------------------------------------------------------------------------------------
def _walk_stop(s, start, end0):
    """steps the polyA walk takes from end0 - 1 back before it stops, None if it reaches start"""
    score = best = 0
    for k, j in enumerate(range(end0 - 1, start - 1, -1)):
        score += 1 if s[j] == "A" else -2
        best = max(best, score)
        if best - score >= tc.XDROP:
            return k
    return None


@pytest.mark.parametrize("umi_len,max_ed,score", PARAMS_5P)
def test_5p_cases_two_forms_agree_and_carry_the_rules_answers(umi_len, max_ed, score):
    C = tc.cases_5p(umi_len, max_ed)
    n = len(C["names"])
    batch = _tuples(trim5p.trim_batch(C["bases"], C["off"], C["recs"], umi_len, max_ed, score))
    one = _tuples(trim5p.trim_reads(C["reads"], C["recs"], umi_len, max_ed, score))
    counts = Counter(C["family"])
    assert set(counts) == set(tc.FAMILIES_5P) and all(counts[f] >= 2 for f in tc.FAMILIES_5P)
    names = Counter(C["names"])
    assert all(names[x + " (rev)"] == names[x] for x in names if not x.endswith(" (rev)")) and sum(names.values()) == n
    with_answer = 0
    for i, name in enumerate(C["names"]):
        assert batch[i] == one[i], (name, batch[i], one[i])
        bad = tc.check_expect(C["expect"][i], batch[i], len(C["reads"][i]), score, max_ed)
        assert not bad, (name, bad, C["expect"][i], batch[i])
        with_answer += bool(C["expect"][i])
    assert with_answer > 0.8 * n


@pytest.mark.parametrize("umi_len", [10, 12, 1])
def test_5p_shapes(umi_len):
    C = tc.cases_5p(umi_len, 4)
    rule = _tuples(trim5p.trim_batch(C["bases"], C["off"], C["recs"], umi_len, 4, 8))
    recs = C["recs"]
    lens = np.diff(C["off"].astype(np.int64))
    fam = np.array(C["family"])
    # anchor: every distance 0 .. 5 by the rule, above and below every max_ed; a tie of the smallest distance
    ds = Counter(C["expect"][i]["d"] for i in np.nonzero(fam == "anchor distance")[0])
    assert set(range(6)) <= set(ds) and ds[1] >= 2 * 13
    for i in np.nonzero(fam == "anchor ties")[0]:
        s = _strand(C, i)
        ue, us = int(recs["umi_end"][i]), int(recs["umi_start"][i])
        t0 = max(us, ue - 3)
        row = tc._anchor_row(s[t0:min(len(s), ue + 19)])
        assert row.count(min(row)) >= 2 and rule[i][0] == t0 + row.index(min(row)) + 1, C["names"][i]
    clip = {int(lens[i] - recs["umi_end"][i]) for i in np.nonzero(fam == "anchor text clipping")[0]}
    assert clip == set(range(21))
    assert all(int(recs["umi_end"][i]) - 3 < int(recs["umi_start"][i]) for i in range(len(fam))) == (umi_len < 3)
    # records the record rule never leaves, each caught by one condition
    odd = np.nonzero(fam == "records from elsewhere")[0]
    us, ue = recs["umi_start"][odd].astype(np.int64), recs["umi_end"][odd].astype(np.int64)
    assert ((us < 0) & (ue - us == umi_len)).sum() == 2 and ((ue == lens[odd] + 1) & (ue - us == umi_len)).sum() == 2
    assert (ue - us == umi_len + 1).sum() == 2 and (ue - us == umi_len - 1).sum() == 2
    assert all(rule[i] == tc.INELIGIBLE for i in odd)
    # polyA walk: end0 - cdna_start 0 .. 17 to the anchor, the stop at every offset of the step with A behind it
    spans, offsets, tails = set(), set(), set()
    for i in np.nonzero(fam == "polyA walk")[0]:
        s = _strand(C, i)
        start, end0 = rule[i][0], rule[i][1] + rule[i][2]
        k = _walk_stop(s, start, end0)
        if k is None:
            spans.add(end0 - start)
        elif "offset" in C["names"][i]:
            offsets.add(k % 8)
            assert s[end0 - 1 - k - 7:end0 - 1 - k] == "A" * 7
    assert spans >= set(range(18)) and offsets == set(range(8))
    for i in np.nonzero(fam == "saturation")[0]:
        s = _strand(C, i)
        run = len(s) - 25 - rule[i][1]
        tails.add(run)
        assert rule[i][2] == min(run, 32767) and s[rule[i][1]:len(s) - 25] == "A" * run
    assert tails == {32766, 32767, 32768}
    kinds = Counter((C["names"][i].split(",")[0].startswith("PRIMER[:"), rule[i][3]) for i in np.nonzero(fam == "primer threshold")[0])
    assert all(kinds[(True, k)] and kinds[(False, k)] for k in range(6, 25)) and kinds[(True, 25)]
    # the best row of the whole TSO in the masked rows: 30 against 25, and 9 (above the smallest threshold) against 4
    for i in np.nonzero(fam == "masked rows")[0]:
        s = _strand(C, i)
        whole = tc.plain_align(tc.TSO, s[max(rule[i][0], len(s) - 64):])
        assert (whole[0], rule[i][3]) in ((30, 25), (9, 4)) and whole[4] - whole[0] + 1 < 5, C["names"][i]
    cut = np.nonzero(fam == "cut against cdna_start")[0]
    assert all(rule[i][1] == rule[i][0] and rule[i][4] & tc.HAS_TSO and not rule[i][4] & tc.EMIT for i in cut)
