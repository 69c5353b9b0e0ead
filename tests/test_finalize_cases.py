"""tests/finalize_cases.py holds what it is for, and its restatement of the record rule agrees with the oracle's.

No GPU.  Three things are checked: every generator delivers every class it names (boundary, side, strand) with at least
PER reads, judged from the restatement's traces; every wave-shaped batch has the stated lanes in the stated kinds, again
from the traces alone; and the restatement's record equals pyoracle.extract_read's on every generated read and on
synthetic reads, under both strand rules and both UMI lengths.  The restatement is written from the reference without the
oracle's extract function (it shares the primitives only), so a disagreement is a finding that the reference decides.
No read is left out anywhere."""
from collections import Counter

import numpy as np
import pytest

import finalize_cases as fc
from badger_amd import synth
from oracle import pyoracle as orc

CONFIGS = [(10, fc.RULE_DEFAULT), (12, fc.RULE_DEFAULT), (10, fc.RULE_NO_POLYA), (12, fc.RULE_NO_POLYA)]


def _assert_same(reads, labels, umi_len, rule):
    bases, off = synth.list_to_reads(reads)
    want = orc.extract_batch(bases, off, umi_len, threads=4, rule=rule)
    got = fc.records(reads, umi_len, rule)
    bad = np.nonzero(got != want)[0]
    assert len(got) == len(reads)
    assert not len(bad), "%d reads differ; first: class %s, oracle %s\n%s" % (
        len(bad), labels[bad[0]], want[bad[0]], fc.describe(reads[bad[0]], umi_len, rule))
    for i in range(0, len(reads), 97):          # the per-read entry point, as the issue names it
        assert orc.extract_read(reads[i], umi_len, rule) == got[i]


def test_every_class_is_delivered():
    cases = fc.all_cases()
    counts = Counter(c.cls for c in cases)
    for name, n in counts.items():
        print("%-72s %d" % (name, n))
    assert all(n >= fc.PER for n in counts.values()) and len(counts) > 500
    assert {c.split("/")[0] for c in counts} == set(fc.GENERATORS)
    # both strands of every class that has a strand
    assert all(c[:-1] + ("-" if c[-1] == "+" else "+") in counts for c in counts if c[-1] in "+-")
    assert max(len(c.read) for c in cases) <= 300
    # a class is what the trace says, independently of collect(): the class's strand took the branch its generator is about
    for c in cases:
        if c.cls[-1] in "+-":
            t = fc.read_result(c.read, c.umi_len).traces[c.cls[-1] == "-"]
            assert t["relaxed"] is not None or t["strict"] is not None, c


def test_the_boundaries_have_both_sides():
    """what the class names promise, read back from traces and expected records"""
    by = {}
    for c in fc.all_cases():
        by.setdefault(c.cls, []).append(c)

    def all_of(cls, pred):
        for sg in "+-":
            for c in by["%s/%s" % (cls, sg)]:
                r = fc.read_result(c.read, c.umi_len)
                assert pred(r.results[sg == "-"], r.traces[sg == "-"], r), (cls, sg, fc.describe(c.read, c.umi_len))
    for e in ("", "_indel"):
        all_of("relaxed_leftover/leftover4" + e, lambda res, t, r: res["valid"] and t["search"] == "relaxed" and t["leftover"] == 4)
        all_of("relaxed_leftover/leftover5" + e, lambda res, t, r: not res["valid"] and t["search"] == "none" and t["relaxed"]["leftover"] == 5)
    all_of("relaxed_leftover/leftover4_indel", lambda res, t, r: res["r1"] == t["relaxed"]["ref_end"] + 4)
    for h in range(4):
        for k in range(3):
            all_of("strict_ends/begin%d_leftover%d" % (h, k), lambda res, t, r: res["valid"] == (h <= 1 and k <= 1) and t["need_rev"] == (k <= 1))
    all_of("strict_ends/full_length_begin1", lambda res, t, r: res["valid"] and t["pattern_start"] == 1 and t["pattern_end"] == 21)
    all_of("strict_ends/full_length_begin2", lambda res, t, r: not res["valid"] and t["need_rev"] and t["pattern_end"] == 21)
    all_of("strict_score/score16_none", lambda res, t, r: not res["valid"] and not t["need_rev"])
    all_of("strict_score/score17", lambda res, t, r: res["valid"] and res["score"] == 17)
    all_of("gap16/u12_gap15", lambda res, t, r: not res["valid"] and res["polyT"] != -1 and res["r1"] == -1)
    all_of("gap16/u12_gap16", lambda res, t, r: res["valid"] and res["polyT"] - res["r1"] == 16)
    for u in (10, 12):
        g = 26 + u
        all_of("gap_research/u%d_gap%d" % (u, g), lambda res, t, r: res["valid"] and not t["research"] and res["polyT"] - res["r1"] == g)
        all_of("gap_research/u%d_gap%d_research_fails" % (u, g + 1), lambda res, t, r: res["valid"] and res["polyT"] == -1 and t["umi_fallback"])
        all_of("gap_research/u%d_gap%d_research_finds" % (u, g + 1), lambda res, t, r: res["valid"] and 0 <= res["polyT"] < t["polyT16"])
        found = {at: {fc.read_result(c.read, u).results[0]["polyT"] != -1 for c in by["research_placement/u%d_run5_at%+d/+" % (u, at)]}
                 for at in range(-7, 13)}
        # common.py:17 and :28 on a window of 14: a window of five T is seen at its places 0 to 8, i.e. from 4 before to 4 after
        assert found == {at: {-4 <= at <= 4} for at in range(-7, 13)}, found
        for k in (4, 5, 6, 7):
            all_of("umi_fallback/u%d_found_polyT_span%d" % (u, k), lambda res, t, r: res["umi_end"] - res["umi_start"] == (u if k <= 5 else k + 1))
    for k in range(31):
        all_of("read_end/ends_%d_behind_r1" % k, lambda res, t, r: res["valid"] and bool(r.record["flags"] & fc.FLAG_BC16) == (k >= 16))
    assert any(fc.read_result(c.read, 12).record["umi_end"] > len(c.read) for k in range(31) for c in by["read_end/ends_%d_behind_r1/+" % k])
    for k in range(16):
        all_of("barcode_letters/N_at_%d" % k, lambda res, t, r: r.record["flags"] & 6 == fc.FLAG_BC16 and r.record["bc_rank"] == 0)
    all_of("barcode_letters/all_A", lambda res, t, r: r.record["flags"] & 6 == 6 and r.record["bc_rank"] == 0)
    all_of("barcode_letters/clean", lambda res, t, r: r.record["flags"] & 6 == 6 and r.record["bc_rank"] != 0)


def test_strand_choice_under_both_rules():
    want = {"both_valid_forward_greater": (0, 0), "both_valid_equal": (1, 0), "both_valid_forward_smaller": (1, 0), "forward_only": (0, 0),
            "reverse_only": (1, 1), "neither_polyT_forward": (0, 1), "neither_polyT_reverse": (0, 1), "neither_polyT_both": (0, 1),
            "neither_polyT_none": (0, 1)}
    seen = Counter()
    for c in fc.all_cases():
        if c.cls.startswith("strand_choice/"):
            r = fc.read_result(c.read, 12)
            side = c.cls.split("/")[1]
            assert side == fc.strand_class(r) and (r.chosen, r.chosen_no_polya) == want[side], fc.describe(c.read)
            rec = r.record
            assert bool(rec["flags"] & fc.FLAG_REV) == bool(r.chosen)
            assert int(rec["strand"]) == (0 if rec["polyT"] == -1 else -1 if r.chosen else 1)
            seen[side] += 1
    assert set(seen) == set(want) and min(seen.values()) >= fc.PER


def test_wave_batches_hold_the_stated_lanes():
    names = Counter()
    for b in fc.wave_batches():
        strand = {"+": 0, "-": 1}[b.name[-1]]
        assert len(b.reads) == len(b.labels)
        kinds = []
        for lane, (s, label) in enumerate(zip(b.reads, b.labels)):
            kind, ncol = fc.lane_kind(s, strand)
            want = label.split(":")
            assert kind == want[0] and (len(want) == 1 or ncol == int(want[1])), (b.name, lane, label, kind, ncol)
            kinds.append((kind, ncol))
        waves = [kinds[i:i + 64] for i in range(0, len(kinds), 64)]
        print("%-40s %5d reads, waves: %s" % (b.name, len(b.reads), " ".join(
            "%d/%d/%d" % (sum(k == "rev" for k, _ in w), sum(k == "revN" for k, _ in w), max(n for _, n in w)) for w in waves[:12])))
        names[b.name[:-2]] += 1
        stem = b.name[:-2]
        if stem == "wave_all_rev":
            assert [k for k, _ in waves[1]] == ["rev"] * 64 and all(k == "plain" for w in (waves[0], waves[2]) for k, _ in w)
        if stem.startswith("wave_all_rev_one_N_at_lane_"):
            at = int(stem.rsplit("_", 1)[1])
            assert [k for k, _ in waves[1]] == ["rev"] * at + ["revN"] + ["rev"] * (63 - at)
        if stem == "wave_one_rev_lane":
            assert sum(k != "plain" for k, _ in kinds) == 1 and kinds[17][0] == "rev"
        if stem == "wave_one_plain_lane":
            assert sum(k != "rev" for k, _ in kinds) == 1 and kinds[40][0] == "plain"
        if stem == "wave_one_ncol39_among_ncol0":
            assert sorted(n for _, n in waves[0]) == [0] * 63 + [39]
        if stem == "wave_one_ncol39_among_ncol17":
            assert sorted(n for _, n in waves[0]) == [17] * 63 + [39]
        if stem == "waves_of_one_ncol_each":
            assert [{n for _, n in w} for w in waves] == [{n} for n in range(17, 40)]
            assert {(n + 3) >> 2 for n in range(17, 40)} == {5, 6, 7, 8, 9, 10}          # every word count the pass can run
        if stem == "wave_of_short_reads":
            assert sorted({len(s) for s in b.reads[:64]}) == list(range(16)) and all(k == "plain" for k, _ in waves[0])
            assert all(k == "rev" for k, _ in waves[1])
        if stem.startswith("batch_of_"):
            n = int(stem.rsplit("_", 1)[1])
            assert len(b.reads) == n and all(k == "rev" for k, _ in kinds[-min(n, 20):]) and all(k == "plain" for k, _ in kinds[:-20])
    assert all(v == 2 for v in names.values())
    assert {"batch_of_%d" % n for n in fc.SIZES} <= set(names) and len(names) == 10 + len(fc.SIZES)


@pytest.mark.parametrize("umi_len,rule", CONFIGS)
def test_restatement_equals_oracle_on_every_generated_read(umi_len, rule):
    total = 0
    for b in fc.generator_batches() + fc.wave_batches() + (fc.shuffled_batch(),):
        _assert_same(b.reads, b.labels, umi_len, rule)
        total += len(b.reads)
    assert total >= 2 * len(fc.all_cases())


@pytest.mark.parametrize("umi_len,rule", CONFIGS)
def test_restatement_equals_oracle_on_synthetic_reads(umi_len, rule):
    wl = synth.make_whitelist(1000)
    for n, seed, errs in ((1000, 3, (0.03, 0.02, 0.03)), (500, 4, (0.0, 0.0, 0.0)), (500, 5, (0.10, 0.05, 0.05))):
        bases, off = synth.make_reads(n, wl, seed=seed, p_sub=errs[0], p_ins=errs[1], p_del=errs[2])
        reads = synth.reads_to_list(bases, off)
        _assert_same(reads, ["synth seed %d" % seed] * n, umi_len, rule)
