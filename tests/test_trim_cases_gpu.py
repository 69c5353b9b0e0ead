"""k_trim_reads, k_trim_reads_5p and the column scan they share on the strands of tests/trim_cases.py: every decision boundary of
the two rules, on both strands, every field against badger_amd/trim.py and trim5p.py (tests/test_trim_cases.py holds those equal
to a third, plain form of the 3' rule and shows that the cases tell each near miss of the rule from the rule).  A failure names
the case."""
import numpy as np
import pytest

from badger_amd import _native, trim, trim5p

import trim_cases as tc

pytestmark = pytest.mark.gpu

FIELDS = tc.FIELDS
_WANT = {}


def _same(got, want, what, names):
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert not len(bad), (what, f, [names[i] for i in bad[:5]], got[bad[:5]].tolist(), want[bad[:5]].tolist())


def _want_3p(score):
    """the rule over the 3' cases: computed once per threshold, shared, never changed"""
    if score not in _WANT:
        C = tc.cases_3p()
        w = trim.trim_batch(C["bases"], C["off"], C["recs"], score)
        w.setflags(write=False)
        _WANT[score] = w
    return _WANT[score]


def _want_5p(umi_len, max_ed, score):
    key = (umi_len, max_ed, score)
    if key not in _WANT:
        C = tc.cases_5p(umi_len, max_ed)
        w = trim5p.trim_batch(C["bases"], C["off"], C["recs"], umi_len, max_ed, score)
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def _saturated(C, got, family="saturation"):
    """tail_len of the three tails around the limit, by the length in the case's name"""
    out = {}
    for i, (name, fam) in enumerate(zip(C["names"], C["family"])):
        if fam == family:
            out.setdefault(int(name.replace(" (rev)", "").split()[-1]), set()).add(int(got["tail_len"][i]))
    return out


@pytest.fixture()
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


# ---- the 3' layout ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("score", tc.SCORES_3P)
def test_3p_cases_equal_the_rule(ctx, score):
    C = tc.cases_3p()
    got = ctx.trim_batch(C["bases"], C["off"], C["recs"], score)
    _same(got, _want_3p(score), "3' cases, tso_min_score %d" % score, C["names"])
    assert _saturated(C, got) == {32766: {32766}, 32767: {32767}, 32768: {32767}}
    for i, exp in enumerate(C["expect"]):                              # and what the construction itself fixes
        bad = tc.check_expect(exp, tuple(int(got[f][i]) for f in FIELDS), len(C["reads"][i]), score)
        assert not bad, (C["names"][i], bad, exp, got[i])


def test_3p_device_form_over_a_poisoned_output(ctx):
    import torch
    C = tc.cases_3p()
    n, total = len(C["names"]), int(C["off"][-1])
    dev = torch.device("cuda", 0)
    ctx.set_stream(0)
    d_bases = torch.zeros((total + 15) // 16 * 16 + 64, dtype=torch.uint8, device=dev)
    d_bases[:total] = torch.from_numpy(C["bases"].copy()).to(dev)
    d_off = torch.from_numpy(C["off"].astype(np.int64)).to(dev)
    d_recs = torch.from_numpy(np.ascontiguousarray(C["recs"]).view(np.uint8).copy()).to(dev)
    d_out = torch.full((n * 12,), 0xAB, dtype=torch.uint8, device=dev)
    ctx.trim_batch_dev(d_bases, d_off, n, d_recs, 20, d_out)
    torch.cuda.synchronize()
    _same(d_out.cpu().numpy().view(_native.TRIM_DTYPE), _want_3p(20), "device form", C["names"])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_3p_prefixes_of_the_batch(ctx, n):
    """block edges; the last read is eligible: a live lane at the end of a partly filled block"""
    C = tc.cases_3p()
    want = _want_3p(20)[:n]
    assert want["cdna_start"][n - 1] >= 0, C["names"][n - 1]
    got = ctx.trim_batch(C["bases"][:int(C["off"][n])], C["off"][:n + 1], C["recs"][:n], 20)
    _same(got, want, "the first %d cases" % n, C["names"])


def test_3p_results_do_not_depend_on_lane_or_block(ctx):
    C = tc.cases_3p()
    reads = C["reads"][::-1]
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    bases = np.frombuffer("".join(reads).encode(), np.uint8)
    got = ctx.trim_batch(bases, off, np.ascontiguousarray(C["recs"][::-1]), 8)
    _same(got[::-1], _want_3p(8), "the cases in reverse order", C["names"])


# ---- the 5' layout ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_ed", range(trim5p.TSO5_MAX_ED_MAX + 1))
@pytest.mark.parametrize("umi_len", [10, 12, 1])
def test_5p_cases_equal_the_rule(ctx, umi_len, max_ed):
    """(umi_len 1: the smallest the entry takes - the anchor's text starts at the UMI's start, not three bases before its end)"""
    C = tc.cases_5p(umi_len, max_ed)
    ctx.extract_set_layout(_native.LAYOUT_5P)
    ctx.trim_set_5p(umi_len, max_ed)
    for score in tc.SCORES_5P:
        got = ctx.trim_batch(C["bases"], C["off"], C["recs"], score)
        _same(got, _want_5p(umi_len, max_ed, score), "5' cases, umi %d, max_ed %d, tso_min_score %d" % (umi_len, max_ed, score), C["names"])
        assert _saturated(C, got) == {32766: {32766}, 32767: {32767}, 32768: {32767}}
        for i, exp in enumerate(C["expect"]):
            bad = tc.check_expect(exp, tuple(int(got[f][i]) for f in FIELDS), len(C["reads"][i]), score, max_ed)
            assert not bad, (C["names"][i], bad, exp, got[i])


def test_3p_call_behind_5p_calls_on_the_same_context(ctx):
    C5, C3 = tc.cases_5p(10, 2), tc.cases_3p()
    ctx.extract_set_layout(_native.LAYOUT_5P)
    ctx.trim_set_5p(10, 2)
    _same(ctx.trim_batch(C5["bases"], C5["off"], C5["recs"], 16), _want_5p(10, 2, 16), "5' cases", C5["names"])
    ctx.extract_set_layout(_native.LAYOUT_3P)
    for score in (30, 8):                                              # (30: out of the 5' layout's range, in range again)
        _same(ctx.trim_batch(C3["bases"], C3["off"], C3["recs"], score), _want_3p(score), "3' cases behind a 5' batch", C3["names"])
