"""The consensus rule in a band of 128 and 256 diagonals on the CPU: badger_amd/consensus.py with its `band` argument against
the plain full-matrix form of tests/consensus_band_cases.py, the hand-derived tie cases (which no band changes), the band's edges
for both widths, the command lines' --consensus_band, the scoped band of device_groups, and what the wider band is for: members
of long molecules that the band of 64 loses."""
import numpy as np
import pytest

import consensus_band_cases as bc
import consensus_cases as cc
from badger_amd import consensus as cs

WIDE = (128, 256)


def _rec(group, band, pct=40, anchor=cs.ANCHOR_START):
    return cs.consensus_groups([group], anchor, pct, band=band)[0][2][1]


@pytest.mark.parametrize("band", WIDE)
@pytest.mark.parametrize("anchor", (cs.ANCHOR_START, cs.ANCHOR_END))
def test_checker_equals_the_plain_matrix(anchor, band):
    """related reads with many indels (so that paths leave the middle of the band), unrelated sequences of 0 .. 300 bases with N,
    members that the band's last row rejects, at a distance bound that accepts some"""
    rng = np.random.default_rng(131 + anchor + band)
    groups = []
    for _ in range(10):
        t = bc.rand_seq(rng, int(rng.integers(0, 301)), 0.02)
        groups.append([t] + [cc.mutate(rng, t[:int(rng.integers(0, len(t) + 1))], 0.05, 0.1, 0.1) for _ in range(int(rng.integers(1, 4)))])
    groups += [[bc.rand_seq(rng, int(rng.integers(0, 301)), 0.05) for _ in range(int(rng.integers(1, 4)))] for _ in range(10)]
    groups += [["", "ACGT"], ["ACGT", ""], [""], ["N" * 40, "N" * 38], ["ACGT" * 3, "A" * (12 + band // 2), "A" * (13 + band // 2)]]
    if anchor == cs.ANCHOR_END:
        groups = [[s[::-1] for s in g] for g in groups]
    seen = set()
    for pct in (20, 60):
        got = cs.consensus_groups(groups, anchor, pct, band=band)
        for g, (cons, voted, recs) in zip(groups, got):
            assert (cons.decode(), voted, recs) == bc.plain_consensus(g, anchor, pct, band), (g, pct)
            seen |= {r[2] for r in recs}
    assert seen == {cs.BACKBONE, cs.ACCEPTED, cs.REJ_DIST, cs.REJ_BAND}


def test_band_64_is_the_call_without_the_argument():
    groups = cc.random_groups(8, 30) + [list(cc.band_pair(k)) for k in (31, 32, -32, -33)] + [["ACGT" * 5, "A" * 52], ["ACGT" * 5, "A" * 53]]
    for anchor in (cs.ANCHOR_START, cs.ANCHOR_END):
        assert cs.consensus_groups(groups, anchor, 40, band=64) == cs.consensus_groups(groups, anchor, 40)
    # the plain form of this file at 64 is the one of consensus_cases.py
    for g in groups[:6] + groups[-6:]:
        assert bc.plain_consensus(g, cs.ANCHOR_START, 40, 64) == cc.plain_consensus(g, cs.ANCHOR_START, 40)
    assert (cs.BAND_LO, cs.BAND_HI, cs.LANES, cs.BAND_DEFAULT, cs.BANDS) == (-32, 31, 64, 64, (64, 128, 256))
    for bad in (0, 32, 96, 512, "128"):
        with pytest.raises(ValueError):
            cs.consensus_groups(groups[:1], cs.ANCHOR_START, 20, band=bad)


@pytest.mark.parametrize("band", (64,) + WIDE)
@pytest.mark.parametrize("case", cc.TIES, ids=[c[0] for c in cc.TIES])
def test_tie_rules_at_every_band(case, band):
    _, group, anchor, pct, want, voted, recs = case
    cons, n, got = cs.consensus_groups([group], anchor, pct, band=band)[0]
    assert (cons.decode(), n) == (want, voted) and (recs is None or got[1:] == recs)
    assert (cons.decode(), n, got) == bc.plain_consensus(group, anchor, pct, band)


@pytest.mark.parametrize("band", WIDE)
def test_band_edges(band):
    H, n = band // 2, 2 * band
    for k, ed in ((H - 1, H - 1), (-H, H)):
        b, m = bc.band_pair(k, n)
        assert _rec([b, m], band) == (ed, len(b) - 10, cs.ACCEPTED)
        assert bc.plain_align(m, b, band)[:2] == (ed, len(b) - 10)
    for k in (H, -H - 1):                                 # one diagonal further: only paths full of mismatches are left
        b, m = bc.band_pair(k, n)
        rec = _rec([b, m], band)
        assert rec[2] == cs.REJ_DIST and rec[0] > abs(k) + 5 and rec[:2] == bc.plain_align(m, b, band)[:2]
    # without a band cell in the last row: Lm = Lb + H + 1; Lb + H still has one
    assert _rec(["ACGT" * 5, "A" * (20 + H + 1)], band, 100) == (0, 0, cs.REJ_BAND)
    assert _rec(["ACGT" * 5, "A" * (20 + H)], band, 100)[2] == cs.ACCEPTED
    assert bc.plain_align("A" * (20 + H + 1), "ACGT" * 5, band) is None and bc.plain_align("A" * (20 + H), "ACGT" * 5, band) is not None
    # what the band of 64 rejects by its last row and this one aligns
    assert _rec(["ACGT" * 5, "A" * 53], 64, 100) == (0, 0, cs.REJ_BAND) and _rec(["ACGT" * 5, "A" * 53], band, 100)[2] == cs.ACCEPTED


def test_drift_of_40_diagonals():
    """a member 40 diagonals off: outside 64 diagonals, inside 128"""
    for k in (40, -40):
        b, m = bc.band_pair(k, 300)
        assert _rec([b, m], 64, 20)[2] == cs.REJ_DIST
        for band in WIDE:
            assert _rec([b, m], band, 20) == (40, len(b) - 10, cs.ACCEPTED)


# ---- the command lines and the driver ----
def test_argparse(capsys):
    from badger_amd import badger
    for bad in ("0", "32", "96", "512", "wide"):
        with pytest.raises(SystemExit):
            cs.parse_args(["-i", "a", "-o", "b", "--consensus_band", bad])
        assert "64, 128 or 256" in capsys.readouterr().err, bad
    assert cs.parse_args(["-i", "a", "-o", "b"]).consensus_band == 64
    assert [cs.parse_args(["-i", "a", "-o", "b", "--consensus_band", str(w)]).consensus_band for w in cs.BANDS] == [64, 128, 256]
    base = ["-r", "reads.fastq", "-d", "tenX_v3"]
    full = base + ["--molecule_consensus", "c.fa", "--tagged_reads", "t.fa", "--umi_dedup"]
    for argv, word in ((base + ["--tagged_reads", "t.fa", "--umi_dedup", "--consensus_band", "128"], "need --molecule_consensus"),
                       (base + ["--consensus_band", "64"], "need --molecule_consensus"),
                       (full + ["--consensus_band", "100"], "64, 128 or 256")):
        with pytest.raises(SystemExit):
            badger.parse_args(argv)
        assert word in capsys.readouterr().err, argv
    assert badger.parse_args(full).consensus_band == 64 and badger.parse_args(base).consensus_band == 64
    assert badger.parse_args(full + ["--consensus_band", "256"]).consensus_band == 256


class _StubContext:
    """what device_groups asks of a context, answered by the checker"""
    def __init__(self, band=64, fail=False):
        self.consensus_band, self.fail, self.calls = band, fail, []

    def consensus_set_band(self, band):
        self.calls.append(band)
        self.consensus_band = band

    def consensus(self, bases, seq_off, grp_off, anchor, max_ed_pct):
        if self.fail:
            raise RuntimeError("no device")
        from badger_amd import _native
        seqs = [bases[int(seq_off[q]):int(seq_off[q + 1])] for q in range(len(seq_off) - 1)]
        groups = [seqs[int(grp_off[g]):int(grp_off[g + 1])] for g in range(len(grp_off) - 1)]
        res = cs.consensus_groups(groups, anchor, max_ed_pct, band=self.consensus_band)
        out_off = np.concatenate([[0], np.cumsum([2 * len(g[0]) for g in groups])]).astype(np.uint64)
        out = np.zeros(int(out_off[-1]), np.uint8)
        for k, (cons, _, _) in enumerate(res):
            out[int(out_off[k]):int(out_off[k]) + len(cons)] = np.frombuffer(cons, np.uint8)
        recs = np.array([r for _, _, rs in res for r in rs], dtype=_native.CONSENSUS_DTYPE)
        return (out, out_off, np.array([len(c) for c, _, _ in res], np.uint32), np.array([v for _, v, _ in res], np.uint32), recs)


def test_device_groups_sets_the_band_and_restores_it():
    b, m = bc.band_pair(40, 300)
    groups = [[b.encode(), m.encode()]]
    for before in (64, 256):
        ctx = _StubContext(before)
        got = cs.device_groups(ctx, band=128)(groups, cs.ANCHOR_START, 20)
        assert got == cs.consensus_groups(groups, cs.ANCHOR_START, 20, band=128) and got[0][2][1][2] == cs.ACCEPTED
        assert ctx.calls == [128, before] and ctx.consensus_band == before
    ctx = _StubContext(256)
    assert cs.device_groups(ctx)(groups, cs.ANCHOR_START, 20)[0][2][1][2] == cs.REJ_DIST and ctx.calls == [64, 256]
    ctx = _StubContext(128, fail=True)
    with pytest.raises(RuntimeError):
        cs.device_groups(ctx, band=256)(groups, cs.ANCHOR_START, 20)
    assert ctx.calls == [256, 128] and ctx.consensus_band == 128


def test_log_line_names_the_band(caplog):
    import logging
    counts = dict(molecules=3, voted=2, accepted=4, rej_dist=1, rej_band=0, rej_len=0, no_molecule=5)
    with caplog.at_level(logging.INFO, logger="BarcodeGraph"):
        cs.log_counts(dict(counts, band=128), "c.fa")
        cs.log_counts(counts, "c.fa")
    said = [r.getMessage() for r in caplog.records]
    assert said[0].endswith("band of 128 diagonals") and said[1].endswith("band of 64 diagonals")


# ---- what it is for ----
def test_a_band_of_128_keeps_the_members_of_long_molecules():
    """50 molecules of 3,000 bases, 5 reads each at synth's error rates, the members cut by up to a quarter at the end away from
    the anchor, max_ed_pct 20: the checker at 64 and at 128 diagonals.  Measured here (edits to the truth summed over the
    molecules): backbone 11,596; band 64: 8 of 200 members rejected, consensus 3,537 edits; band 128: 0 rejected, 3,241 edits
    (DESIGN 4.17)."""
    rng = np.random.default_rng(7)
    truths, groups = [], []
    for _ in range(50):
        t, r = cc.molecule(rng, 3000, 5, cs.ANCHOR_END)
        truths.append(t)
        groups.append(cc.elected(r))
    rejected, edits = {}, {}
    for band in (64, 128):
        res = cs.consensus_groups(groups, cs.ANCHOR_END, 20, band=band)
        rejected[band] = sum(1 for _, _, recs in res for r in recs[1:] if not r[2] & cs.ACCEPTED)
        edits[band] = sum(cc.edit_distance(c.decode(), t) for (c, _, _), t in zip(res, truths))
    backbone = sum(cc.edit_distance(g[0], t) for g, t in zip(groups, truths))
    print("backbone edits %d; band 64: rejected %d of 200, consensus edits %d (%.3f); band 128: rejected %d of 200, consensus edits %d (%.3f)" % (
        backbone, rejected[64], edits[64], edits[64] / backbone, rejected[128], edits[128], edits[128] / backbone))
    assert rejected[128] <= 2
    assert rejected[128] < rejected[64]
    assert edits[128] <= edits[64]
