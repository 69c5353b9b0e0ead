"""k_split_scan's cell ring on the CPU (tests/split_ring_cases.py): the model of the kernel's scheme equals the selection rule at
the kernel's values - on every case wave and on random waves - every boundary a case names by hand is what the rule gives, and
every wrong limit changes the answer of a case family named here."""
import numpy as np
import pytest

import split_ring_cases as rc
from badger_amd import chimera_split as cs


def _lengths_and_hits(wave):
    return [len(s) for s in wave["reads"]], [rc.hits_of(s, wave["max_ed"]) for s in wave["reads"]]


def _noticed(knobs):
    """-> {family: cases whose read the model with these knobs answers differently from the rule}, reads of no case likewise
    under the family 'filler'"""
    seen = {}
    for wave in rc.waves():
        lengths, hits = _lengths_and_hits(wave)
        got = rc.ring_model(lengths, hits, **knobs)
        owner = {c[2]: c for c in wave["cases"]}
        for r, h in enumerate(hits):
            if got[r] != cs.select(h):
                seen.setdefault(owner[r][0] if r in owner else "filler", []).append((wave["label"], owner.get(r)))
    return seen


def test_geometry():
    lengths = [768] * 64
    assert rc.wave_cells(lengths)[:3] == [0, 24, 48] and rc.wave_cells(lengths)[63] == 1512
    assert [rc.place(lengths, B) for B in (256, 512, 768, 1024, 1280)] == [(10, 16), (21, 8), (32, 0), (42, 16), (53, 8)]
    assert [rc.place([256] + lengths[1:], B) for B in rc.BORDERS] == [(11, 8), (22, 0), (43, 8), (54, 0)]
    assert [rc.place([512] + lengths[1:], B) for B in rc.BORDERS] == [(11, 0), (21, 16), (43, 0), (53, 16)]
    mixed = [0, 127, 128, 100, 256, 257, 0]                             # a read shorter than 128 bases has no segment, no cell
    assert rc.wave_cells(mixed) == [0, 0, 0, 8, 8, 16, 32]
    assert rc.place(mixed, 0) == (2, 0) and rc.place(mixed, 8) == (4, 0) and rc.place(mixed, 31) == (5, 15)
    with pytest.raises(AssertionError):
        rc.place(mixed, 32)


def test_the_case_list():
    """how many cases each family holds (a case is left out only where the geometry leaves no place for a mark: fixed numbers),
    and that the waves are what the GPU tier takes them for"""
    assert rc.family_counts() == {"single": 184, "pair": 408, "apart": 228, "chain": 24, "quad": 32, "rank": 12, "columns": 78,
                                  "shape": 65, "zero": 41, "short": 3}
    waves = rc.waves()
    assert all(len(w["reads"]) == 64 for w in waves[:-1]) and len(waves[-1]["reads"]) == 5
    totals = {sum(rc.segments(len(s)) for s in w["reads"]) for w in waves if w["label"][0] == "shape"}
    assert totals == {32, 33, 64, 65}
    for B in rc.BORDERS:                                                # every family stands at every border
        at = {c[0] for w in waves for c in w["cases"] if c[1][0] == B and c[0] in ("single", "pair", "apart", "chain", "quad", "rank")}
        assert at == {"single", "pair", "apart", "chain", "quad", "rank"}, B
    zero = next(w for w in waves if w["label"] == ("zero_segment_reads",))
    assert len(zero["reads"][0]) == 0 and len(zero["reads"][63]) == 100


def test_hand_derived_boundaries_are_the_rule_and_the_model():
    for wave in rc.waves():
        lengths, hits = _lengths_and_hits(wave)
        got = rc.ring_model(lengths, hits)
        for r, h in enumerate(hits):
            want = wave["bounds"].get(r, [])
            assert cs.select(h) == want and got[r] == want, (wave["label"], r, got[r], want)


def test_marks_sit_where_the_cases_say():
    """in wave cells, from the reads' hits: a border case's marks lie within 7 cells of its border; at every border at least 40
    cases hold non-empty cells on both sides of the window's first cell B - 2 (for each of the two leading reads that leave the
    border inside a read: 9 pairs, 9 of the cases 3 cells apart, 2 chains); each of the cells B - 4 .. B - 1 - emptied one window
    late, carried into the next - is non-empty beside a second non-empty cell; the rank reads have boundaries in three
    consecutive windows"""
    across = dict.fromkeys(rc.BORDERS, 0)
    beside = {(B, o): 0 for B in rc.BORDERS for o in (-4, -3, -2, -1)}
    for wave in rc.waves():
        lengths, hits = _lengths_and_hits(wave)
        first = rc.wave_cells(lengths)
        for family, label, r in wave["cases"]:
            B = label[0]
            if family in ("single", "pair", "apart", "chain", "quad"):
                cells = sorted({first[r] + h[1] // rc.CELL for h in hits[r]})
                assert all(abs(c - B) <= 7 for c in cells), (family, label, cells)
                across[B] += cells[0] < B - 2 <= cells[-1]
                for o in (-4, -3, -2, -1):
                    beside[B, o] += len(cells) > 1 and B + o in cells
            if family == "rank":
                windows = {(first[r] + p // rc.CELL + 2) // rc.ROUND_CELLS for p, _, _ in wave["bounds"][r]}
                assert windows == {B // 256 - 1, B // 256, B // 256 + 1} and len(wave["bounds"][r]) == 9
    assert all(v >= 40 for v in across.values()), across
    assert all(v >= 20 for v in beside.values()), beside


# where a border lies on a read's start (a leading read of 512 bases at 256 and 1,024, of 256 bases at 512 and 1,280) no two marks
# of a read lie on either side of it
ON_A_READ_START = {(256, 2), (1024, 2), (512, 1), (1280, 1)}


@pytest.mark.parametrize("name,families", [
    # the last two cells of a window are selected before their right neighbours are scanned: a pair or a chain across the border
    ("window_at_round_start", ("pair", "chain")),
    # cells 256 q - 4 and 256 q - 3 are gone when 256 q - 2 and 256 q - 1 are selected: a better mark there no longer beats them
    ("emptying_two_cells_short", ("pair",)),
    # cell c and cell c + 256 share a slot: marks are lost, or seen again a round later
    ("ring_256", ("single", "pair", "apart", "chain", "quad", "rank", "shape", "zero")),
    # a read's first boundary of a later window takes rank 0 again
    ("rank_reset_each_round", ("rank", "apart")),
])
def test_a_wrong_limit_is_noticed(name, families):
    seen = _noticed(rc.WRONG_KNOBS[name])
    for family in families:
        assert seen.get(family), (name, family, sorted(seen))
        if name != "ring_256":                                          # at every border, behind every leading read
            where = {c[1][:2] for _, c in seen[family]}
            everywhere = {(B, k) for B in rc.BORDERS for k in (0, 1, 2)}
            assert where == (everywhere if family == "rank" else everywhere - ON_A_READ_START), (name, family, where)
    if name != "ring_256":
        assert set(seen) <= {"pair", "chain", "apart", "rank"}, sorted(seen)    # (and nowhere but at a border)


@pytest.mark.parametrize("name", sorted(rc.REDUNDANT_KNOBS))
def test_what_the_model_cannot_tell(name):
    """a ring of 512 and neighbours that are not clipped to the read give every answer of the rule: nothing here tests the
    ring's other half or the clip, and nothing claims to"""
    assert _noticed(rc.REDUNDANT_KNOBS[name]) == {}


def _random_wave(rng):
    lengths = [int(x) for x in rng.choice([0, 100, 130, 256, 700, 768, 1500, 9000], size=64)]
    hits = []
    for L in lengths:
        k = int(rng.integers(0, 61)) if L >= 2 * rc.MARGIN else 0
        pos = rng.integers(rc.MARGIN, L - rc.MARGIN + 1, size=k) if k else []
        hits.append([(int(rng.integers(0, 5)), int(p), int(rng.integers(0, 4))) for p in pos])
    return lengths, hits


def test_random_waves():
    """200 waves of 64 reads with up to 60 hits a read anywhere the margins leave: the model is the rule at the kernel's values,
    with rounds of 8 segments (the scheme does not rest on the round's size), with a ring of 512 and without the clip; the
    wrong limits are noticed in some of the waves (the cases notice them always)"""
    rng = np.random.default_rng(31)
    settings = dict(rc.WRONG_KNOBS, default={}, rounds_of_8_segments=dict(round_segs=8), **rc.REDUNDANT_KNOBS)
    differ = dict.fromkeys(settings, 0)
    for _ in range(200):
        lengths, hits = _random_wave(rng)
        want = [cs.select(h) for h in hits]
        for name, knobs in settings.items():
            differ[name] += rc.ring_model(lengths, hits, **knobs) != want
    assert differ["default"] == differ["rounds_of_8_segments"] == differ["ring_512"] == differ["no_clip"] == 0, differ
    assert all(differ[name] > 0 for name in rc.WRONG_KNOBS), differ
