"""The inputs of tests/umi_cases.py hold what they are for: conditions on the inputs, checked from the Python rule alone
(badger_amd/umi_dedup.py), without a GPU.  A generator that stops producing the hard cases fails here, before the device
tests (tests/test_umi_kernels_gpu.py) quietly stop testing them."""
import numpy as np
import pytest

import umi_cases as uc
from badger_amd import umi_dedup as ud

UMI_LENS = (3, 10, 12)


@pytest.mark.parametrize("umi_len", UMI_LENS)
def test_dense_sets_are_hard(umi_len):
    c = uc.case("dense", umi_len)
    h = uc.hardness(c, umi_len)
    print(umi_len, c, {k: v for k, v in h.items() if k not in ("by_len", "refused")}, sorted(h["by_len"].items()), sorted(h["refused"].items()))
    assert h["depth"] >= 4
    for what in ("boundary", "ties", "multi", "cross"):
        assert h[what] >= 1000, (what, h[what])
    # the window's edge and one length outside it
    for L in (umi_len - 2, umi_len + 2):
        assert h["by_len"][L] >= 100, (L, h["by_len"][L])
    for L in (umi_len - 3, umi_len + 3):
        if 0 <= L <= uc.MAX_LEN:
            assert h["refused"][L] >= 100, (L, h["refused"][L])
    assert not [L for L in h["by_len"] if abs(L - umi_len) > 2] and not [L for L in h["refused"] if abs(L - umi_len) <= 2]


@pytest.mark.parametrize("umi_len", UMI_LENS)
def test_runs_hold_every_length_and_merge_across_them(umi_len):
    c = uc.case("runs", umi_len)
    lo, hi = uc.window(umi_len)
    texts = set(c.umi_text)
    for L in range(max(1, lo - 1), min(hi + 1, uc.MAX_LEN + 1) + 1):
        assert "A" * L in texts and "T" * L in texts
        if L >= 3:
            assert any(t == "A" * i + "C" * (L - i) for t in texts for i in range(1, L))
            assert any(len(t) == L and t[0] == t[-1] == "A" and "C" in t for t in texts)
    h = uc.hardness(c, umi_len)
    assert h["cross"] >= 50 and h["multi"] >= 20 and h["depth"] >= 3
    # the homopolymers of one letter share a cell, one deletion from the next: every usable length is there to merge
    rows, _ = ud.dedup(c.cell_text, c.umi_text, umi_len, 1)
    homo = {u for (u, m) in rows if u != "*" and set(u) == {"A"}}
    assert {len(u) for u in homo} == set(range(lo, hi + 1))
    assert len({m for (u, m) in rows if u in homo}) < len(homo)


@pytest.mark.parametrize("umi_len", UMI_LENS)
def test_ladders_hold_every_count_pair(umi_len):
    c = uc.case("ladders", umi_len)
    lo, hi = uc.window(umi_len)
    per_cell = {}
    for cell, u in zip(c.cell_text, c.umi_text):
        per_cell.setdefault(cell, {}).setdefault(u, 0)
        per_cell[cell][u] += 1
    seen, stars = set(), {"one_length": 0, "lengths": 0}
    for counts in per_cell.values():
        assert all(ud.usable(u, umi_len) for u in counts)
        if len(counts) == 2:
            a, b = counts
            assert ud.within_one(a, b)
            seen.add(tuple(sorted([(len(a), counts[a]), (len(b), counts[b])])))
        elif len(counts) >= 3:
            child = min(counts, key=lambda u: (counts[u], [ud.within_one(u, v) for v in counts if v != u].count(False)))
            parents = [u for u in counts if u != child]
            if all(ud.within_one(child, p) for p in parents) and len({counts[p] for p in parents}) == 1:
                stars["one_length" if len({len(p) for p in parents}) == 1 else "lengths"] += 1
    for L in range(lo, hi + 1):
        for kind in ("sub", "del", "ins"):
            if (kind == "del" and L - 1 < lo) or (kind == "ins" and L + 1 > hi):
                continue
            Lb = L + {"sub": 0, "del": -1, "ins": 1}[kind]
            for k in (1, 2, 3, 50):
                for m in (2 * k - 1, 2 * k - 2, k, k + 1):
                    if m:                                             # (a pair with lengths and counts (L, m), (Lb, k) has a cell)
                        assert tuple(sorted([(L, m), (Lb, k)])) in seen, (L, kind, k, m)
    assert stars["one_length"] >= hi - lo and stars["lengths"] >= hi - lo
    h = uc.hardness(c, umi_len)
    assert h["boundary"] >= 50 and h["ties"] >= 20 and h["multi"] >= 20 and h["cross"] >= 50


@pytest.mark.parametrize("umi_len", UMI_LENS)
@pytest.mark.parametrize("n_cells", (1, 2, 3000))
def test_cell_lists(umi_len, n_cells):
    c = uc.case("cells%d" % n_cells, umi_len)
    assert len(c.cells) == n_cells and (np.diff(c.cells.astype(np.int64)) > 0).all()
    inside = set(c.cells.tolist())
    outside = [i for i in range(c.n) if int(c.rank[i]) not in inside]
    assert len(outside) >= 6 and all(c.cell_text[i] == "*" for i in outside) and all(c.has[i] for i in outside)
    no_cell = [i for i in range(c.n) if not c.has[i]]
    assert no_cell and all(int(c.rank[i]) in inside and c.umi[i] != ud.NONE and c.cell_text[i] == "*" for i in no_cell)
    _, counts = uc.rule(c, umi_len, 1)
    assert counts[0, 3] >= 1 and counts[-1, 3] >= 1                  # the first and the last ordinal hold molecules
    if n_cells >= 3:
        assert c.cells[0] == 0 and c.cells[-1] == 0xFFFFFFFF
        assert (counts[c.empty_cell] == 0).all() and counts[c.empty_cell - 1, 0] > 0
        assert min(c.rank[outside]) < c.cells[1] and max(c.rank[outside]) > c.cells[-2]
    else:
        assert min(c.rank[outside]) < c.cells[0] and max(c.rank[outside]) > c.cells[-1]
    if n_cells >= 2:
        # the same UMIs in several cells, and no cell's molecule count is the sum's
        rows, _ = ud.dedup(c.cell_text, c.umi_text, umi_len, 1)
        by_umi = {}
        for cell, (u, _) in zip(c.cell_text, rows):
            if u != "*":
                by_umi.setdefault(u, set()).add(cell)
        assert max(len(v) for v in by_umi.values()) >= 2


@pytest.mark.parametrize("umi_len", UMI_LENS)
def test_hot_cell_and_codes(umi_len):
    c = uc.case("hot", umi_len)
    _, counts = uc.rule(c, umi_len, 1)
    assert counts[2, 0] >= 20000 and (counts[[0, 1, 3, 4], 0] < 100).all() and (counts[:, 3] >= 1).all()
    c = uc.case("codes", umi_len)
    lo, hi = uc.window(umi_len)
    h = uc.hardness(c, umi_len)
    lens_refused = {len(ud.umi_str(int(x))) for x, cell, u in zip(c.umi, c.cell_text, c.umi_text) if x != ud.NONE and not ud.usable(u, umi_len)}
    for L in (umi_len - 3, umi_len + 3, 1, uc.MAX_LEN):
        if 1 <= L <= uc.MAX_LEN and not lo <= L <= hi:
            assert L in lens_refused, (L, lens_refused)
    none = [u for u, x in zip(c.umi_text, c.umi) if x == ud.NONE]
    assert "" in none and any(len(u) == 15 for u in none) and any("N" in u for u in none) and any(u.islower() for u in none)
    # a refused text has more reads than any usable UMI and is one edit from one: let in, it would be its parent
    assert h["pairs"] >= 6 and h["molecules"] >= h["pairs"] - 1
    mol, counts = uc.rule(c, umi_len, 1)
    assert (mol[c.umi == ud.NONE] == ud.NONE).all() and (counts[:, 0] > counts[:, 1]).all()


def test_distinct_keys_and_shuffles():
    for n in (0, 1, 2, 511, 1025):
        c = uc.distinct_keys(12, n, seed=n)
        assert c.n == n and len(set(zip(c.rank.tolist(), c.umi.tolist()))) == n
        assert all(ud.usable(u, 12) for u in c.umi_text) and c.has.all()
    c = uc.distinct_keys(12, 1025, seed=1025)
    mol, counts = uc.rule(c, 12, 1)
    assert counts[:, 2].sum() == 1025 and 100 < counts[:, 3].sum() < 1000
    s, perm = c.shuffled(3)
    mol2, counts2 = uc.rule(s, 12, 1)
    assert (mol2 == mol[perm]).all() and (counts2 == counts).all() and not (perm == np.arange(c.n)).all()


@pytest.mark.parametrize("n", uc.WAVE_SIZES)
def test_wave_shapes_hold_what_they_claim(n):
    waves = [range(a, min(a + uc.WAVE, n)) for a in range(0, n, uc.WAVE)]
    keys = {s: uc.wave_keys(s, n) for s in uc.WAVE_SHAPES}
    assert all(len(k) == n for k in keys.values())
    per_wave = {s: [sorted({k[i] for i in w if k[i] is not None}) for w in waves] for s, k in keys.items()}
    assert all(len(d) == 1 for d in per_wave["same"]) and len(set(keys["same"])) == 1
    assert all(len(d) == len(w) for d, w in zip(per_wave["distinct"], waves)) and len(set(keys["distinct"])) == n
    assert all(len(d) == min(2, len(w)) for d, w in zip(per_wave["alternate"], waves))
    assert all(a != b for a, b in zip(keys["alternate"], keys["alternate"][1:]))
    assert set(keys["none"]) == {None}
    # ends: a key on lanes 0 and 63 and nowhere else; the two lanes share it in an even wave and differ in an odd one
    for w, lanes in enumerate(waves):
        held = [i - lanes[0] for i in lanes if keys["ends"][i] is not None]
        assert held == [l for l in (0, 63) if l < len(lanes)]
        if len(lanes) == uc.WAVE:
            assert (keys["ends"][lanes[0]] == keys["ends"][lanes[63]]) == (w % 2 == 0)
    assert len({k for k in keys["ends"] if k is not None}) == sum(len(d) for d in per_wave["ends"])   # (no key in two waves)
    # straddle: one key; its holders are the last lanes of wave 0 - none of them lane 0 in a full wave - and the first of wave 1
    held = [i for i in range(n) if keys["straddle"][i] is not None]
    assert len({keys["straddle"][i] for i in held}) == 1
    assert held == list(range(max(0, min(n, uc.WAVE) - 3), min(n, uc.WAVE + 3)))
    if n > uc.WAVE:
        assert held[0] == 61 and held[-1] == min(n, 67) - 1 and 64 in held
    # as reads: equal keys are equal (cell, UMI) pairs and different keys different ones; a lane without a key takes no part
    for shape in uc.WAVE_SHAPES:
        for absent in ("cell", "umi"):
            c = uc.wave_case(shape, n, absent)
            pairs = {}
            for i, k in enumerate(keys[shape]):
                takes_part = c.cell_text[i] != "*" and ud.usable(c.umi_text[i], 12)
                assert takes_part == (k is not None), (shape, absent, i)
                if k is None:
                    assert (c.cell_text[i] == "*") == (absent == "cell") and (c.umi[i] != ud.NONE or absent == "umi")
                else:
                    assert pairs.setdefault(k, (c.cell_text[i], c.umi_text[i])) == (c.cell_text[i], c.umi_text[i])
            assert len(set(pairs.values())) == len(pairs)
