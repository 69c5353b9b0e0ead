"""--umi_dedup on the CPU: the rule of badger_amd/umi_dedup.py on hand-built cells and against an independent O(n^2) form,
the command line's argument checks, and the native TSV importer's and writer's UMI handling (no GPU needed for those)."""
import random

import numpy as np
import pytest

from badger_amd import umi_dedup as ud

A12 = "ACGTACGTACGT"


def _sub(u, p, c):
    return u[:p] + c + u[p + 1:]


def _molecules(counts, dist=1):
    return ud.cell_molecules(counts, dist)


def test_exact_duplicates_are_one_molecule():
    rows, stats = ud.dedup(["C1"] * 3, [A12] * 3, 12)
    assert rows == [(A12, A12)] * 3
    assert stats == {"C1": [3, 3, 1, 1]}


def test_substitution_merges_by_the_directional_condition():
    b = _sub(A12, 4, "T")
    assert _molecules({A12: 10, b: 1}) == {A12: A12, b: A12}
    assert _molecules({A12: 3, b: 3}) == {A12: A12, b: b}            # 3 < 2 * 3 - 1: two molecules
    assert _molecules({A12: 5, b: 3}) == {A12: A12, b: A12}          # 5 >= 2 * 3 - 1


def test_one_against_one_goes_to_the_smaller_umi():
    a, b = "AAAAAAAAAAAC", "AAAAAAAAAAAG"
    assert _molecules({b: 1, a: 1}) == {a: a, b: a}


def test_chain_is_one_molecule():
    a = "AAAAAAAAAAAA"
    b = _sub(a, 3, "C")
    c = _sub(b, 8, "G")                                               # two edits from a
    m = _molecules({a: 10, b: 4, c: 1})
    assert m == {a: a, b: a, c: a}
    rows, stats = ud.dedup(["X"] * 15, [a] * 10 + [b] * 4 + [c], 12)
    assert stats["X"] == [15, 15, 3, 1]


def test_two_candidate_parents():
    c = "AAAAAAAAAAAA"
    p1, p2 = _sub(c, 2, "C"), _sub(c, 9, "G")                          # p1 and p2 are two edits apart
    assert _molecules({c: 1, p1: 5, p2: 7}) == {c: p2, p1: p1, p2: p2}
    # equal counts: the smaller UMI in the (length, A < C < G < T) order
    assert _molecules({c: 1, p1: 5, p2: 5})[c] == min(p1, p2)
    # a shorter UMI comes first whatever its letters
    short = c[:-1]
    assert _molecules({c: 1, short: 5, p2: 5})[c] == short


def test_insertion_and_deletion_across_lengths():
    u = "ACGTTGCAACGT"
    d = u[:5] + u[6:]                                                 # 11 letters
    i = u[:7] + "T" + u[7:]                                           # 13 letters
    assert _molecules({u: 10, d: 1, i: 1}) == {u: u, d: u, i: u}
    assert ud.within_one(u, d) and ud.within_one(i, u) and not ud.within_one(d, i)


def test_transposition_is_distance_two():
    a, b = "AC" + "A" * 10, "CA" + "A" * 10
    assert not ud.within_one(a, b)
    assert _molecules({a: 10, b: 1}) == {a: a, b: b}


def test_unusable_umis_and_reads_without_a_cell():
    cells = ["C", "C", "C", "C", "C", "*", "C"]
    umis = [A12, A12[:-1] + "N", A12[:9], A12 + "ACG", "", A12, A12 + "AC"]
    rows, stats = ud.dedup(cells, umis, 12)
    # 9 letters and 15 letters are outside 12 +- 2, N is not ACGT, '' is no UMI, '*' has no cell; 14 letters is usable
    assert rows == [(A12, A12), ("*", "*"), ("*", "*"), ("*", "*"), ("*", "*"), ("*", "*"), (A12 + "AC", A12 + "AC")]
    assert stats == {"C": [6, 2, 2, 2]}
    # tenX_v2: umi_len 10, so 8 .. 12 letters
    rows, _ = ud.dedup(["C"] * 3, [A12[:8], A12[:7], A12], 10)
    assert [r[0] for r in rows] == [A12[:8], "*", A12]


def test_umi_dist_zero_keeps_distinct_umis_apart():
    b = _sub(A12, 4, "T")
    rows, stats = ud.dedup(["C"] * 11, [A12] * 10 + [b], 12, umi_dist=0)
    assert rows[-1] == (b, b) and stats["C"] == [11, 11, 2, 2]


def _lev(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def _brute(counts, dist):
    """every pair by its Levenshtein distance, the rule's words taken literally"""
    def above(a, b):
        return counts[a] > counts[b] or (counts[a] == counts[b] and (len(a), a) < (len(b), b))

    us = sorted(counts)
    parent = {}
    for b in us:
        best = None
        for a in us:
            if a != b and _lev(a, b) <= dist and counts[a] >= 2 * counts[b] - 1 and above(a, b):
                if best is None or above(a, best):
                    best = a
        parent[b] = best
    out = {}
    for u in us:
        r = u
        while parent[r] is not None:
            r = parent[r]
        out[u] = r
    return out


def test_rule_equals_brute_force_on_random_cells():
    rng = random.Random(7)
    for trial in range(300):
        L = rng.choice((4, 5, 6))
        base = ["".join(rng.choice("ACGT") for _ in range(L)) for _ in range(rng.randint(1, 4))]
        counts = {}
        for _ in range(rng.randint(1, 40)):
            u = rng.choice(base)
            for _ in range(rng.randint(0, 2)):                        # a few random edits: many neighbours, chains, ties
                k = rng.random()
                p = rng.randrange(len(u))
                if k < 0.5:
                    u = _sub(u, p, rng.choice("ACGT"))
                elif k < 0.75 and len(u) > 3:
                    u = u[:p] + u[p + 1:]
                else:
                    u = u[:p] + rng.choice("ACGT") + u[p:]
            counts[u] = counts.get(u, 0) + rng.choice((1, 1, 1, 2, 3, 7))
        for dist in (0, 1):
            assert ud.cell_molecules(counts, dist) == _brute(counts, dist), (trial, counts, dist)


def test_umi_codes_order_like_the_rule():
    rng = random.Random(3)
    us = ["".join(rng.choice("ACGT") for _ in range(rng.randint(1, 14))) for _ in range(2000)]
    codes = [ud.umi_code(u) for u in us]
    assert [ud.umi_str(c) for c in codes] == us
    assert sorted(us, key=ud.order_key) == [ud.umi_str(c) for c in sorted(codes)]
    assert ud.umi_code("ACGN") == ud.NONE and ud.umi_code("") == ud.NONE and ud.umi_code("A" * 15) == ud.NONE


def test_argument_errors():
    from badger_amd import badger
    with pytest.raises(SystemExit):
        badger.parse_args(["-r", "x.tsv", "-d", "tenX_v3", "--umi_dist", "1"])       # --umi_dist without --umi_dedup
    with pytest.raises(SystemExit):
        badger.parse_args(["-r", "x.tsv", "-d", "tenX_v3", "--umi_dedup", "--umi_dist", "2"])
    a = badger.parse_args(["-r", "x.tsv", "-d", "tenX_v3", "--umi_dedup"])
    assert a.umi_dedup and a.umi_dist == 1
    a = badger.parse_args(["-r", "x.tsv", "-d", "tenX_v3"])
    assert not a.umi_dedup


def _lib():
    from badger_amd import _native
    try:
        _native.load()
    except ImportError as e:
        pytest.skip(str(e))
    return _native


def test_tsv_importer_reads_the_umi_column(tmp_path):
    N = _lib()
    header = "#read_id\tbarcode\tUMI\tBC_score\tvalid_UMI\tstrand\tpolyT_start\tR1_end"
    bc = "ACGTACGTACGTACGT"
    rows = [
        "r1\t%s\tACGTACGTACGT\t0\tFalse\t+\t10\t20" % bc,
        "r2\t%s\t\"ACGTTT\"\t0\tFalse\t+\t10\t20" % bc,           # quoted
        "r3\t%s\tNA\t0\tFalse\t+\t10\t20" % bc,                    # pandas' missing value
        "r4\t%s\t*\t-1\tFalse\t.\t-1\t-1" % "*",
        "r5\t%s" % bc,                                             # the row ends before the UMI column
        "r6\t%s\tACGTNACGTACG\t0\tFalse\t-\t3\t4" % bc,
        "",
        header,                                                    # a repeated header row is skipped
        "r7\t%s\t%s\t0\tFalse\t+\t1\t2" % (bc, "T" * 14),
        "r8\t%s\t%s\t0\tFalse\t+\t1\t2" % (bc, "T" * 15),
        "r9\t%s\t\t0\tFalse\t+\t1\t2" % bc,
    ]
    p = tmp_path / "s1.tsv"
    p.write_text(header + "\n" + "\n".join(rows) + "\n")
    ids, rank, usable, codes = N.import_stage1_tsv_umis(str(p))
    pids, pbcs, pumis = ud.read_stage1_umis(str(p))
    assert ids.to_list() == pids == ["r1", "r2", "r3", "r4", "r5", "r6", "r7", "r8", "r9"]
    assert [int(c) for c in codes] == [ud.umi_code(u) for u in pumis]
    assert [ud.umi_str(int(c)) if c != ud.NONE else None for c in codes] == \
        ["ACGTACGTACGT", "ACGTTT", None, None, None, None, "T" * 14, None, None]
    # the barcodes are what the plain importer reads
    ids2, rank2, usable2 = N.import_stage1_tsv(str(p))
    assert np.array_equal(rank, rank2) and np.array_equal(usable, usable2) and ids2.to_list() == ids.to_list()
    # no UMI column: an error for the UMI importer only
    q = tmp_path / "nou.tsv"
    q.write_text("#read_id\tbarcode\nr1\t%s\n" % bc)
    with pytest.raises(ValueError):
        N.import_stage1_tsv_umis(str(q))
    assert N.import_stage1_tsv(str(q))[0].to_list() == ["r1"]


def test_molecules_writer(tmp_path):
    N = _lib()
    from badger_amd.common import rank
    ids = N.IdStore(["a", "b", "c", "d"])
    bc = "ACGTACGTACGTACGT"
    rk = np.array([rank(bc, 16), 0, rank(bc, 16), rank(bc, 16)], np.uint32)
    has = np.array([1, 0, 1, 1], np.uint8)
    umi = np.array([ud.umi_code(A12), ud.NONE, ud.umi_code("ACGTACGTACGA"), ud.umi_code("ACGTACGTACG")], np.uint32)
    mol = np.array([ud.umi_code(A12), ud.NONE, ud.umi_code(A12), ud.NONE], np.uint32)
    out = str(tmp_path / "m.tsv")
    N.write_molecules(ids, rk, has, umi, mol, out)
    assert open(out).read() == ("readID\tbarcode\tUMI\tmolecule\n"
                                "a\t%s\t%s\t%s\nb\t*\t*\t*\nc\t%s\tACGTACGTACGA\t%s\nd\t%s\t*\t*\n" % (bc, A12, A12, bc, A12, bc))
    assert N.umi_code(A12) == ud.umi_code(A12) and N.umi_code("ACGN") == N.UMI_NONE
