"""Inputs for the UMI rule at distance 2 (umi_dedup.cell_molecules, k_umi_parent2 of csrc/umi_kernels.hip) with the answers
derived by hand: a pair for every pair of edit kinds at exactly distance 2 and one at distance 3, count ladders across a
distance-2 edge, a UMI with a candidate at distance 1 and one at distance 2, a chain whose middle is absent, 14-letter UMIs a
shift apart, UMIs at the low edge of the window, 1-letter UMIs.  A helper module (imported like umi_cases.py), no test itself:
tests/test_umi_dist2.py holds the checker against the answers, tests/test_umi_dist2_gpu.py the device against the checker.

A hand cell is (name, umi_len, {UMI: reads}, {UMI: root at distance 2})."""
import random

import numpy as np

import umi_cases as uc

A12 = "ACGTTGCAAGTC"
A14 = "ACGTTGCAAGTCGA"
A10 = "ACGTTGCAAG"


def sub(u, p):
    """the letter at p replaced by the next of ACGT"""
    return u[:p] + "ACGT"[("ACGT".index(u[p]) + 1) & 3] + u[p + 1:]


def dele(u, p):
    return u[:p] + u[p + 1:]


def ins(u, p, c):
    return u[:p] + c + u[p:]


# (name, a, b at exactly distance 2 of a, c at exactly distance 3 of a); tests/test_umi_dist2.py checks the distances by the
# plain recurrence
PAIRS = [
    ("sub + sub", A12, sub(sub(A12, 2), 8), sub(sub(sub(A12, 2), 8), 5)),
    ("sub + del", A12, dele(sub(A12, 2), 8), sub(dele(sub(A12, 2), 8), 5)),
    ("sub + ins", A12, ins(sub(A12, 2), 8, "T"), sub(ins(sub(A12, 2), 8, "T"), 5)),
    ("del + del", A12, dele(dele(A12, 8), 2), sub(dele(dele(A12, 8), 2), 4)),
    ("ins + ins", A12, ins(ins(A12, 8, "T"), 2, "A"), sub(ins(ins(A12, 8, "T"), 2, "A"), 6)),
    ("ins + del (a shift)", A12, ins(dele(A12, 2), 8, "C"), sub(ins(dele(A12, 2), 8, "C"), 5)),
]

K_LADDER = (1, 2, 3, 50)


def hand_cells():
    """-> [(name, umi_len, counts, roots at distance 2)]"""
    out = []
    for name, a, b, c in PAIRS:
        out.append((name + ", two edits", 12, {a: 5, b: 1}, {a: a, b: a}))
        out.append((name + ", three edits", 12, {a: 5, c: 1}, {a: a, c: c}))
    # count ladders across a distance-2 edge: a is a candidate from 2k - 1 reads on, and at k reads when its code is smaller
    a, b = A12, sub(sub(A12, 2), 8)                                   # (b's third letter is T, a's G: a comes first)
    for k in K_LADDER:
        out.append(("ladder 2k - 1, k = %d" % k, 12, {a: 2 * k - 1, b: k}, {a: a, b: a}))
        if k > 1:                                                     # (k = 1: a has no read)
            out.append(("ladder 2k - 2, k = %d" % k, 12, {a: 2 * k - 2, b: k}, {a: a, b: b}))
        out.append(("ladder k, k = %d" % k, 12, {a: k, b: k}, {a: a, b: a} if k == 1 else {a: a, b: b}))
        out.append(("ladder k + 1, k = %d" % k, 12, {a: k + 1, b: k}, {a: a, b: a} if k + 1 >= 2 * k - 1 else {a: a, b: b}))
    # a candidate at distance 1 (p1) and one at distance 2 (p2), three edits from each other and too close in count to merge
    b = A12
    p1, p2 = sub(b, 0), sub(sub(b, 5), 9)
    out.append(("the distance-2 candidate ranks higher", 12, {b: 1, p1: 5, p2: 8}, {b: p2, p1: p1, p2: p2}))
    out.append(("the distance-1 candidate ranks higher", 12, {b: 1, p1: 8, p2: 5}, {b: p1, p1: p1, p2: p2}))
    out.append(("equal counts: the smaller code", 12, {b: 1, p1: 5, p2: 5}, {b: min(p1, p2), p1: p1, p2: p2}))
    # a - b - c, one edit each, b absent: a and c are two edits apart
    a, mid = A12, sub(A12, 3)
    c = dele(mid, 9)
    out.append(("a chain with its middle absent", 12, {a: 4, c: 2}, {a: a, c: a}))
    # 14 letters, a shift apart: inserting first would need 15 letters
    a = A14
    out.append(("14 letters, a shift", 12, {a: 3, ins(dele(a, 1), 13, "T"): 1, dele(ins(a, 14, "C"), 0): 2},
                {a: a, ins(dele(a, 1), 13, "T"): a, dele(ins(a, 14, "C"), 0): a}))
    # the low edge of the window (10 of 10 .. 14; 8 of 8 .. 12): deleting first leaves the window
    a = A10
    out.append(("low edge, a shift", 12, {a: 3, ins(dele(a, 1), 8, "T"): 1}, {a: a, ins(dele(a, 1), 8, "T"): a}))
    out.append(("low edge, two insertions up", 12, {a: 1, ins(ins(a, 7, "T"), 2, "A"): 3},
                {a: ins(ins(a, 7, "T"), 2, "A"), ins(ins(a, 7, "T"), 2, "A"): ins(ins(a, 7, "T"), 2, "A")}))
    out.append(("below the window: not usable", 12, {a: 3, dele(a, 1): 9}, {a: a}))
    a = A10[:8]
    out.append(("low edge of umi_len 10", 10, {a: 3, ins(dele(a, 1), 6, "T"): 1}, {a: a, ins(dele(a, 1), 6, "T"): a}))
    # umi_len 3: usable lengths 1 .. 5, the intermediate of two 1-letter UMIs may be empty
    out.append(("one letter each", 3, {"A": 5, "C": 1, "T": 2}, {"A": "A", "C": "A", "T": "A"}))
    out.append(("one letter and two", 3, {"A": 5, "CG": 1}, {"A": "A", "CG": "A"}))
    out.append(("one letter and three", 3, {"A": 5, "CGT": 1}, {"A": "A", "CGT": "CGT"}))
    out.append(("one letter and three that hold it", 3, {"A": 5, "CAT": 1}, {"A": "A", "CAT": "A"}))
    out.append(("two letters down to one", 3, {"AC": 1, "G": 5}, {"AC": "G", "G": "G"}))
    return out


def case_of(name, umi_len, cells_of, seed=1):
    """one cell per {UMI: reads} -> umi_cases.Case"""
    rng = random.Random(seed)
    cells = uc._ranks(rng, len(cells_of))
    reads = []
    for c, counts in zip(cells, cells_of):
        for u, k in counts.items():
            reads += [(c, 1, u)] * k
    rng.shuffle(reads)
    return uc.Case("%s%d" % (name, umi_len), cells, reads)


def hand_case(umi_len):
    """the hand cells of one umi_len as one Case, a cell each"""
    return case_of("by_hand", umi_len, [c for _, ul, c, _ in hand_cells() if ul == umi_len])


# ---- blocks of k_umi_parent2 ------------------------------------------------------------------------------------------------
def slot_of(keys, mask):
    """slot_of of csrc/umi_kernels.hip (the 64-bit mix), on a uint64 array"""
    k = keys.astype(np.uint64)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xff51afd7ed558ccd)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xc4ceb9fe1a85ec53)
    k = k ^ (k >> np.uint64(33))
    return (k & np.uint64(0xFFFFFFFF)).astype(np.uint32) & np.uint32(mask)


def block_pattern(seed=11, umi_len=12):
    """512 reads with different (cell, UMI) keys - a table of 1,024 slots, four blocks of 256 - chosen by their place: slots
    0 .. 255 all taken, 256 .. 511 all empty, one key in 512 .. 767, 255 keys in 768 .. 1023.  Which slots a set of keys fills
    does not depend on the order they arrive in.  Many keys are one or two edits from an earlier one of their cell.
    -> (Case, occupied bool [1024])"""
    from badger_amd import umi_dedup as ud
    rng = random.Random(seed)
    cells = uc._ranks(rng, 3)
    lo, hi = uc.window(umi_len)
    P = 1024
    want = {0: 256, 1: 0, 2: 1, 3: 255}
    used = np.zeros(P, bool)
    have = {0: 0, 1: 0, 2: 0, 3: 0}
    seen, reads = set(), []
    while len(reads) < 512:
        if reads and rng.random() < 0.7:
            c, _, u = reads[rng.randrange(len(reads))]
            for _ in range(rng.choice((1, 2, 2))):
                u = uc._neighbour(rng, u, rng.choice(("sub", "sub", "del", "ins")))
        else:
            c, u = rng.randrange(3), uc._rand(rng, umi_len)
        if not lo <= len(u) <= hi or (c, u) in seen:
            continue
        key = np.array([c << 32 | ud.umi_code(u)], dtype=np.uint64)
        s = home = int(slot_of(key, P - 1)[0])
        while used[s]:
            s = (s + 1) & (P - 1)
        if s < home or have[s >> 8] >= want[s >> 8]:
            continue
        used[s] = True
        have[s >> 8] += 1
        seen.add((c, u))
        reads.append((c, 1, u))
    case = uc.Case("blocks%d" % umi_len, cells, [(cells[c], 1, u) for c, _, u in reads])
    return case, used
