"""Hand-built reads for the barcode rescue (badger_amd/rescue.py, bdg_rescue_batch): every case is made so that its expected
record follows from the rule alone, without running it.

A case read is  PRE + barcode + UMI + T * 30 + CDNA  (or its reverse complement):
  - PRE and CDNA hold only C and G, the UMI no T: the first window of 16 letters with 12 'T' starts four letters in front of
    the tail, the first "TTT" from there is the tail's, so p = len(PRE) + 16 + len(UMI) exactly;
  - no stretch of 16 letters here holds 12 A, so the reverse complement has no such window: p = -1 on the other strand;
  - with U = 12 the window of offset d starts at len(PRE) + len(UMI) - 12 + d: a UMI of 12 - d letters puts the barcode at d.
The whitelist: 2,000 entries in a shuffled order - the hand entries below, ten neighbours of one centre (the centre itself is
not an entry), the rest random.  build() checks that the entries within distance 1 of a case window are the ones the case names.
"""
import numpy as np

from badger_amd import rescue, synth
from badger_amd.trim import revcomp

U = 12
UMI = "ACGACGACGACG"
TAIL = "T" * 30
CDNA = "GCCGGCGCCGCGGCCGCGCGGCGCCGGCCGCGGCGCGCCG"
PRE = "GCGGCCGCGC"

E_A = "ACGGTCAGCTAGGCTC"        # support 5
E_B = "GTCCGATGGCTCAGTC"        # support 5
E_LOW = "CCGTGACTGGATCGGT"      # support M - 1 = 1
E_M = "TGCCGTAGGCTCTGCA"        # support exactly M = 2
E_P = "ACACACACACACACAC"        # support 5: the same window two letters on
W_AMB = "GGCTAGTCCGATCGTG"      # not an entry; X1, X2 at distance 1
X1 = "GGCAAGTCCGATCGTG"         # support 5
X2 = "GGCTAGTCCGTTCGTG"         # support 5
W_ONE = "CTGGACGTCCTGAGTC"      # not an entry; Y1 (support 5), Y2 (support 1) at distance 1
Y1 = "CTGCACGTCCTGAGTC"
Y2 = "CTGGACGTCCTGTGTC"
CENTRE = "GACCTGAGGACTCAGG"     # not an entry; its ten neighbours (support 5 each) are
E_S = CENTRE[1:] + UMI[0]       # support 5: the centre's window one letter on
NEIGHBOURS = [CENTRE[:k] + ("C" if CENTRE[k] != "C" else "G") + CENTRE[k + 1:] for k in range(10)]
HAND = [E_A, E_B, E_LOW, E_M, E_P, X1, X2, Y1, Y2, E_S] + NEIGHBOURS
M = rescue.MIN_SUPPORT_DEFAULT
_SUPPORT = {E_LOW: M - 1, E_M: M, Y2: 1}

NONE_REC = dict(entry=rescue.NONE_IDX, support=0, polyT=-1, bc_start=-1, offset=0, strand=0, umi=b"")


def whitelist(n=2000, seed=5):
    """(ranks uint32 [n] in a shuffled caller order, support uint32 [n], {sequence: index})"""
    rnd = [synth.rank_to_str(r) for r in synth.make_whitelist(n - len(HAND), seed=77)]
    seqs = HAND + rnd
    order = np.random.default_rng(seed).permutation(n)
    seqs = [seqs[i] for i in order]
    index = {s: i for i, s in enumerate(seqs)}
    assert len(index) == n
    rng = np.random.default_rng(seed + 1)
    support = rng.choice([0, 1, 2, 3, 7, 40], size=n).astype(np.uint32)     # the random entries: every side of M = 1, 2, 3
    for s in HAND:
        support[index[s]] = _SUPPORT.get(s, 5)
    return np.array([synth.str_to_rank(s) for s in seqs], dtype=np.uint32), support, index


def _read(bc, umi=UMI, pre=PRE, cdna=CDNA):
    return pre + bc + umi + TAIL + cdna


def _rec(valid=0, flags=0):
    r = np.zeros(1, dtype=rescue_rec_dtype())[0]
    r["valid"], r["flags"] = valid, flags
    return r


def rescue_rec_dtype():
    from badger_amd import _native
    return _native.REC_DTYPE


def build():
    """-> dict(wl, support, index, cases): cases = [(name, read, record, expected)], expected None (no record: not eligible, or
    no candidate) or the fields of the read's bdg_rescue_rec at max_ed 1, min_support 2 as a dict"""
    wl, support, index = whitelist()
    p0 = len(PRE) + 16 + U

    def rescued(seq, dist, p, b, d, strand, umi):
        return dict(status=rescue.RESCUED, entry=index[seq], support=int(support[index[seq]]), polyT=p, bc_start=b, offset=d,
                    dist=dist, strand=strand, umi=umi.encode())

    def other(status, dist):
        return dict(NONE_REC, status=status, dist=dist)

    cases = []
    add = lambda name, read, exp, rec=None: cases.append((name, read, _rec() if rec is None else rec, exp))   # noqa: E731
    # ---- strands
    add("tail on the forward strand", _read(E_A), rescued(E_A, 0, p0, len(PRE), 0, 1, UMI))
    add("tail on the reverse strand", revcomp(_read(E_B, pre="CCGCG")), rescued(E_B, 0, 5 + 28, 5, 0, -1, UMI))
    two = lambda a, b, pre_b="GGC": _read(a) + revcomp(_read(b, pre=pre_b, cdna=""))                          # noqa: E731
    add("tails on both strands, two entries", two(E_A, E_B), other(rescue.AMBIGUOUS, 0))
    add("tails on both strands, the nearer entry wins", two(E_A, E_B[:7] + "A" + E_B[8:]), rescued(E_A, 0, p0, len(PRE), 0, 1, UMI))
    add("the same entry at d = 0 on both strands: the forward strand reports", two(E_A, E_A), rescued(E_A, 0, p0, len(PRE), 0, 1, UMI))
    add("the same entry on both strands, |d| decides before the strand", _read(E_A, umi=UMI[:11]) + revcomp(_read(E_A, pre="GGC", cdna="")),
        rescued(E_A, 0, 3 + 28, 3, 0, -1, UMI))
    # ---- each offset as the only hit: a UMI of 12 - d letters
    for d in range(-2, 3):
        umi = (UMI + "AC")[:U - d]
        add("offset %+d alone" % d, _read(E_A, umi=umi), rescued(E_A, 0, len(PRE) + 16 + len(umi), len(PRE), d, 1, umi))
    # ---- d = -1 and d = +1 hold the same window (period 2): the negative offset reports
    per = "GCGG" + "CA" * 10 + "GCGACGACGC"                                # s[b0 - 2 : b0 + 18] = (CA)*10, b0 = 6; UMI = s[22:34]
    add("equal |d| on both signs", per + TAIL + CDNA, rescued(E_P, 0, 34, 5, -1, 1, per[21:34]))
    # ---- the read's start
    add("the window runs off the start by one base", _read(E_A[1:], pre=""), other(rescue.NONE, -1))
    add("the window fits the start exactly", _read(E_A, pre=""), rescued(E_A, 0, 28, 0, 0, 1, UMI))
    add("an N in every window", _read(E_A[:5] + "N" + E_A[6:]), None)
    # ---- support
    add("support M - 1", _read(E_LOW), other(rescue.NONE, -1))
    add("support exactly M", _read(E_M), rescued(E_M, 0, p0, len(PRE), 0, 1, UMI))
    add("two entries at the smallest distance", _read(W_AMB), other(rescue.AMBIGUOUS, 1))
    add("the same with one entry below M", _read(W_ONE), rescued(Y1, 1, p0, len(PRE), 0, 1, UMI))
    # ---- a cut list
    # (a UMI that starts with C: the window one letter on is not E_S but one substitution from it, a second pair at distance 1)
    add("ten entries within distance 1 of the window", _read(CENTRE, umi="C" + UMI[1:]), other(rescue.TRUNCATED, 1))
    add("the same window beside a nearer unique entry", _read(CENTRE, umi=UMI[:1] + UMI), rescued(E_S, 0, p0 + 1, len(PRE) + 1, 0, 1, UMI))
    # ---- never eligible, or nothing to look at
    add("a read with a barcode of its own", _read(E_A), None, _rec(valid=1))
    add("a placeholder record", _read(E_A), None, _rec(valid=0, flags=rescue.FLAG_INCOMPLETE))
    add("no polyT", PRE + E_A + UMI + CDNA + CDNA, None)
    add("shorter than 16 bases", "TTTTTTTTTTTTTTT", None)
    add("sixteen T", "T" * 16, None)
    # ---- the construction holds: the windows' neighbourhoods are what the cases say
    m = rescue.Matcher(wl)
    for w, want in ((E_A, {E_A}), (E_B, {E_B}), (E_LOW, {E_LOW}), (E_M, {E_M}), (E_P, {E_P}), (W_AMB, {X1, X2}), (W_ONE, {Y1, Y2}),
                    (CENTRE, set(NEIGHBOURS)), (E_S, {E_S})):
        got = {m.wl[i] for d, i in m.near(w) if d <= 1}
        assert got == want, (w, got)
    return dict(wl=wl, support=support, index=index, cases=cases)


def random_set(n, seed, wl, support):
    """n reads of up to 300 bases for the kernels, with hand-made records: a planted barcode of a supported entry with 0 .. 2
    edits, a UMI of 10 .. 14 letters, a tail of 14 .. 30 T with an error now and then, either strand; some reads random, some
    with an N, some with a record that is valid or a placeholder -> (reads, records)"""
    rng = np.random.default_rng(seed)
    good = np.nonzero(support >= 1)[0]
    acgt = np.array(list("ACGT"))
    rnd = lambda k: "".join(rng.choice(acgt, size=k))                       # noqa: E731
    reads = []
    recs = np.zeros(n, dtype=rescue_rec_dtype())
    for i in range(n):
        kind = rng.integers(0, 10)
        if kind == 0:
            s = rnd(int(rng.integers(1, 300)))
        else:
            bc = list(synth.rank_to_str(wl[good[rng.integers(0, len(good))]]))
            for _ in range(int(rng.integers(0, 3))):
                k, op = int(rng.integers(0, len(bc))), int(rng.integers(0, 3))
                if op == 0:
                    bc[k] = "ACGT"[int(rng.integers(0, 4))]
                elif op == 1:
                    del bc[k]
                else:
                    bc.insert(k, "ACGT"[int(rng.integers(0, 4))])
            tail = ["T"] * int(rng.integers(14, 31))
            if rng.integers(0, 3) == 0:
                tail[int(rng.integers(0, len(tail)))] = "ACG"[int(rng.integers(0, 3))]
            s = rnd(int(rng.integers(0, 30))) + "".join(bc) + rnd(int(rng.integers(10, 15))) + "".join(tail) + rnd(int(rng.integers(0, 200)))
            s = s[:300]
            if kind == 1:
                k = int(rng.integers(0, len(s)))
                s = s[:k] + "N" + s[k + 1:]
            if rng.integers(0, 2):
                s = revcomp(s)
        reads.append(s)
        what = rng.integers(0, 12)
        recs[i]["valid"] = 1 if what == 0 else 0
        recs[i]["flags"] = rescue.FLAG_INCOMPLETE if what == 1 else 0
    return reads, recs
