"""Inputs of the consensus tests (fixed seeds), and the rule once more in the plainest form: a full matrix with the band as a
mask, one Python loop per cell, the votes as lists.  test_consensus.py holds badger_amd/consensus.py against it; the device tests
use the generators."""
import numpy as np

from badger_amd import consensus as cs

INF = 1 << 30
ACGT = "ACGT"


def code(c):
    return ACGT.find(c) if c in ACGT else 4


def plain_align(M, B):
    """strings in anchor-first order -> (ed, span, steps) or None without a band cell in the last row; steps from the end:
    ('d', i, j) / ('v', i, j) / ('h', i, j) leaving cell (i, j)"""
    Lm, Lb = len(M), len(B)
    D = [[INF] * (Lb + 1) for _ in range(Lm + 1)]
    for i in range(Lm + 1):
        for j in range(Lb + 1):
            if not -32 <= j - i <= 31:
                continue
            if i == 0 and j == 0:
                D[i][j] = 0
                continue
            best = INF
            if i and j and D[i - 1][j - 1] < INF:
                best = min(best, D[i - 1][j - 1] + (0 if M[i - 1] == B[j - 1] and M[i - 1] in ACGT else 1))
            if i and D[i - 1][j] < INF:
                best = min(best, D[i - 1][j] + 1)
            if j and D[i][j - 1] < INF:
                best = min(best, D[i][j - 1] + 1)
            D[i][j] = best
    ed = min(D[Lm])
    if ed >= INF:
        return None
    span = D[Lm].index(ed)
    i, j, steps = Lm, span, []
    while i or j:
        if i and j and D[i - 1][j - 1] < INF and D[i - 1][j - 1] + (0 if M[i - 1] == B[j - 1] and M[i - 1] in ACGT else 1) == D[i][j]:
            steps.append(("d", i, j)); i -= 1; j -= 1
        elif i and D[i - 1][j] < INF and D[i - 1][j] + 1 == D[i][j]:
            steps.append(("v", i, j)); i -= 1
        else:
            steps.append(("h", i, j)); j -= 1
    return ed, span, steps


def plain_consensus(group, anchor, max_ed_pct=20):
    """one group of strings -> (consensus str, n_voted, records)"""
    g = [s[::-1] for s in group] if anchor == cs.ANCHOR_END else list(group)
    B = g[0]
    Lb = len(B)
    recs = [(0, Lb, cs.BACKBONE)]
    base = [[0] * 4 for _ in range(Lb)]
    dele, cov, ins_n = [0] * Lb, [1] * Lb, [0] * Lb
    ins_base = [[0] * 4 for _ in range(Lb)]
    for j, c in enumerate(B):
        if code(c) < 4:
            base[j][code(c)] += 1
    voted = 1
    for M in g[1:]:
        if Lb > cs.MAX_LEN or len(M) > cs.MAX_LEN:
            recs.append((0, 0, cs.REJ_LEN)); continue
        a = plain_align(M, B)
        if a is None:
            recs.append((0, 0, cs.REJ_BAND)); continue
        ed, span, steps = a
        if ed * 100 > max_ed_pct * len(M):
            recs.append((ed, span, cs.REJ_DIST)); continue
        recs.append((ed, span, cs.ACCEPTED))
        voted += 1
        for j in range(span):
            cov[j] += 1
        runs = {}
        for kind, i, j in steps:
            if kind == "d" and code(M[i - 1]) < 4:
                base[j - 1][code(M[i - 1])] += 1
            elif kind == "h":
                dele[j - 1] += 1
            elif kind == "v":
                runs[j] = max(runs.get(j, 0), i)          # the run's last base anchor-first: its largest i
        for j, i in runs.items():
            if j < Lb:
                ins_n[j] += 1
                if code(M[i - 1]) < 4:
                    ins_base[j][code(M[i - 1])] += 1
    if Lb > cs.MAX_LEN:
        return group[0], 1, recs
    out = []
    for j in range(Lb):
        if 2 * ins_n[j] > cov[j] and max(ins_base[j]) > 0:
            out.append(ACGT[ins_base[j].index(max(ins_base[j]))])
        if 2 * dele[j] > cov[j]:
            continue
        top = max(base[j])
        if top == 0:
            out.append(B[j])
        elif code(B[j]) < 4 and base[j][code(B[j])] == top:
            out.append(B[j])
        else:
            out.append(ACGT[base[j].index(top)])
    s = "".join(out)
    return (s[::-1] if anchor == cs.ANCHOR_END else s), voted, recs


# ---- generators ----
def rand_seq(rng, n, n_rate=0.0):
    s = rng.choice(list("ACGT"), size=n)
    if n_rate:
        s = np.where(rng.random(n) < n_rate, "N", s)
    return "".join(s.tolist())


def mutate(rng, s, sub=0.03, ins=0.02, dele=0.03):
    """synth's error rates by default"""
    out = []
    for c in s:
        r = rng.random()
        if r < dele:
            continue
        if r < dele + sub:
            c = "ACGT"[(ACGT.find(c) + int(rng.integers(1, 4))) % 4] if c in ACGT else "A"
        out.append(c)
        if rng.random() < ins:
            out.append("ACGT"[int(rng.integers(0, 4))])
    return "".join(out)


def molecule(rng, length, reads, anchor, truncate=0.25):
    """reads of one molecule: the truth mutated; every read but the first has the end away from the anchor cut by up to
    `truncate` of the length -> (truth, reads)"""
    truth = rand_seq(rng, length)
    out = []
    for k in range(reads):
        cut = int(rng.integers(0, int(length * truncate) + 1)) if k else 0
        t = truth[cut:] if anchor == cs.ANCHOR_END else truth[:length - cut]
        out.append(mutate(rng, t))
    return truth, out


def elected(reads):
    """the group the driver makes of a molecule's reads: the longest first (the earliest at a tie), the others in order"""
    b = max(range(len(reads)), key=lambda i: (len(reads[i]), -i))
    return [reads[b]] + [r for i, r in enumerate(reads) if i != b]


def edit_distance(a, b):
    prev = np.arange(len(b) + 1)
    bb = np.frombuffer(b.encode(), dtype=np.uint8)
    for i, c in enumerate(a.encode(), 1):
        cur = np.minimum(prev[1:] + 1, prev[:-1] + (bb != c))
        cur = np.concatenate([[i], cur])
        cur = np.minimum.accumulate(cur - np.arange(len(cur))) + np.arange(len(cur))
        prev = cur
    return int(prev[-1])


def random_groups(seed, n_groups, reads=(3, 6), length=(40, 120), anchor=cs.ANCHOR_END):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_groups):
        _, r = molecule(rng, int(rng.integers(length[0], length[1] + 1)), int(rng.integers(reads[0], reads[1] + 1)), anchor)
        out.append(elected(r))
    return out


# band-edge pairs in anchor-first order (use with ANCHOR_START), over a random text so that no shifted path is cheap.
# k >= 0: the member is the text without its first k bases, so its only cheap path deletes k backbone bases and then runs on the
# diagonal j - i = k.  k < 0: the member has |k| bases of its own in front, the path inserts them and runs on j - i = k.
# The backbone goes on for `tail` bases behind the member's end, so that the last row always has band cells.
def band_pair(k, n=80, tail=10):
    text = rand_seq(np.random.default_rng(4242), n + abs(k) + tail)
    if k >= 0:
        return text, text[k:k + n]                          # (backbone, member)
    return text[-k:], text[:n - k]


# hand-derived known answers for the tie rules: (name, group, anchor, max_ed_pct, consensus, n_voted, member records or None)
TIES = [
    # the end column: the member ACG against ACGACG reaches distance 0 at j = 3 and nowhere else; AC + ACAC: ed 0 at j = 2 first
    ("end column smallest j", ["ACAC", "AC"], 0, 20, "ACAC", 2, [(0, 2, cs.ACCEPTED)]),
    # the member AG ends at the smallest j of its least row value: D[2][1] = D[2][2] = D[2][3] = 1, so span 1; from (2, 1) the
    # diagonal (G on A from D[1][0] = 1) gives 2, the vertical step from D[1][1] = 0 gives 1: G is a run in column 1, which the
    # member does not cover (cov[1] = 1, the backbone alone) - 2 * 1 > 1 and the G is emitted in front of position 1
    ("a trailing run votes in the column behind the span", ["AAG", "AG"], 0, 100, "AGAG", 2, [(1, 1, cs.ACCEPTED)]),
    # traceback order: ACGT on AACGT comes down the diagonal to (1, 2), where the diagonal (A on A from D[0][1] = 1) and the
    # horizontal step (from D[1][1] = 0) both give 1: the diagonal goes first, so the member votes A at position 1 and the
    # deletion at position 0.  With two members saying G at position 1 that is A 2 : G 2, the backbone's A wins; the other
    # order would leave A 1 : G 2
    ("traceback takes the diagonal first", ["AACGT", "ACGT", "AGCGT", "AGCGT"], 0, 30, "AACGT", 4, [(1, 5, cs.ACCEPTED)] * 3),
    # the backbone wins a base tie: one member says C where the backbone says A: 1 : 1
    ("backbone wins a tie", ["GATTACA", "GCTTACA"], 0, 20, "GATTACA", 2, [(1, 7, cs.ACCEPTED)]),
    # two members against the backbone: 2 : 1 for C
    ("majority beats the backbone", ["GATTACA", "GCTTACA", "GCTTACA"], 0, 20, "GCTTACA", 3, None),
    # smallest code: backbone N, members say G and C: tie between C and G, the backbone's N is no maximum: C
    ("smallest code at a tie", ["GANTACA", "GAGTACA", "GACTACA"], 0, 20, "GACTACA", 3, None),
    # deletion at exactly half is no deletion: cov 2, del 1
    ("deletion at half", ["GATTTACAGG", "GATTACAGG"], 0, 20, "GATTTACAGG", 2, [(1, 10, cs.ACCEPTED)]),
    # at half plus one: cov 3, del 2
    ("deletion above half", ["GATCTACAGG", "GATTACAGG", "GATTACAGG"], 0, 20, "GATTACAGG", 3, None),
    # insertion at exactly half (cov 2, ins 1) is none; two of three is one
    ("insertion at half", ["GATTACAGG", "GATCTACAGG"], 0, 20, "GATTACAGG", 2, [(1, 9, cs.ACCEPTED)]),
    ("insertion above half", ["GATTACAGG", "GATCTACAGG", "GATCTACAGG"], 0, 20, "GATCTACAGG", 3, None),
    # N in the member never matches and votes nothing; N in the backbone is filled by one member
    ("member N", ["GATTACA", "GANTACA", "GANTACA"], 0, 20, "GATTACA", 3, None),
    ("backbone N filled", ["GANTACA", "GATTACA"], 0, 20, "GATTACA", 2, [(1, 7, cs.ACCEPTED)]),
    # all N backbone alone: the bytes as they are
    ("lower case is N and kept", ["GAtTACA"], 0, 20, "GAtTACA", 1, []),
    # an insertion run of two votes its last base (the one next to the position behind the gap): members insert CG in front of
    # the second T: G is emitted, one base per gap
    ("run votes its last base", ["GATTACAGG", "GATCGTACAGG", "GATCGTACAGG"], 0, 40, "GATGTACAGG", 3, None),
    # a run at j == Lb votes nothing: members longer than the backbone at the far end
    ("run behind the backbone", ["GATTACA", "GATTACAC", "GATTACAC"], 0, 20, "GATTACA", 3, [(1, 7, cs.ACCEPTED)] * 2),
    # a gap in front of position 0
    ("gap in front of position 0", ["GATTACAGG", "CGATTACAGG", "CGATTACAGG"], 0, 20, "CGATTACAGG", 3, None),
    # anchor end: the same, mirrored
    ("anchor end mirrors", ["GGACATTAG", "GGACATCTAG", "GGACATCTAG"], 1, 20, "GGACATCTAG", 3, None),
]
