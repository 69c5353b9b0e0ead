"""The consensus rule in a band of W diagonals, once more in the plainest form: a full matrix with the band -H <= j - i <= H - 1
(H = W / 2) as a mask, one Python loop per cell, the votes as lists.  Written out again beside tests/consensus_cases.py (whose
band is 64); test_consensus_band.py holds badger_amd/consensus.py against it at 128 and 256, the device tests use band_pair."""
import numpy as np

from badger_amd import consensus as cs

INF = 1 << 30
ACGT = "ACGT"


def code(c):
    return ACGT.find(c) if c in ACGT else 4


def _cost(m, b):
    return 0 if m == b and m in ACGT else 1


def plain_align(M, B, band):
    """strings in anchor-first order -> (ed, span, steps) or None without a band cell in the last row; steps from the end:
    ('d', i, j) / ('v', i, j) / ('h', i, j) leaving cell (i, j)"""
    H = band // 2
    Lm, Lb = len(M), len(B)
    D = [[INF] * (Lb + 1) for _ in range(Lm + 1)]
    for i in range(Lm + 1):
        for j in range(max(0, i - H), min(Lb, i + H - 1) + 1):
            if i == 0 and j == 0:
                D[i][j] = 0
                continue
            best = INF
            if i and j and D[i - 1][j - 1] < INF:
                best = min(best, D[i - 1][j - 1] + _cost(M[i - 1], B[j - 1]))
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
        if i and j and D[i - 1][j - 1] < INF and D[i - 1][j - 1] + _cost(M[i - 1], B[j - 1]) == D[i][j]:
            steps.append(("d", i, j)); i -= 1; j -= 1
        elif i and D[i - 1][j] < INF and D[i - 1][j] + 1 == D[i][j]:
            steps.append(("v", i, j)); i -= 1
        else:
            steps.append(("h", i, j)); j -= 1
    return ed, span, steps


def plain_consensus(group, anchor, max_ed_pct, band):
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
        a = plain_align(M, B, band)
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


def rand_seq(rng, n, n_rate=0.0):
    s = rng.choice(list("ACGT"), size=n)
    if n_rate:
        s = np.where(rng.random(n) < n_rate, "N", s)
    return "".join(s.tolist())


# band-edge pairs in anchor-first order (use with ANCHOR_START), over a random text so that no shifted path is cheap.
# k >= 0: the member is the text without its first k bases, so its only cheap path deletes k backbone bases and then runs on the
# diagonal j - i = k (ed k).  k < 0: the member has |k| bases of its own in front, the path inserts them and runs on j - i = k.
# The backbone goes on for `tail` bases behind the member's end, so that the last row always has band cells.
def band_pair(k, n, tail=10):
    text = rand_seq(np.random.default_rng(4242), n + abs(k) + tail)
    if k >= 0:
        return text, text[k:k + n]                          # (backbone, member)
    return text[-k:], text[:n - k]
