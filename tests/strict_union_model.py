"""Host model of k_strict_filter's search (extract_kernels.hip: myers_search) and of the windows it runs over, shared by
test_strict_union_model.py (CPU) and test_strict_union_gpu.py.  Not a test module."""
import numpy as np

R1 = "CTACACGACGCTCTTCCGATCT"
R1_LEN, KMER = 22, 6
MAX_ED = 5                        # a strict alignment (score >= 17) needs semi-global edit distance <= 5
_PEQ = {c: sum(1 << i for i, x in enumerate(R1) if x == c) for c in "ACGT"}      # 'N' matches nothing
_M = (1 << R1_LEN) - 1


def hit_window(L, pos):
    """[start, end) of the window of one hit at strand position pos of a strand of L bases"""
    return max(0, pos - (R1_LEN - KMER)), min(L, pos + R1_LEN + 1)


def union_window(L, pos, last):
    """the window of a group of hits from pos to last: from the first hit's start to the last hit's end"""
    return max(0, pos - (R1_LEN - KMER)), min(L, last + R1_LEN + 1)


def myers_best(texts, columns=40):
    """min over the end columns of the edit distance of R1 to a substring ending there (free start), for each text
    (str, at most `columns` bases): the kernel's recurrence, every text padded with 'N' to `columns` columns."""
    n = len(texts)
    assert all(len(t) <= columns for t in texts)
    arr = np.full((n, columns), ord("N"), np.uint8)
    for i, t in enumerate(texts):
        arr[i, :len(t)] = np.frombuffer(t.encode("ascii"), np.uint8)
    peq = np.zeros(256, np.int64)
    for c, v in _PEQ.items():
        peq[ord(c)] = v
    pv = np.full(n, _M, np.int64)
    mv = np.zeros(n, np.int64)
    score = np.full(n, R1_LEN, np.int64)
    best = score.copy()
    for j in range(columns):
        eq = peq[arr[:, j]]
        xv = eq | mv
        xh = ((((eq & pv) + pv) ^ pv) | eq) & _M
        ph = (mv | ~(xh | pv)) & _M
        mh = pv & xh
        score += (ph >> (R1_LEN - 1)) & 1
        score -= (mh >> (R1_LEN - 1)) & 1
        ph = (ph << 1) & _M                                   # search: D[0][j] = 0
        mh = (mh << 1) & _M
        pv = (mh | ~(xv | ph)) & _M
        mv = ph & xv
        best = np.minimum(best, score)
    return best


def semi_global_dp(text):
    """the same quantity from the edit-distance table: D[0][j] = 0, D[i][0] = i, min over the last row (column 0 included)"""
    col = list(range(R1_LEN + 1))
    best = col[R1_LEN]
    for c in text:
        new = [0] * (R1_LEN + 1)
        for i in range(1, R1_LEN + 1):
            new[i] = min(col[i] + 1, new[i - 1] + 1, col[i - 1] + (0 if (c == R1[i - 1] and c != "N") else 1))
        col = new
        best = min(best, col[R1_LEN])
    return best


def edited_r1(rng, run, edits):
    """a copy of R1 that keeps one `run`-mer of R1 whole (run - 5 neighbouring 6-mer hits) and carries `edits`
    substitutions, insertions and deletions elsewhere, the bases on both sides of the run among them.
    -> (sequence, offset of the run inside it)"""
    q = int(rng.integers(0, R1_LEN - run + 1))
    cells = [[c] for c in R1]                                  # cell i: what stands for R1[i]
    free = [i for i in range(R1_LEN) if i < q or i >= q + run]
    first = [i for i in (q - 1, q + run) if 0 <= i < R1_LEN]
    order = first + [i for i in rng.permutation(free).tolist() if i not in first]
    for i in order[:edits]:
        kind = rng.random()
        other = [b for b in "ACGT" if b != R1[i]]
        if kind < 0.6 or i in first:
            cells[i] = [other[int(rng.integers(0, 3))]]
        elif kind < 0.8:
            cells[i] = []
        else:
            cells[i] = [other[int(rng.integers(0, 3))], R1[i]] if i >= q + run else [R1[i], other[int(rng.integers(0, 3))]]
    seq = "".join("".join(c) for c in cells)
    return seq, len("".join("".join(c) for c in cells[:q]))
