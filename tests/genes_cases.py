"""Inputs for the gene-call tests (badger_amd/genes.py, csrc/genes_kernels.hip): the rule once more in its plainest form, a
dictionary from window text to the set of features it occurs in; random small indexes and reads; a model transcriptome with
paralogs and a shared repeat; hand-derived cases for every clause of the rule."""
import numpy as np

from badger_amd import genes as gn

ACGT = "ACGT"


def rand_seq(rng, n, n_rate=0.0):
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)]
    if n_rate:
        s = np.where(rng.random(n) < n_rate, np.uint8(ord("N")), s)
    return s.astype(np.uint8).tobytes().decode()


def mutate(rng, s, sub=0.03, ins=0.02, dele=0.03):
    """synth's error rates by default; vectorised: a deletion, a substitution or neither per base, then an insertion behind it"""
    a = np.frombuffer(s.encode(), dtype=np.uint8)
    r = rng.random(len(a))
    code = gn._CODE[a].astype(np.int64) & 3
    subst = np.frombuffer(b"ACGT", dtype=np.uint8)[(code + rng.integers(1, 4, size=len(a))) % 4]
    b = np.where((r >= dele) & (r < dele + sub), subst, a)
    keep = r >= dele
    insert = rng.random(len(a)) < ins
    out = np.zeros((len(a), 2), dtype=np.uint8)
    out[:, 0] = np.where(keep, b, 0)
    out[:, 1] = np.where(insert, np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=len(a))], 0)
    out = out.ravel()
    return out[out != 0].tobytes().decode()


# ---------------------------------------------------------------- the plain form ----
def plain_index(seqs, features, k):
    """window text -> set of features; windows: how many had a key"""
    idx, windows = {}, 0
    for s, f in zip(seqs, features):
        for p in range(len(s) - k + 1):
            w = s[p:p + k]
            if all(c in ACGT for c in w):
                idx.setdefault(w, set()).add(int(f))
                windows += 1
    return idx, windows


def plain_assign(idx, read, k, min_hits):
    """-> (feature, hits, second, n_keys, n_found, flags)"""
    hits, n_keys, n_found = {}, 0, 0
    for p in range(len(read) - k + 1):
        w = read[p:p + k]
        if not all(c in ACGT for c in w):
            continue
        n_keys += 1
        if w in idx:
            n_found += 1
            if len(idx[w]) == 1:
                f = next(iter(idx[w]))
                hits[f] = hits.get(f, 0) + 1
    if len(hits) > gn.MAX_FEATURES:
        return (gn.NONE, 0, 0, n_keys, n_found, gn.CROWDED)
    if not hits:
        return (gn.NONE, 0, 0, n_keys, n_found, gn.LOW)
    top = max(hits.values())
    feature = min(f for f, c in hits.items() if c == top)
    second = max([c for f, c in hits.items() if f != feature], default=0)
    if top >= min_hits and top > second:
        flags = gn.ASSIGNED
    else:
        flags = (gn.LOW if top < min_hits else 0) | (gn.TIE if top == second and second > 0 else 0)
    return (feature, top, second, n_keys, n_found, flags)


def rec_tuples(recs):
    return [tuple(int(x) for x in r) for r in recs.tolist()]


# ---------------------------------------------------------------- random small inputs ----
def small_case(rng, k, n_seqs=None, max_len=None, n_rate=0.02):
    """a few short sequences over few features that share text, and reads cut from them, mutated, or random"""
    n_seqs = int(rng.integers(1, 7)) if n_seqs is None else n_seqs
    max_len = k + 40 if max_len is None else max_len
    pool = rand_seq(rng, max_len + 20)
    seqs, feats = [], []
    for _ in range(n_seqs):
        L = int(rng.integers(0, max_len + 1))
        if rng.random() < 0.5:
            a = int(rng.integers(0, 20))
            s = pool[a:a + L]                                            # shares windows with the others
        else:
            s = rand_seq(rng, L, n_rate)
        seqs.append(s)
        feats.append(int(rng.integers(0, 4)) if rng.random() < 0.9 else int(rng.integers(0, gn.AMBIGUOUS)))
    reads = []
    for _ in range(int(rng.integers(1, 8))):
        src = seqs[int(rng.integers(0, len(seqs)))] + pool
        a = int(rng.integers(0, 10))
        r = src[a:a + int(rng.integers(0, max_len + 10))]
        reads.append(mutate(rng, r) if rng.random() < 0.5 else r)
    reads.append(rand_seq(rng, int(rng.integers(0, 3 * k)), n_rate))
    return seqs, feats, reads


def tiny_index_case(rng, k, windows):
    """sequences with about `windows` windows in all, 1 .. 3 of them"""
    n = int(rng.integers(1, 4))
    cuts = sorted(int(x) for x in rng.integers(0, windows + 1, size=n - 1))
    parts = [b - a for a, b in zip([0] + cuts, cuts + [windows])]
    seqs = [rand_seq(rng, w + k - 1) if w else rand_seq(rng, int(rng.integers(0, k))) for w in parts]
    return seqs, [int(rng.integers(0, 3)) for _ in seqs]


# ---------------------------------------------------------------- the model transcriptome ----
def transcriptome(rng, n_genes=600, length=1500, n_paralogs=50, n_repeat=100, repeat_len=300, divergence=0.05):
    """random genes; the last n_paralogs are copies of the first ones with `divergence` of their bases substituted; n_repeat
    others share one repeat_len-base stretch at a random place"""
    genes = [rand_seq(rng, length) for _ in range(n_genes - n_paralogs)]
    genes += [mutate(rng, genes[i], sub=divergence, ins=0.0, dele=0.0) for i in range(n_paralogs)]
    repeat = rand_seq(rng, repeat_len)
    for g in rng.choice(np.arange(n_paralogs, n_genes - n_paralogs), size=n_repeat, replace=False).tolist():
        at = int(rng.integers(0, length - repeat_len + 1))
        genes[g] = genes[g][:at] + repeat + genes[g][at + repeat_len:]
    return genes


def fragments(rng, genes, n, lo, hi, random_every=5):
    """n reads: 3' fragments of lo .. hi bases of a random gene with synth's errors, every random_every-th a random sequence
    -> (reads, the gene of each or -1)"""
    reads, truth = [], []
    for i in range(n):
        L = int(rng.integers(lo, hi + 1))
        if random_every and i % random_every == random_every - 1:
            reads.append(rand_seq(rng, L))
            truth.append(-1)
        else:
            g = int(rng.integers(0, len(genes)))
            reads.append(mutate(rng, genes[g][-L:]))
            truth.append(g)
    return reads, truth


# ---------------------------------------------------------------- hand-derived cases ----
def hand_cases(k):
    """(name, sequences, features, read, min_hits, the record) - derived by hand from the rule, not from any code.
    X, Y, Z: three texts of k + 4 bases none of whose windows occur elsewhere (checked by the caller's plain form)."""
    rng = np.random.default_rng(100 + k)
    X, Y, Z = (rand_seq(rng, k + 4) for _ in range(3))            # 5 windows each
    A, N = gn.ASSIGNED, gn.NONE
    cases = [
        # one transcript holds X twice: its keys are unique all the same; the read X has 5 windows, all of feature 7
        ("twice in one transcript", [X + "N" + X], [7], X, 3, (7, 5, 0, 5, 5, A)),
        ("two transcripts of one gene", [X, X + "N" + Y], [7, 7], X, 3, (7, 5, 0, 5, 5, A)),
        # X in genes 1 and 2: its keys are found but belong to nobody
        ("two genes", [X, X], [1, 2], X, 3, (N, 0, 0, 5, 5, gn.LOW)),
        # ... while Y behind it in the read is gene 2's alone: X N Y has 5 + 5 windows with a key
        ("ambiguous and unique", [X, X + "N" + Y], [1, 2], X + "N" + Y, 3, (2, 5, 0, 10, 10, A)),
        ("a sequence of k - 1 bases", [X[:k - 1]], [0], X, 1, (N, 0, 0, 5, 0, gn.LOW)),
        ("a sequence of k bases", [X[:k]], [0], X, 1, (0, 1, 0, 5, 1, A)),
        ("a read of k - 1 bases", [X], [0], X[:k - 1], 1, (N, 0, 0, 0, 0, gn.LOW)),
        ("an empty read", [X], [0], "", 1, (N, 0, 0, 0, 0, gn.LOW)),
        ("a read of k bases", [X], [0], X[2:k + 2], 1, (0, 1, 0, 1, 1, A)),
        # hits at min_hits - 1 and at min_hits: the read holds 3 windows of X
        ("hits below min_hits", [X], [4], X[:k + 2], 4, (4, 3, 0, 3, 3, gn.LOW)),
        ("hits at min_hits", [X], [4], X[:k + 2], 3, (4, 3, 0, 3, 3, A)),
        # 5 windows of feature 9 and 5 of feature 3: a tie, the smaller id is reported
        ("a tie", [X, Y], [9, 3], X + "N" + Y, 3, (3, 5, 5, 10, 10, gn.TIE)),
        ("a tie below min_hits", [X, Y], [9, 3], X + "N" + Y, 6, (3, 5, 5, 10, 10, gn.LOW | gn.TIE)),
        # 5 of feature 9, 4 of feature 3, 2 of feature 5: the runner-up is the 4
        ("second best", [X, Y, Z], [9, 3, 5], X + "N" + Y[:k + 3] + "N" + Z[:k + 1], 3, (9, 5, 4, 11, 11, A)),
        # lower case is N: no window of the read has a key
        ("lower case", [X], [0], X.lower(), 1, (N, 0, 0, 0, 0, gn.LOW)),
        ("a window unknown to the index", [X], [0], Y, 1, (N, 0, 0, 5, 0, gn.LOW)),
    ]
    # an N at each position of a window: the read is one window of X with base j replaced; with the N it has no key
    for j in range(k):
        w = X[:k]
        cases.append(("N at %d" % j, [X], [0], w[:j] + "N" + w[j + 1:], 1, (N, 0, 0, 0, 0, gn.LOW)))
    return cases, (X, Y, Z)


def crowded_case(rng, k, n_features):
    """n_features transcripts of k bases, a feature each, and the read that strings them together with an N between: one
    window, one hit per feature -> (sequences, features, read)"""
    seqs = [rand_seq(rng, k) for _ in range(n_features)]
    return seqs, list(range(10, 10 + n_features)), "N".join(seqs)
