"""Inputs for the variant-discovery tests (CPU and GPU): the rule of badger_amd/discover.py once more in its plainest form,
dictionaries from window text to genes and first place; random small cases; cases derived by hand from the rule's clauses; the
substitution scan that moves the enclosed base and its partner across every lane, chunk border and step border of the kernel;
and the planted pool of donors of the accuracy condition and the command-line tests."""
import numpy as np

import alleles_cases as ac
import genes_cases as gc
from badger_amd import discover as dv
from badger_amd import genes as gn

ACGT = "ACGT"
gene_recs = ac.gene_recs
other_letter = ac.other_letter


def _text(s):
    return s.decode() if isinstance(s, (bytes, bytearray)) else s


# ---------------------------------------------------------------- the plain form ----
def plain_index(seqs, features, k):
    """window text -> [set of features, smallest site]"""
    idx, start = {}, 0
    for s, f in zip(seqs, features):
        s = _text(s)
        for p in range(len(s) - k + 1):
            w = s[p:p + k]
            if all(c in ACGT for c in w):
                e = idx.setdefault(w, [set(), start + p])
                e[0].add(int(f))
                e[1] = min(e[1], start + p)
        start += len(s)
    return idx


def plain_pileup(idx, n_sites, reads, recs, k, counts=None):
    """-> counts as a list of [A, C, G, T] per site"""
    counts = [[0, 0, 0, 0] for _ in range(n_sites)] if counts is None else counts
    for read, rec in zip(reads, recs.tolist()):
        f, flags = rec[0], rec[5]
        if not flags & gn.ASSIGNED:
            continue
        read = _text(read)

        def site(i):
            e = idx.get(read[i:i + k]) if i + k <= len(read) else None
            return e[1] if e is not None and e[0] == {f} else None
        for i in range(len(read) - 2 * k):
            a, b, letter = site(i), site(i + k + 1), read[i + k]
            if a is not None and b is not None and b == a + k + 1 and letter in ACGT:
                counts[a + k][ACGT.index(letter)] += 1
    return counts


def plain_select(bases, counts, min_alt, ppm):
    """-> [(site, ref code, alt code, (counts))] by site"""
    out = []
    for s, c in enumerate(counts):
        depth, ref = sum(c), ACGT.find(chr(bases[s]))
        if depth == 0 or ref < 0:
            continue
        alt = max((a for a in range(4) if a != ref), key=lambda a: (c[a], -a))
        if c[alt] >= min_alt and c[alt] * 1000000 >= ppm * depth:
            out.append((s, ref, alt, tuple(c)))
    return out


def site_tuples(recs):
    return [(int(r["site"]), int(r["ref"]), int(r["alt"]), tuple(int(x) for x in r["count"])) for r in recs]


def plain_stats(idx, k):
    """the six figures through genes.Index.stats over the plain form's keys"""
    keys = np.array(sorted(int(gn.keys_of(w, k)[0]) for w in idx), dtype=np.uint64)
    by_key = {int(gn.keys_of(w, k)[0]): e for w, e in idx.items()}
    values = np.array([next(iter(by_key[int(x)][0])) if len(by_key[int(x)][0]) == 1 else gn.AMBIGUOUS for x in keys], dtype=np.uint32)
    return keys, values


# ---------------------------------------------------------------- random small cases ----
def small_case(rng, k, n_genes=None, n_reads=40):
    """a few genes of one or two transcripts (the second shares a stretch with the first), with N here and there; reads cut from
    them with a substitution or two, some with N, some assigned to another gene, some not ASSIGNED
    -> (seqs as bytes, features, reads, gene records)"""
    n_genes = int(rng.integers(1, 5)) if n_genes is None else n_genes
    seqs, feats = [], []
    for g in range(n_genes):
        t = gc.rand_seq(rng, int(rng.integers(2 * k + 2, 6 * k + 40)), n_rate=0.01 if rng.random() < 0.5 else 0.0)
        seqs.append(t)
        feats.append(g)
        if rng.random() < 0.5:
            a = int(rng.integers(0, len(t) // 2))
            seqs.append(gc.rand_seq(rng, int(rng.integers(0, 2 * k))) + t[a:a + int(rng.integers(k, len(t)))])
            feats.append(g)
    if n_genes > 1 and rng.random() < 0.7:                      # a stretch that two genes share: its keys are ambiguous
        seqs.append(seqs[0][:2 * k + 5] + gc.rand_seq(rng, k))
        feats.append(1)
    reads, of = [], []
    for _ in range(n_reads):
        q = int(rng.integers(0, len(seqs)))
        t = seqs[q]
        a = int(rng.integers(0, max(1, len(t) - k)))
        r = list(t[a:a + int(rng.integers(0, len(t) - a + 1))])
        for _ in range(int(rng.integers(0, 3))):
            if r:
                p = int(rng.integers(0, len(r)))
                r[p] = "N" if rng.random() < 0.2 else other_letter(rng, r[p]) if r[p] in ACGT else "A"
        reads.append("".join(r))
        of.append(feats[q] if rng.random() < 0.85 else int(rng.integers(0, n_genes)))
    return [s.encode() for s in seqs], np.array(feats, dtype=np.uint32), reads, gene_recs(of, rng.random(n_reads) < 0.9)


# ---------------------------------------------------------------- cases derived by hand ----
def _sub(t, p, letter=None):
    """t with another letter at p (the next of ACGT, cyclically, unless given)"""
    return t[:p] + (letter or ACGT[(ACGT.index(t[p]) + 1) % 4]) + t[p + 1:]


def hand_cases(k):
    """-> {name: dict(seqs, features, reads, recs, want: {site: [A, C, G, T]} of every site with evidence)}, each derived from the
    rule's clauses by counting windows, not by running code.  T is a random text whose windows are distinct."""
    rng = np.random.default_rng(1000 + k)
    L = 4 * k + 10
    while True:
        T = gc.rand_seq(rng, L)
        U = gc.rand_seq(rng, L)
        if len({(T + "N" + U)[i:i + k] for i in range(2 * L + 1 - k + 1)}) == 2 * L + 2 - k:
            break
    code = ACGT.index
    cases = {}

    def row(letter, n=1):
        c = [0, 0, 0, 0]
        c[code(letter)] = n
        return c

    # the whole transcript as a read: window i and window i + k + 1 both hit on the diagonal for i = 0 .. L - 2k - 1, so the sites
    # k .. L - k - 1 get their own letter once; the k sites at either end have no evidence
    cases["whole"] = dict(seqs=[T], features=[0], reads=[T], recs=gene_recs([0]), want={s: row(T[s]) for s in range(k, L - k)})
    # a read of exactly 2k + 1 bases cut at a: one pair, one site, a + k; 2k bases: none
    a = 7
    cases["shortest"] = dict(seqs=[T], features=[0], reads=[T[a:a + 2 * k + 1], T[a:a + 2 * k]], recs=gene_recs([0, 0]),
                             want={a + k: row(T[a + k])})
    # one substitution at p, k <= p < L - k: the windows that cover p do not hit, so of the pairs only i = p - k survives among
    # those whose either anchor is within k of p - the sites p - k .. p + k lose their evidence but for p itself, which gets the new
    # letter; sites further off keep theirs
    p = 2 * k + 3
    x = _sub(T, p)
    want = {s: row(T[s]) for s in range(k, L - k) if abs(s - p) > k}
    want[p] = row(x[p])
    cases["substitution"] = dict(seqs=[T], features=[0], reads=[x], recs=gene_recs([0]), want=want)
    # two variants d <= k apart (closer than k + 1): a read with both alternative letters gives neither site evidence (each one's
    # anchor holds the other), one with a single alternative letter gives exactly that site.  q = p + k: in the read with both, no
    # site from p - k to q + k (past the last site with evidence, L - k - 1) has two clean anchors; in the read with p's alone
    # the sites further than k from p keep theirs, those behind q included, and q itself (k from p) has none
    q = p + k
    both, only_p = _sub(x, q), x
    assert q + k >= L - k - 1
    want = {s: row(T[s], 2) for s in range(k, p - k)}
    want.update({s: row(T[s]) for s in range(p + k + 1, L - k)})
    want[p] = row(x[p])
    cases["two_close"] = dict(seqs=[T], features=[0], reads=[both, only_p], recs=gene_recs([0, 0]), want=want)
    # an N in the transcript at p: no key covers it, so the sites within k of it have no evidence.  Its own site has: the windows
    # on either side of it are whole, lie k + 1 apart and enclose the read's letter - a count that the selection never looks at
    # (the transcript's base there is no letter)
    tn = T[:p] + "N" + T[p + 1:]
    cases["transcript_N"] = dict(seqs=[tn], features=[0], reads=[T], recs=gene_recs([0]),
                                 want={s: row(T[s]) for s in range(k, L - k) if abs(s - p) > k or s == p})
    # an N in the read at the site: both anchors hit, the enclosed base is no letter: nothing at p, and as for a substitution around it
    rn = T[:p] + "N" + T[p + 1:]
    cases["read_N"] = dict(seqs=[T], features=[0], reads=[rn], recs=gene_recs([0]),
                           want={s: row(T[s]) for s in range(k, L - k) if abs(s - p) > k})
    # a read assigned to another gene, and one not ASSIGNED: the keys are found, nothing counts
    cases["other_gene"] = dict(seqs=[T, U], features=[0, 1], reads=[T, T, U], recs=gene_recs([1, 0, 1], [True, False, True]),
                               want={L + s: row(U[s]) for s in range(k, L - k)})
    # a stretch in two genes: its keys are ambiguous and hit for neither.  U' = U with T's first 2k + 1 bases in front; a read of
    # gene 0 that is T has no left anchor i < k + 2 (windows 0 .. k + 1 lie inside the shared stretch... those that start at
    # 0 .. k + 1 are whole inside T[:2k + 1]), so the first pair is i = k + 2 and the first site 2k + 2
    shared = T[:2 * k + 1] + _sub(T, 2 * k + 1)[2 * k + 1] + U     # (another letter behind the stretch than T has there)
    cases["two_genes"] = dict(seqs=[T, shared], features=[0, 1], reads=[T], recs=gene_recs([0]),
                              want={s: row(T[s]) for s in range(2 * k + 2, L - k)})
    # two isoforms of one gene: A = E1 E2 E3 first in the file, B = E1 E3 (E2 skipped).  Sites are A's coordinates for everything B
    # shares.  A read that is B: pairs inside E1 and inside E3 count at A's coordinates; a pair whose anchors lie on either side of
    # B's junction, or across it, resolves to two places that are not k + 1 apart (or to B's own junction keys, at B's coordinates,
    # next to anchors at A's) - no evidence within k of the junction
    e = 2 * k + 3
    E1, E3 = T[:e], T[e:2 * e]
    # (E2 starts with another letter than E3 and ends with another than E1: no window across a junction of A is one of B's)
    E2 = _sub(E3, 0)[0] + U[1:e - 1] + _sub(E1, e - 1)[e - 1]
    A, B = E1 + E2 + E3, E1 + E3
    want = {s: row(A[s]) for s in range(k, e - k)}                                   # inside E1
    want.update({2 * e + s: row(E3[s]) for s in range(k, e - k)})                     # inside E3, at A's coordinate
    cases["isoforms"] = dict(seqs=[A, B], features=[0, 0], reads=[B], recs=gene_recs([0]), want=want)
    # a key that recurs inside its gene: R = X + T[:k] with X = T, so the last window's key stands at site 0 first.  A read of the
    # tail R[L - k - 1:] (k + 1 + k bases) has one pair, i = L - k - 1: its left anchor resolves to L - k - 1, the partner to 0 and
    # not to L: dropped.  The same read one base longer to the left has a second pair, i = L - k - 2 with partner L - 1: it counts
    R = T + T[:k]
    cases["recurring"] = dict(seqs=[R], features=[0], reads=[R[L - k - 1:], R[L - k - 2:L + k - 1]], recs=gene_recs([0, 0]),
                              want={L - 2: row(R[L - 2])})
    for c in cases.values():
        c["seqs"] = [s.encode() for s in c["seqs"]]
        c["features"] = np.array(c["features"], dtype=np.uint32)
    return cases


# ---------------------------------------------------------------- shapes for the kernel ----
def scan_case(k, length=700, seed=5):
    """one transcript of `length` bases and a read per position p: the transcript with one substitution at p"""
    rng = np.random.default_rng(seed + k)
    T = gc.rand_seq(rng, length)
    return [T.encode()], np.zeros(1, dtype=np.uint32), [_sub(T, p) for p in range(length)], gene_recs([0] * length)


def length_case(k, seed=6):
    """reads of the lengths 0, 2k, 2k + 1, 2k + 2 and around one and two steps of 256 - (k + 1) windows, each with a substitution
    in its middle where it has one"""
    rng = np.random.default_rng(seed + k)
    T = gc.rand_seq(rng, 700)
    step = 256 - (k + 1)
    lens = [0, 1, k, 2 * k, 2 * k + 1, 2 * k + 2] + [m * step + d for m in (1, 2) for d in (-1, 0, 1, k, 2 * k, 2 * k + 1, 2 * k + 2)] + \
        [255, 256, 257, 511, 512, 513]
    reads = []
    for i, n in enumerate(lens):
        a = (3 * i) % (700 - n + 1)
        r = T[a:a + n]
        reads.append(_sub(r, n // 2) if n else r)
    return [T.encode()], np.zeros(1, dtype=np.uint32), reads, gene_recs([0] * len(reads))


def hot_case(k, n_reads=20000, length=300, seed=7):
    """n_reads reads of one transcript of `length` bases: whole copies with a substitution each, so that every add meets the same
    few hundred addresses"""
    rng = np.random.default_rng(seed + k)
    T = gc.rand_seq(rng, length)
    where = rng.integers(0, length, size=n_reads)
    return [T.encode()], np.zeros(1, dtype=np.uint32), [_sub(T, int(p)) for p in where], gene_recs([0] * n_reads)


# ---------------------------------------------------------------- the planted pool ----
def pool(rng, n_genes=40, length=1500, per_gene=4, n_donors=4, n_cells=200, n_reads=6000, lo=300, hi=1000, errors=True):
    """random genes with per_gene sites each, donors with random genotypes 0 / 1 / 2 at every site, cells of one donor each; a read
    is a 3' fragment of lo .. hi bases of a random gene from a random cell, each site carrying an allele drawn from the cell's
    donor's genotype, with genes_cases.mutate's default errors -> dict(tx_names, tx_seqs (bytes), sites: {(gene, pos): (ref, alt)},
    geno [n_sites, n_donors], reads, gene (per read), cell (per read), donor (per cell))"""
    tx, sites, keys = [], {}, []
    for g in range(n_genes):
        t = gc.rand_seq(rng, length)
        for p in sorted(int(x) for x in rng.choice(length, size=per_gene, replace=False)):
            sites[(g, p)] = (t[p], other_letter(rng, t[p]))
            keys.append((g, p))
        tx.append(t)
    geno = rng.integers(0, 3, size=(len(keys), n_donors))
    donor = rng.integers(0, n_donors, size=n_cells)
    reads, gene, cell = [], [], []
    for _ in range(n_reads):
        g, c = int(rng.integers(0, n_genes)), int(rng.integers(0, n_cells))
        n = int(rng.integers(lo, hi + 1))
        text = list(tx[g][length - n:])
        for i, (sg, p) in enumerate(keys):
            dosage = int(geno[i, donor[c]])
            if sg == g and p >= length - n and (dosage == 2 or (dosage == 1 and rng.integers(0, 2) == 1)):
                text[p - (length - n)] = sites[(sg, p)][1]
        text = "".join(text)
        reads.append(gc.mutate(rng, text) if errors else text)
        gene.append(g)
        cell.append(c)
    return dict(tx_names=["g%d" % g for g in range(n_genes)], tx_seqs=[t.encode() for t in tx], sites=sites, keys=keys, geno=geno,
                reads=reads, gene=np.array(gene), cell=np.array(cell), donor=donor, length=length)


def score(model, recs):
    """-> (true, false, polymorphic): selected records that are a planted site with its letters, the others, and the planted sites
    at which some donor carries the alternative letter"""
    L = model["length"]
    planted = {g * L + p: (ACGT.index(r), ACGT.index(a)) for (g, p), (r, a) in model["sites"].items()}
    true = sum(1 for r in recs if planted.get(int(r["site"])) == (int(r["ref"]), int(r["alt"])))
    return true, len(recs) - true, int((model["geno"].sum(axis=1) > 0).sum())
