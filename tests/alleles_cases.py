"""Inputs for the allele-count tests (CPU and GPU): a plain dictionary form of the rule of badger_amd/alleles.py, random small
cases, cases derived by hand from the rule's clauses, and the planted transcriptome of the accuracy condition."""
import numpy as np

import genes_cases as gc
from badger_amd import alleles as al
from badger_amd import genes as gn

ACGT = "ACGT"


def gene_recs(features, assigned=None):
    """gene records ASSIGNED to the features (assigned: a bool per read, False -> LOW with the feature kept)"""
    recs = np.zeros(len(features), dtype=gn.REC_DTYPE)
    recs["feature"] = features
    recs["hits"] = 5
    recs["flags"] = gn.ASSIGNED if assigned is None else np.where(assigned, gn.ASSIGNED, gn.LOW)
    return recs


# ---------------------------------------------------------------- the plain form ----
def plain_index(seqs, values, k):
    """window text -> set of values"""
    idx = {}
    for s, v in zip(seqs, values):
        s = s.decode() if isinstance(s, bytes) else s
        for p in range(len(s) - k + 1):
            w = s[p:p + k]
            if all(c in ACGT for c in w):
                idx.setdefault(w, set()).add(int(v))
    return idx


def plain_assign(idx, gene_of_variant, reads, recs, k):
    """-> (sorted list of (read, variant, ref_hits, alt_hits), crowded reads)"""
    gene_of_variant = [int(g) for g in gene_of_variant]
    out, crowded = [], 0
    for r, read in enumerate(reads):
        read = read.decode() if isinstance(read, bytes) else read
        g = int(recs["feature"][r])
        if not int(recs["flags"][r]) & gn.ASSIGNED or g not in gene_of_variant:
            continue
        hits = {}
        for p in range(len(read) - k + 1):
            vs = idx.get(read[p:p + k])
            if vs is not None and len(vs) == 1:
                v = next(iter(vs))
                if gene_of_variant[v >> 1] == g:
                    hits[v] = hits.get(v, 0) + 1
        which = sorted({v >> 1 for v in hits})
        if len(which) > al.MAX_VARIANTS:
            crowded += 1
            continue
        out += [(r, v, hits.get(2 * v, 0), hits.get(2 * v + 1, 0)) for v in which]
    return out, crowded


def plain_stats(idx, n_variants):
    """-> (distinct keys, ambiguous keys, usable keys per value)"""
    per_value = [0] * (2 * n_variants)
    for vs in idx.values():
        if len(vs) == 1:
            per_value[next(iter(vs))] += 1
    return len(idx), sum(1 for vs in idx.values() if len(vs) > 1), per_value


def rec_tuples(recs):
    return sorted(tuple(int(x) for x in r) for r in recs.tolist())


def other_letter(rng, c):
    return ACGT[(ACGT.index(c) + 1 + int(rng.integers(0, 3))) % 4]


def with_alleles(t, sites, hap):
    """the text t with the alt letter at every site (p, ref, alt) whose bit of hap is set"""
    s = list(t)
    for (p, _, a), h in zip(sites, hap):
        if h:
            s[p] = a
    return "".join(s)


# ---------------------------------------------------------------- random small cases ----
def small_case(rng, k, n_genes=None, n_reads=40):
    """a few genes of one or two isoforms (the second lacks a stretch of the first), a few sites per gene - some close together,
    some next to an N, some genes without any - and reads cut from random haplotypes with errors, with gene records that are
    mostly the read's own gene, now and then another's or not ASSIGNED
    -> dict(tx_seqs bytes, feat, names, variants, reads, recs)"""
    n_genes = int(rng.integers(1, 5)) if n_genes is None else n_genes
    tx_seqs, feat, names, ids, ref, alt, gene, occ, sites_of = [], [], [], [], [], [], [], [], []
    for g in range(n_genes):
        L = int(rng.integers(k + 2, 4 * k + 30))
        a = gc.rand_seq(rng, L, n_rate=0.02 if rng.integers(0, 2) else 0.0)
        names.append("g%d" % g)
        qa = len(tx_seqs)
        tx_seqs.append(a.encode())
        feat.append(g)
        cut = None
        if rng.integers(0, 2) and L > k + 10:
            c0 = int(rng.integers(1, L - 5))
            c1 = int(rng.integers(c0 + 1, min(L, c0 + 20)))
            cut = (c0, c1)
            tx_seqs.append((a[:c0] + a[c1:]).encode())
            feat.append(g)
        sites = []
        if rng.integers(0, 5):
            want = int(rng.integers(1, 5))
            places = sorted({int(x) for x in rng.integers(0, L, size=want)} | ({min(L - 1, int(rng.integers(0, L)) + 3)} if want > 1 else set()))
            for p in places:
                if a[p] not in ACGT:
                    continue
                v = len(ids)
                ids.append("v%d" % v)
                ref.append(a[p])
                alt.append(other_letter(rng, a[p]))
                gene.append(g)
                occ.append((v, qa, p))
                if cut is not None and not cut[0] <= p < cut[1]:
                    occ.append((v, qa + 1, p if p < cut[0] else p - (cut[1] - cut[0])))
                sites.append((p, ref[-1], alt[-1]))
        sites_of.append((a, sites))
    reads, feats, ok = [], [], []
    for _ in range(n_reads):
        g = int(rng.integers(0, n_genes))
        a, sites = sites_of[g]
        text = with_alleles(a, sites, rng.integers(0, 2, size=len(sites)))
        lo = int(rng.integers(0, max(1, len(text) - k)))
        frag = text[lo:int(rng.integers(lo, len(text) + 1))]
        reads.append(gc.mutate(rng, frag) if rng.integers(0, 3) == 0 else frag)
        feats.append(g if rng.integers(0, 10) else int(rng.integers(0, n_genes)))
        ok.append(bool(rng.integers(0, 12)))
    return dict(tx_seqs=tx_seqs, feat=np.array(feat, dtype=np.uint32), names=names, variants=al.Variants(ids, ref, alt, gene, occ),
                reads=reads, recs=gene_recs(feats, np.array(ok, dtype=bool)))


# ---------------------------------------------------------------- by hand ----
def hand_cases(k):
    """cases derived by hand from the rule, not from any code: dict(name, tx_seqs, feat, names, variants, reads, recs, want - the
    records as sorted tuples, per_value - usable keys per value, ambiguous - ambiguous keys).  The texts are random: none of
    their windows recurs (the caller's plain form agrees or the test fails)."""
    rng = np.random.default_rng(400 + k)
    out = []

    def case(name, tx, feat, variants, reads, recs, want, per_value, ambiguous):
        out.append(dict(name=name, tx_seqs=[t.encode() for t in tx], feat=np.array(feat, dtype=np.uint32),
                        names=["g%d" % g for g in range(max(feat) + 1)], variants=variants, reads=reads, recs=recs, want=sorted(want),
                        per_value=per_value, ambiguous=ambiguous))

    # a site at the transcript's first and at its last base: the sequences are clipped to k bases, one window each
    t = gc.rand_seq(rng, k + 5)
    a0, a1 = other_letter(rng, t[0]), other_letter(rng, t[-1])
    v = al.Variants(["first", "last"], [t[0], t[-1]], [a0, a1], [0, 0], [(0, 0, 0), (1, 0, k + 4)])
    case("first and last base", [t], [0], v, [a0 + t[1:], t, a0 + t[1:-1] + a1, t[1:]], gene_recs([0, 0, 0, 0]),
         [(0, 0, 0, 1), (0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 1, 0), (2, 0, 0, 1), (2, 1, 0, 1), (3, 1, 1, 0)], [1, 1, 1, 1], 0)

    # a site right behind an N: of the k windows that would cover it only the one that starts at the site has a key
    x, y = gc.rand_seq(rng, k + 3), gc.rand_seq(rng, k + 3)
    t = x + "N" + y
    p = len(x) + 1
    a0 = other_letter(rng, y[0])
    v = al.Variants(["behind_N"], [y[0]], [a0], [0], [(0, 0, p)])
    case("next to an N", [t], [0], v, [t, y, a0 + y[1:], x + "A" + a0 + y[1:]], gene_recs([0, 0, 0, 0]),
         [(0, 0, 1, 0), (1, 0, 1, 0), (2, 0, 0, 1), (3, 0, 0, 1)], [1, 1], 0)

    # two sites k - 1 and k apart: one window covers both at k - 1, none at k
    for d in (k - 1, k):
        t = gc.rand_seq(rng, 3 * k)
        p1, p2 = k, k + d
        s = [(p1, t[p1], other_letter(rng, t[p1])), (p2, t[p2], other_letter(rng, t[p2]))]
        v = al.Variants(["left", "right"], [s[0][1], s[1][1]], [s[0][2], s[1][2]], [0, 0], [(0, 0, p1), (1, 0, p2)])
        reads = [with_alleles(t, s, h) for h in ((0, 0), (1, 0), (0, 1), (1, 1))]
        if d == k - 1:
            # the one window over both: ref/ref ambiguous, one alt votes for that alt (k hits with the k - 1 others), alt/alt absent
            want = [(0, 0, k - 1, 0), (0, 1, k - 1, 0), (1, 0, 0, k), (1, 1, k - 1, 0), (2, 0, k - 1, 0), (2, 1, 0, k), (3, 0, 0, k - 1), (3, 1, 0, k - 1)]
            per_value, ambiguous = [k - 1, k, k - 1, k], 1
        else:
            want = [(0, 0, k, 0), (0, 1, k, 0), (1, 0, 0, k), (1, 1, k, 0), (2, 0, k, 0), (2, 1, 0, k), (3, 0, 0, k), (3, 1, 0, k)]
            per_value, ambiguous = [k, k, k, k], 0
        case("two sites %d apart" % d, [t], [0], v, reads, gene_recs([0] * 4), want, per_value, ambiguous)

    # the same site in two isoforms of one gene, in the second three bases behind its start: they share the keys
    t = gc.rand_seq(rng, 3 * k)
    p = k + 4
    a0 = other_letter(rng, t[p])
    v = al.Variants(["shared"], [t[p]], [a0], [0], [(0, 0, p), (0, 1, 3)])
    case("one site in two isoforms", [t, t[p - 3:]], [0, 0], v, [t, t[:p] + a0 + t[p + 1:], t[p - 3:]], gene_recs([0, 0, 0]),
         [(0, 0, k, 0), (1, 0, 0, k), (2, 0, 4, 0)], [k, k], 0)

    # gene 0's keys in reads given to gene 1 (which has a variant of its own) and to gene 2 (which has none); a read that is not
    # ASSIGNED; a read with both alleles: k ref windows, an N, the alt sequence without its first base, k - 1 alt windows
    t0, t1, t2 = gc.rand_seq(rng, 2 * k + 1), gc.rand_seq(rng, 2 * k + 1), gc.rand_seq(rng, 2 * k + 1)
    a0, b0 = other_letter(rng, t0[k]), other_letter(rng, t1[k])
    v = al.Variants(["in_g0", "in_g1"], [t0[k], t1[k]], [a0, b0], [0, 1], [(0, 0, k), (1, 1, k)])
    alt0 = t0[:k] + a0 + t0[k + 1:]
    reads = [t0, t0, t0, t0, t0 + "N" + alt0[2:], t0 + "N" + alt0[1:], t1 + "N" + t0]
    recs = gene_recs([0, 1, 2, 0, 0, 0, 1], np.array([1, 1, 1, 0, 1, 1, 1], dtype=bool))
    case("gene gate, not assigned, both alleles", [t0, t1, t2], [0, 1, 2], v, reads, recs,
         [(0, 0, k, 0), (4, 0, k, k - 1), (5, 0, k, k), (6, 1, k, 0)], [k, k, k, k], 0)
    return out


def crowded_case(rng, k, n_variants):
    """one gene with n_variants sites k apart, read whole: every site has its k windows, none covers two -> (transcript, Variants)"""
    t = gc.rand_seq(rng, k * (n_variants + 1))
    places = [k * (i + 1) - 1 for i in range(n_variants)]
    return t, al.Variants(["c%d" % i for i in range(n_variants)], [t[p] for p in places], [other_letter(rng, t[p]) for p in places],
                          [0] * n_variants, [(i, 0, p) for i, p in enumerate(places)])


# ---------------------------------------------------------------- the accuracy condition ----
def planted(rng, n_genes=200, length=1500, per_gene=4, n_molecules=300, per_molecule=5, lo=300, hi=1000):
    """random genes with per_gene sites each; molecules of a random gene and haplotype, per_molecule fragments of lo .. hi bases of
    each with genes_cases.mutate's default errors -> dict(tx_seqs, variants, reads, recs: ASSIGNED to the read's own gene,
    molecule per read, truth: {(read, variant): allele} for every site the read's fragment covers)"""
    tx, ids, ref, alt, gene, occ, sites_of = [], [], [], [], [], [], []
    for g in range(n_genes):
        t = gc.rand_seq(rng, length)
        places = sorted(int(x) for x in rng.choice(length, size=per_gene, replace=False))
        sites = []
        for p in places:
            sites.append((p, t[p], other_letter(rng, t[p])))
            occ.append((len(ids), g, p))
            ids.append("snv%d" % len(ids))
            ref.append(t[p])
            alt.append(sites[-1][2])
            gene.append(g)
        tx.append(t)
        sites_of.append(sites)
    reads, feats, molecule, truth = [], [], [], {}
    for m in range(n_molecules):
        g = int(rng.integers(0, n_genes))
        hap = rng.integers(0, 2, size=per_gene)
        text = with_alleles(tx[g], sites_of[g], hap)
        for _ in range(per_molecule):
            n = int(rng.integers(lo, hi + 1))
            a = int(rng.integers(0, length - n + 1))
            for i, (p, _, _) in enumerate(sites_of[g]):
                if a <= p < a + n:
                    truth[(len(reads), g * per_gene + i)] = int(hap[i])
            reads.append(gc.mutate(rng, text[a:a + n]))
            feats.append(g)
            molecule.append(m)
    return dict(tx_seqs=[t.encode() for t in tx], variants=al.Variants(ids, ref, alt, gene, occ), reads=reads, recs=gene_recs(feats),
                molecule=np.array(molecule), truth=truth, n_features=n_genes)


def recurring_keys(tx_seqs, variants, k):
    """allele keys that also stand in a transcript of their own gene at a window that does not cover the site (ref keys only can:
    the count is over both alleles' keys looked up in the gene's reference text)"""
    seqs, values = al.allele_sequences(variants, tx_seqs, k)
    n = 0
    for (v, q, p), i in zip(variants.occ, range(0, len(seqs), 2)):
        t = tx_seqs[q]
        starts = {}
        for s in range(len(t) - k + 1):
            starts.setdefault(t[s:s + k], []).append(s)
        for a in (0, 1):
            s_ = seqs[i + a]
            for w in {s_[j:j + k] for j in range(len(s_) - k + 1)}:
                n += any(not p - k + 1 <= s <= p for s in starts.get(w, ()))
    return n
