"""Inputs for the isoform tests (badger_amd/genes.py, the k_iso kernels of csrc/genes_kernels.hip): the rule once more in its
plainest form, dictionaries from window text to the set of features and to the set of local indices; random small genes with
several transcripts; the model of genes, exons and skipping isoforms that the accuracy condition states."""
import numpy as np

import genes_cases as gc
from badger_amd import genes as gn

ACGT = "ACGT"
ALL = (1 << 64) - 1


# ---------------------------------------------------------------- the plain form ----
def plain_masks(seqs, local, k):
    """window text -> set of local indices, over every sequence whatever its feature"""
    out = {}
    for s, t in zip(seqs, local):
        for p in range(len(s) - k + 1):
            w = s[p:p + k]
            if all(c in ACGT for c in w):
                out.setdefault(w, set()).add(int(t))
    return out


def plain_iso(idx, masks, read, k, gene_rec, margin):
    """idx: genes_cases.plain_index's dictionary; gene_rec: the read's gene record as a tuple
    -> (compat, feature, best, second, n_gene, flags, pad)"""
    if not gene_rec[5] & gn.ASSIGNED:
        return (0, gn.NONE, 0, 0, 0, gn.ISO_NOGENE, 0)
    f, cnt, n_gene = gene_rec[0], [0] * 64, 0
    for p in range(len(read) - k + 1):
        w = read[p:p + k]
        if w in idx and idx[w] == {f}:
            n_gene += 1
            for t in masks[w]:
                cnt[t] += 1
    best = max(cnt)
    second = max([c for c in cnt if c < best], default=0)
    compat = sum(1 << t for t in range(64) if cnt[t] > 0 and best - cnt[t] < margin)
    bits = bin(compat).count("1")
    return (compat, f, best, second, n_gene, gn.ISO_UNIQUE if bits == 1 else gn.ISO_MULTI if bits > 1 else 0, 0)


def iso_tuples(recs):
    return [tuple(int(x) for x in r) for r in recs.tolist()]


def rule(index, reads, min_hits, margin):
    """both records of the checker -> (gene tuples, iso tuples)"""
    g = gn.assign_reads(index, reads, min_hits)
    return gc.rec_tuples(g), iso_tuples(gn.iso_assign_reads(index, reads, g, margin))


# ---------------------------------------------------------------- random small inputs ----
def small_case(rng, k):
    """a few genes of a few transcripts cut from one pool each (so that they share windows, within a gene and now and then
    across genes), local indices by the command line's rule or random, and reads cut from them, mutated, or random"""
    seqs, feats = [], []
    for g in range(int(rng.integers(1, 4))):
        pool = gc.rand_seq(rng, k + 60)
        for _ in range(int(rng.integers(1, 5))):
            a, b = int(rng.integers(0, 20)), len(pool) - int(rng.integers(0, 20))
            cut = int(rng.integers(a, b + 1))
            s = pool[a:cut] + pool[min(b, cut + int(rng.integers(0, 30))):b]      # an exon of the pool skipped
            seqs.append(s if rng.random() < 0.9 else s[:len(s) // 2] + "N" + s[len(s) // 2:])
            feats.append(g if rng.random() < 0.9 else int(rng.integers(0, 3)))
    local = gn.local_indices(feats)[0].tolist() if rng.random() < 0.5 else [int(x) for x in rng.integers(0, 64, size=len(seqs))]
    reads = []
    for _ in range(int(rng.integers(2, 9))):
        src = seqs[int(rng.integers(0, len(seqs)))]
        a = int(rng.integers(0, 10))
        r = src[a:a + int(rng.integers(0, k + 70))]
        reads.append(gc.mutate(rng, r) if rng.random() < 0.3 else r)
    reads.append(gc.rand_seq(rng, int(rng.integers(0, 3 * k))))
    return seqs, feats, local, reads


# ---------------------------------------------------------------- the model of the accuracy condition ----
def model(rng, n_genes, exon_lo=60, exon_hi=300, polya=30):
    """genes of 4 .. 8 random exons of exon_lo .. exon_hi bases; 2 .. 4 isoforms per gene that each skip a different subset of
    the internal exons (never more isoforms than there are subsets), the first and the last exon in all of them; a polyA of
    `polya` bases behind each -> (transcript names, sequences, gene id of each)"""
    names, seqs, gene = [], [], []
    for g in range(n_genes):
        exons = [gc.rand_seq(rng, int(rng.integers(exon_lo, exon_hi + 1))) for _ in range(int(rng.integers(4, 9)))]
        inner = len(exons) - 2
        n_iso = min(int(rng.integers(2, 5)), 1 << inner)
        for i, subset in enumerate(rng.choice(1 << inner, size=n_iso, replace=False).tolist()):
            kept = [exons[0]] + [e for j, e in enumerate(exons[1:-1]) if not subset >> j & 1] + [exons[-1]]
            names.append("G%d.%d" % (g, i))
            seqs.append("".join(kept) + "A" * polya)
            gene.append(g)
    return names, seqs, gene


def fragments(rng, seqs, gene, n, lo=150, hi=1000):
    """n reads: the last lo .. hi bases of a random transcript at synth's error rates
    -> (reads, the transcript of each, whether the fragment as cut lies in no other transcript of the gene)"""
    by_gene = {}
    for q, g in enumerate(gene):
        by_gene.setdefault(g, []).append(q)
    reads, truth, alone = [], [], []
    for _ in range(n):
        q = int(rng.integers(0, len(seqs)))
        frag = seqs[q][-int(rng.integers(lo, hi + 1)):]
        reads.append(gc.mutate(rng, frag))
        truth.append(q)
        alone.append(not any(frag in seqs[o] for o in by_gene[gene[q]] if o != q))
    return reads, truth, alone
