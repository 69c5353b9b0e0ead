"""Inputs for bdg_umi_dedup_genes_dev (csrc/umi_kernels.hip) and the rule it computes (umi_dedup.dedup_per_gene): the cases of
tests/umi_cases.py with features dealt over each cell's reads, group tables as full as they get, one hot group, groups of one
read, the extreme ordinals, and a hand-derived case for every clause of the rule.  A helper module (imported like
umi_cases.py), no test itself.

A GeneCase holds the reads as the device takes them: cell ordinal uint32 (NONE: no cell), gene records (feature, flags; the
other fields do not matter to the rule), UMI code uint32, and the UMI text beside it."""
import random

import numpy as np

import umi_cases as uc
from badger_amd import genes as gn
from badger_amd import umi_dedup as ud

NONE = 0xFFFFFFFF
NOT_ASSIGNED = (gn.TIE, gn.LOW, gn.CROWDED, gn.LOW | gn.TIE, 0)


class GeneCase:
    def __init__(self, name, reads):
        """reads: (cell ordinal or None, feature, flags, UMI text) per read"""
        self.name = name
        self.n = len(reads)
        self.cell = np.array([NONE if r[0] is None else r[0] for r in reads], dtype=np.uint32)
        self.recs = np.zeros(self.n, dtype=gn.REC_DTYPE)
        self.recs["feature"] = np.array([r[1] for r in reads], dtype=np.uint32)
        self.recs["flags"] = np.array([r[2] for r in reads], dtype=np.uint32)
        self.recs["hits"] = 7                                        # (what a record holds beside feature and flags is not read)
        self.umi_text = [r[3] for r in reads]
        self.umi = ud.umi_codes(self.umi_text)
        self.reads = list(reads)

    def __repr__(self):
        return "GeneCase(%s, %d reads)" % (self.name, self.n)

    def shuffled(self, seed):
        perm = np.random.default_rng(seed).permutation(self.n)
        return GeneCase(self.name + "/shuffled", [self.reads[i] for i in perm]), perm

    def features(self):
        """per read its feature, None where the record is not ASSIGNED (what dedup_per_gene takes)"""
        return [int(f) if fl & gn.ASSIGNED else None for f, fl in zip(self.recs["feature"].tolist(), self.recs["flags"].tolist())]

    def cells(self):
        return [None if c == NONE else c for c in self.cell.tolist()]


def rule(case, umi_len, umi_dist):
    """what the rule makes of the case, as the device's arrays -> (molecule code per read, group records sorted)"""
    return gn.checker_dedup_genes(case.cell, case.recs, case.umi, umi_len, umi_dist)


def from_umi_case(case, seed=1, stray=0.04):
    """a case of umi_cases.py: the cell ordinal is the rank's place among the cells; cell k's reads are dealt over 1 + k % 7
    features at random, so that one UMI (and UMIs one edit apart) meet in several genes of a cell; a few reads in a hundred carry
    a record that is not ASSIGNED, with the feature of an assigned neighbour"""
    rng = random.Random(seed)
    inside = {int(c): k for k, c in enumerate(case.cells.tolist())}
    reads = []
    for r, h, u in zip(case.rank.tolist(), case.has.tolist(), case.umi_text):
        k = inside.get(r) if h else None
        spread = 1 + (k or 0) % 7
        f = 11 * (k or 0) % 97 + rng.randrange(spread)
        reads.append((k, f, rng.choice(NOT_ASSIGNED) if rng.random() < stray else gn.ASSIGNED, u))
    return GeneCase(case.name + "/genes", reads)


def distinct_groups(n, seed, umi_len=12):
    """n reads that all take part, every (cell, feature) key different: the group table of 2^ceil(log2 2n) slots is as full as
    it gets (n = 512: 1,024 slots at load 0.5)"""
    rng = random.Random(seed)
    keys = set()
    while len(keys) < n:
        keys.add((rng.randrange(0, 5000), rng.randrange(0, 30000)))
    return GeneCase("groups%d_%d" % (n, seed), [(c, f, gn.ASSIGNED, uc._rand(rng, umi_len)) for c, f in sorted(keys, key=lambda k: rng.random())])


def hot_group(umi_len, n=20000, seed=5):
    """one group holding all the reads: UMIs over two letters (ties, chains), every fiftieth without a usable UMI"""
    rng = random.Random(100 * umi_len + seed)
    alphabet = "AC" if umi_len > 6 else "ACGT"
    reads = []
    for i in range(n):
        u = "N" * umi_len if i % 50 == 0 else uc._rand(rng, umi_len if rng.randrange(5) else umi_len + rng.choice((-1, 1)), alphabet)
        reads.append((3, 17, gn.ASSIGNED, u))
    return GeneCase("hot_group%d" % umi_len, reads)


def single_read_groups(n=3000, seed=6, umi_len=12):
    """n groups of one read each, all carrying one of three UMIs: nothing merges"""
    rng = random.Random(seed)
    umis = [uc._rand(rng, umi_len) for _ in range(3)]
    return GeneCase("singles%d" % n, [(i % 50, i // 50, gn.ASSIGNED, umis[i % 3] if i % 7 else "") for i in range(n)])


def extremes(umi_len=12):
    """features 0 and 0xFFFFFFFE and cell ordinals 0 and 0xFFFFFFFE in every combination, the same UMI family in each"""
    rng = random.Random(9)
    fam = uc._family(rng, umi_len)
    reads = []
    for c in (0, 0xFFFFFFFE):
        for f in (0, 0xFFFFFFFE):
            for u, k in fam.items():
                reads += [(c, f, gn.ASSIGNED, u)] * k
    rng.shuffle(reads)
    return GeneCase("extremes", reads)


A = gn.ASSIGNED
U, U1, W = "ACGTACGTAC", "ACGTACGTAG", "TTTTTGGGGG"          # U1 is U with its last letter changed; W is far from both
# every clause of the rule at umi_len 10, distance 1, with the answer derived by hand: (name, reads, molecule text per read (None:
# takes no part, '*': a molecule of its own), {(cell, feature): [molecules, umis, umi_reads, own]})
CLAUSES = [
    ("same UMI in two genes of one cell", [(0, 1, A, U), (0, 2, A, U)], [U, U], {(0, 1): [1, 1, 1, 0], (0, 2): [1, 1, 1, 0]}),
    ("one edit apart across genes", [(0, 1, A, U), (0, 1, A, U), (0, 2, A, U1)], [U, U, U1], {(0, 1): [1, 1, 2, 0], (0, 2): [1, 1, 1, 0]}),
    ("one edit apart inside a gene", [(0, 1, A, U), (0, 1, A, U), (0, 1, A, U1), (0, 1, A, W)], [U, U, U, W], {(0, 1): [2, 3, 4, 0]}),
    ("same UMI and gene in two cells", [(0, 1, A, U), (1, 1, A, U)], [U, U], {(0, 1): [1, 1, 1, 0], (1, 1): [1, 1, 1, 0]}),
    ("TIE, LOW and CROWDED take no part", [(0, 1, A, U), (0, 1, gn.TIE, U), (0, 1, gn.LOW, U), (0, 1, gn.CROWDED, U), (0, 1, gn.LOW | gn.TIE, U1),
                                           (0, 2, gn.TIE, W)], [U, None, None, None, None, None], {(0, 1): [1, 1, 1, 0]}),
    ("an unusable UMI is a molecule of its own", [(0, 1, A, U), (0, 1, A, "ACGTNCGTAC"), (0, 1, A, "ACGTACG"), (0, 1, A, "*"), (0, 1, A, "")],
     [U, "*", "*", "*", "*"], {(0, 1): [5, 1, 1, 4]}),
    ("a read without a cell takes no part", [(None, 1, A, U), (0, 1, A, U), (None, 2, A, W)], [None, U, None], {(0, 1): [1, 1, 1, 0]}),
]


def clause_case(k):
    name, reads, rows, stats = CLAUSES[k]
    return GeneCase(name, reads), rows, stats


def clause_arrays(k):
    """the hand-derived answer of clause k as the device's arrays"""
    _, reads, rows, stats = CLAUSES[k]
    mol = np.array([NONE if r is None or r == "*" else ud.umi_code(r) for r in rows], dtype=np.uint32)
    groups = np.array([(f, c) + tuple(s) for (c, f), s in sorted(stats.items())],
                      dtype=[("feature", "<u4"), ("cell", "<u4"), ("molecules", "<u4"), ("umis", "<u4"), ("umi_reads", "<u4"), ("own", "<u4")])
    return mol, groups


# ---- an independent form of the rule ----------------------------------------------------------------------------------------
def _levenshtein(a, b):
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        new = [i]
        for j, y in enumerate(b, 1):
            new.append(min(row[j] + 1, new[j - 1] + 1, row[j - 1] + (x != y)))
        row = new
    return row[-1]


def brute_force(cells, features, umis, umi_len, umi_dist):
    """the rule from its text, all pairs of a group compared: -> what dedup_per_gene returns"""
    groups, stats = {}, {}
    for c, f, u in zip(cells, features, umis):
        if c is None or f is None:
            continue
        s = stats.setdefault((c, f), [0, 0, 0, 0])
        if u is not None and abs(len(u) - umi_len) <= 2 and set(u) <= set("ACGT"):
            groups.setdefault((c, f), {}).setdefault(u, 0)
            groups[(c, f)][u] += 1
            s[2] += 1
        else:
            s[3] += 1
    root_of = {}
    for g, n in groups.items():
        rank = lambda u: (n[u], -len(u), [-"ACGT".index(x) for x in u])      # noqa: E731  (more reads, then the earlier UMI)
        parent = {}
        for b in n:
            cands = [a for a in n if a != b and _levenshtein(a, b) <= umi_dist and n[a] >= 2 * n[b] - 1 and rank(a) > rank(b)]
            if cands:
                parent[b] = max(cands, key=rank)
        for u in n:
            r = u
            while r in parent:
                r = parent[r]
            root_of[g + (u,)] = r
        stats[g][1] = len(n)
        stats[g][0] = sum(1 for u in n if root_of[g + (u,)] == u)
    for s in stats.values():
        s[0] += s[3]
    rows = []
    for c, f, u in zip(cells, features, umis):
        rows.append(None if c is None or f is None else root_of.get((c, f, u), "*"))
    return rows, stats


# ---- the accuracy condition -------------------------------------------------------------------------------------------------
def planted_cell(umi_len=10, molecules=5000, genes=2000, seed=2026):
    """one cell: `molecules` molecules of 1 .. 3 reads each, a random UMI and a gene drawn from `genes` for each
    -> (features per read, UMI texts per read, distinct (gene, UMI) pairs planted, planted pairs that have another pair of the
    same gene within one edit: what the rule may merge inside a gene)"""
    rng = random.Random(seed)
    feats, umis, planted = [], [], set()
    for _ in range(molecules):
        g, u = rng.randrange(genes), uc._rand(rng, umi_len)
        planted.add((g, u))
        for _ in range(rng.randint(1, 3)):
            feats.append(g)
            umis.append(u)
    by_gene = {}
    for g, u in planted:
        by_gene.setdefault(g, []).append(u)
    close = sum(1 for us in by_gene.values() for a in us if any(a != b and _levenshtein(a, b) <= 1 for b in us))
    return feats, umis, len(planted), close
