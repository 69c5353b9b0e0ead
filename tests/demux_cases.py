"""Inputs and a plain form of the clustering rule (badger_amd/donors.py, --donors) for the tests: the rule once more over
dictionaries and loops of Python integers, random cells with random assignments, and pools of planted haplotypes."""
import numpy as np

from badger_amd import donors as dn

MASK = (1 << 64) - 1


# ---------------------------------------------------------------- the plain form ----
def plain_best(r, a, tables):
    best = None
    for g in range(3):
        x = r * int(tables[2 * g]) + a * int(tables[5 + 2 * g])
        if best is None or x > best[0]:
            best = (x, g)
    return best[1]


def plain_pooled(cells, n_variants, tables):
    tot = {}
    for cell in cells:
        for v, r, a in cell:
            old = tot.get(v, (0, 0))
            tot[v] = (old[0] + r, old[1] + a)
    return [plain_best(*tot.get(v, (0, 0)), tables) for v in range(n_variants)]


def plain_counts(cells, z):
    """{(v, k): [R, Al]}"""
    out = {}
    for cell, k in zip(cells, z):
        for v, r, a in cell:
            pair = out.setdefault((v, int(k)), [0, 0])
            pair[0] += r
            pair[1] += a
    return out


def plain_loo(cells, z, gp, n_clusters, tables):
    """[cell][entry][k] -> g"""
    counts = plain_counts(cells, z)
    out = []
    for cell, zc in zip(cells, z):
        rows = []
        for v, r, a in cell:
            row = []
            for k in range(n_clusters):
                r1, a1 = counts.get((v, k), (0, 0))
                if k == int(zc):
                    r1, a1 = r1 - r, a1 - a
                row.append(gp[v] if r1 + a1 == 0 else plain_best(r1, a1, tables))
            rows.append(row)
        out.append(rows)
    return out


def plain_step(cells, z, gp, n_clusters, tables):
    """-> (z', L, changed, S)"""
    loo = plain_loo(cells, z, gp, n_clusters, tables)
    s, z1 = [], []
    for cell, rows in zip(cells, loo):
        row = [sum(r * int(tables[2 * g[k]]) + a * int(tables[5 + 2 * g[k]]) for (v, r, a), g in zip(cell, rows)) for k in range(n_clusters)]
        best = 0
        for k in range(1, n_clusters):
            if row[k] > row[best]:
                best = k
        s.append(row)
        z1.append(best)
    return z1, sum(row[k] for row, k in zip(s, z1)), sum(int(a != int(b)) for a, b in zip(z1, z)), s


def plain_words(cells, z, gp, n_clusters, tables):
    return [sum(g << (2 * k) for k, g in enumerate(row)) for rows in plain_loo(cells, z, gp, n_clusters, tables) for row in rows]


def plain_genotypes(cells, z, n_variants, n_clusters, tables):
    counts = plain_counts(cells, z)
    return [[plain_best(*counts[(v, k)], tables) if (v, k) in counts else dn.NO_GENOTYPE for v in range(n_variants)] for k in range(n_clusters)]


def plain_splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def plain_z0(seed, r, c, n_clusters):
    return plain_splitmix64((seed << 40) ^ (r << 32) ^ c) % n_clusters


# ---------------------------------------------------------------- random and planted inputs ----
def random_cells(rng, sizes, n_variants, high=4):
    """cells of the given numbers of entries, variants ascending inside a cell, ref + alt > 0, counts below `high`"""
    cells = []
    for m in sizes:
        vs = np.sort(rng.choice(n_variants, size=m, replace=False))
        ref, alt = rng.integers(0, high, size=m), rng.integers(0, high, size=m)
        ref = np.where(ref + alt == 0, 1, ref)
        cells.append(list(zip(vs.tolist(), ref.tolist(), alt.tolist())))
    return cells


def haplotype_cells(rng, genotypes, who, covered, error=0.02):
    """cells of the donors `who` (a donor per cell) of [variant][donor] genotypes: about `covered` variants per cell, 1 or 2
    molecules at each, each showing one of the donor's two alleles and the other allele with the chance `error`"""
    n_variants = len(genotypes)
    cells = []
    for d in who:
        cell = []
        for v in np.sort(rng.choice(n_variants, size=min(n_variants, covered), replace=False)).tolist():
            n = 1 + int(rng.random() < 0.3)
            alts = sum(int((rng.random() < genotypes[v][d] / 2) != (rng.random() < error)) for _ in range(n))
            cell.append((v, n - alts, alts))
        cells.append(cell)
    return cells


def counts_of(cells):
    """[[(variant, ref, alt)]] -> the dictionaries {(variant, cell): molecules} that a Demux is called with"""
    ref, alt = {}, {}
    for c, cell in enumerate(cells):
        for v, r, a in cell:
            if r:
                ref[(v, c)] = r
            if a:
                alt[(v, c)] = a
    return ref, alt
