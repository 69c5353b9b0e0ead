"""Inputs and a plain form of the donor rule (badger_amd/donors.py) for the tests: the rule once more over dictionaries and loops
of Python integers, random cells, cells whose winners sit at chosen places, and the planted pool of the accuracy condition."""
import numpy as np

from badger_amd import donors as dn

INT64_MIN = -(1 << 63)

# the tables at e = 0.01, by hand: p = 0.01, 0.255, 0.5, 0.745, 0.99; ln(0.99) 2^16 = -658.66, ln(0.745) 2^16 = -19291.9,
# ln(0.5) 2^16 = -45426.1, ln(0.255) 2^16 = -89554.4, ln(0.01) 2^16 = -301804.4
TABLES_001 = [-659, -19292, -45426, -89554, -301804, -301804, -89554, -45426, -19292, -659]

# one cell, two donors A and B, three entries.  Dosages at the variants 0, 1, 2: A 0, 2, 1; B 0, 0, 2.
#   entry (0, ref 3, alt 0), (1, ref 0, alt 2), (2, ref 1, alt 1)
#   A   levels 0, 4, 2:  3 A_0 + 2 B_4 + (A_2 + B_2) = -1977 - 1318 - 90852          = -94147
#   B   levels 0, 0, 4:  3 A_0 + 2 B_0 + (A_4 + B_4) = -1977 - 603608 - 302463       = -908048
#   A,B levels 0, 2, 3:  3 A_0 + 2 B_2 + (A_3 + B_3) = -1977 - 90852 - 108846        = -201675
# priors at pi = 0.1: P_s = rint(ln(0.45) 2^16) = rint(-52331.0) = -52331, P_d = rint(ln(0.1) 2^16) = rint(-150902.2) = -150902
#   T_s = -146478, T_s2 = -960379, T_d = -352577: singlet A, margin -146478 + 352577 = 206099 (3.145 in natural units)
HAND = dict(genotypes=[[0, 0], [2, 0], [1, 2]], cells=[[(0, 3, 0), (1, 0, 2), (2, 1, 1)]], scores=[[-94147, -908048, -201675]],
            record=(-94147, -908048, -201675, 0, 1, 0 | 1 << 16, 0), priors=(-52331, -150902), margin=206099)


def pack(genotypes):
    """[variant][donor] dosages -> uint64 word per variant"""
    return np.array([sum(int(g) << (2 * d) for d, g in enumerate(row)) for row in genotypes], dtype=np.uint64)


def flatten(cells):
    """[[(variant, ref, alt)]] -> (ENTRY_DTYPE, uint64 offsets)"""
    flat = [e for cell in cells for e in cell]
    out = np.zeros(len(flat), dtype=dn.ENTRY_DTYPE)
    if flat:
        out["variant"], out["ref"], out["alt"] = (np.array(x, dtype=np.uint32) for x in zip(*flat))
    return out, np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.uint64)


# ---------------------------------------------------------------- the plain form ----
def plain_scores(cells, genotypes, n_donors, tables):
    hyp = [(h, h) for h in range(n_donors)]
    for a in range(n_donors):
        for b in range(a + 1, n_donors):
            hyp.append((a, b))
    out = []
    for cell in cells:
        row = []
        for a, b in hyp:
            total = 0
            for v, ref, alt in cell:
                level = int(genotypes[v][a]) + int(genotypes[v][b])
                total += int(ref) * int(tables[level]) + int(alt) * int(tables[5 + level])
            row.append(total)
        out.append(row)
    return hyp, out


def plain_records(hyp, rows, n_donors):
    out = []
    for row in rows:
        best = second = pair = None
        for d in range(n_donors):
            if best is None or row[d] > row[best]:
                best = d
        for d in range(n_donors):
            if d != best and (second is None or row[d] > row[second]):
                second = d
        for h in range(n_donors, len(hyp)):
            if pair is None or row[h] > row[pair]:
                pair = h
        out.append((row[best], INT64_MIN if second is None else row[second], INT64_MIN if pair is None else row[pair], best,
                    dn.NONE if second is None else second, dn.NONE if pair is None else hyp[pair][0] | hyp[pair][1] << 16, 0))
    return out


# ---------------------------------------------------------------- random and placed cells ----
def random_genotypes(rng, n_variants, n_donors):
    return rng.integers(0, 3, size=(n_variants, n_donors))


def random_cells(rng, sizes, n_variants, high=6):
    """cells of the given numbers of entries, variants ascending inside a cell, ref + alt > 0, counts below `high`"""
    cells = []
    for m in sizes:
        vs = np.sort(rng.choice(n_variants, size=m, replace=False))
        ref, alt = rng.integers(0, high, size=m), rng.integers(0, high, size=m)
        ref = np.where(ref + alt == 0, 1, ref)
        cells.append(list(zip(vs.tolist(), ref.tolist(), alt.tolist())))
    return cells


def cell_of_levels(genotypes, donors, per_level=2):
    """the cell whose counts are what the donors (one, or a pair) make without errors: at every variant, per_level molecules per
    allele copy - level l of 4 gives alt = l * per_level, ref = (4 - l) * per_level (a singlet counts twice)"""
    a, b = donors if len(donors) == 2 else (donors[0], donors[0])
    return [(v, (4 - int(g[a]) - int(g[b])) * per_level, (int(g[a]) + int(g[b])) * per_level) for v, g in enumerate(genotypes)]


# ---------------------------------------------------------------- the planted pool ----
def planted_pool(seed, n_donors=8, n_variants=3000, singlets=500, doublets=100, covered=100, error=0.02, ambient=0.0):
    """a pool of donors with random genotypes (alt frequency of a variant uniform in 0.05 .. 0.5, dosage binomial), cells that cover
    about `covered` variants with 1 or 2 molecules each; a molecule comes from the cell's donor (of a doublet: either, evenly), or
    with the chance `ambient` from a random donor of the pool, shows one of that donor's two alleles, and the other allele with the
    chance `error` -> dict(genotypes [variant][donor], ref / alt {(variant, cell): molecules}, truth: per cell a tuple of one or two
    donors, n_cells)"""
    rng = np.random.default_rng(seed)
    freq = rng.uniform(0.05, 0.5, size=n_variants)
    genotypes = rng.binomial(2, freq[:, None], size=(n_variants, n_donors))
    truth = [(int(rng.integers(0, n_donors)),) for _ in range(singlets)]
    for _ in range(doublets):
        a, b = sorted(rng.choice(n_donors, size=2, replace=False).tolist())
        truth.append((a, b))
    ref, alt = {}, {}
    for c, who in enumerate(truth):
        for v in rng.choice(n_variants, size=min(n_variants, max(1, int(rng.poisson(covered)))), replace=False).tolist():
            for _ in range(1 + int(rng.random() < 0.3)):
                d = int(rng.integers(0, n_donors)) if rng.random() < ambient else who[int(rng.integers(0, len(who)))]
                is_alt = (rng.random() < genotypes[v, d] / 2) != (rng.random() < error)
                side = alt if is_alt else ref
                side[(v, c)] = side.get((v, c), 0) + 1
    return dict(genotypes=genotypes, ref=ref, alt=alt, truth=truth, n_cells=len(truth))


def genotype_lines(genotypes, ids, names):
    return ["variant\t%s\n" % "\t".join(names)] + ["%s\t%s\n" % (i, "\t".join(str(int(g)) for g in row)) for i, row in zip(ids, genotypes)]
