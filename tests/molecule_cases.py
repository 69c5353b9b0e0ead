"""Inputs for bdg_molecule_reps_dev (csrc/umi_kernels.hip: k_mol_insert, k_mol_reads) built where the kernels can go wrong:
sizes around a wave, one molecule holding every read, ties at the longest cDNA (inside a wave and across a wave boundary),
molecules without any cDNA, lengths that need the election word's upper 32 bits in full, reads that belong to no molecule, one
molecule code in two cells, and all-distinct keys that fill half of a 1,024- or 2,048-slot table.  A helper module (imported like
umi_cases.py), no test itself: tests/test_molecule_reads.py checks without a GPU that every generator delivers what it is for,
tests/test_molecule_reads_gpu.py holds the device against the rule (badger_amd/molecule_reads.py) on them."""
import numpy as np

from badger_amd import molecule_reads as mr

NONE = mr.NONE
WAVE = 64


class Case:
    def __init__(self, name, cells, rank, has, mol, length):
        self.name = name
        self.cells = np.array(sorted({int(c) for c in cells}), dtype=np.uint32)
        self.rank = np.asarray(rank, dtype=np.uint32)
        self.has = np.asarray(has, dtype=np.uint8)
        self.mol = np.asarray(mol, dtype=np.uint32)
        self.length = np.asarray(length, dtype=np.uint32)
        self.n = len(self.rank)
        assert len(self.has) == len(self.mol) == len(self.length) == self.n

    def __repr__(self):
        return "Case(%s, %d reads, %d cells)" % (self.name, self.n, len(self.cells))

    def rule(self):
        """-> (rep uint8 [n], mol_reads uint32 [n]) by the checker"""
        return mr.molecule_reps(self.rank, self.has, self.mol, self.length, self.cells)

    def shuffled(self, seed):
        """the same reads in another order -> (Case, perm) with new read i = old read perm[i]"""
        perm = np.random.default_rng(seed).permutation(self.n)
        return Case(self.name + "/shuffled", self.cells, self.rank[perm], self.has[perm], self.mol[perm], self.length[perm]), perm

    def groups(self):
        """the molecules as lists of read indices, from a plain dictionary (not from the checker)"""
        inside = {int(c) for c in self.cells}
        out = {}
        for i in range(self.n):
            if self.has[i] and int(self.rank[i]) in inside and int(self.mol[i]) != NONE:
                out.setdefault((int(self.rank[i]), int(self.mol[i])), []).append(i)
        return out


def code(rng, length=12):
    """a random UMI code of `length` letters (bdg_extract_keep_umis' packing)"""
    return length << 28 | int(rng.integers(0, 1 << (2 * length)))


def _cells(rng, k):
    out = set()
    while len(out) < k:
        out.add(int(rng.integers(1, 0xFFFFFFFF)))
    return sorted(out)


def mixed(n, seed):
    """n reads over a few cells and few molecule codes (molecules of several reads, the same code in several cells), about one
    read in ten each without a cell, with a rank that is no cell, without a molecule; a fifth without cDNA; lengths from a
    small range (ties) and a few from 2^16 on"""
    rng = np.random.default_rng(seed)
    cells = _cells(rng, max(1, min(12, n // 8)))
    strangers = _cells(rng, 3)
    codes = [code(rng, int(rng.integers(10, 15))) for _ in range(max(1, n // 40))]
    rank = np.array([cells[int(rng.integers(0, len(cells)))] for _ in range(n)], dtype=np.uint32)
    u = rng.random(n)
    rank[u < 0.1] = [strangers[int(x)] for x in rng.integers(0, 3, size=int((u < 0.1).sum()))]
    has = (rng.random(n) >= 0.1).astype(np.uint8)
    mol = np.array([codes[int(rng.integers(0, len(codes)))] for _ in range(n)], dtype=np.uint32)
    mol[rng.random(n) < 0.1] = NONE
    length = rng.integers(1, 6, size=n).astype(np.uint32) * 100
    big = rng.random(n) < 0.05
    length[big] = rng.integers(1 << 16, 1 << 20, size=int(big.sum()))
    length[rng.random(n) < 0.2] = 0
    return Case("mixed_%d" % n, [c for c in cells if c not in strangers], rank, has, mol, length)


def one_molecule(n, seed=1):
    """every read in one molecule; a third without cDNA, the others of five lengths, so the longest is shared by thousands"""
    rng = np.random.default_rng(seed)
    cells = _cells(rng, 5)
    length = rng.integers(0, 6, size=n).astype(np.uint32) * 77
    length[rng.random(n) < 0.33] = 0
    return Case("one_molecule_%d" % n, cells, np.full(n, cells[2]), np.ones(n), np.full(n, code(rng)), length)


def wave_ties(seed=2, n=1024):
    """every read alone in its molecule, except planted groups whose longest cDNA is shared by two or three reads: neighbours
    inside a wave, the last lane of a wave and the first of the next, lanes far apart in one wave, reads of different blocks;
    each group also holds a shorter read behind the tied ones and one without cDNA in front of them where there is room"""
    rng = np.random.default_rng(seed)
    cells = _cells(rng, 4)
    rank = np.array([cells[i % 4] for i in range(n)], dtype=np.uint32)
    mol = np.array([12 << 28 | i for i in range(n)], dtype=np.uint32)              # all distinct
    length = rng.integers(1, 1000, size=n).astype(np.uint32)
    groups = [(10, 11), (63, 64), (62, 65), (127, 128), (130, 191), (192, 255, 256), (255, 256), (300, 700), (511, 512, 513),
              (639, 640), (5, 900), (767, 768, 1000)]
    taken = set()
    planted = []
    for g, tied in enumerate(groups):
        tied = [t for t in tied if t not in taken]
        if len(tied) < 2:
            continue
        extra = [x for x in (tied[0] - 2, tied[-1] + 3) if 0 <= x < n and x not in taken and x not in tied]
        members = tied + extra
        taken.update(members)
        key = 13 << 28 | (7000 + g)
        for x in members:
            rank[x], mol[x] = cells[g % 4], key
        length[tied] = 5000 + g
        if extra:
            length[extra[-1]] = 4999 + g                              # a shorter read behind the tie
            if len(extra) == 2:
                length[extra[0]] = 0                                  # a read without cDNA in front of it
        planted.append((tied, extra))
    case = Case("wave_ties", cells, rank, np.ones(n), mol, length)
    case.planted = planted
    return case


def no_cdna(seed=3, n=600):
    """molecules of 1 .. 9 reads, half of them without any cDNA (no representative, but counted)"""
    rng = np.random.default_rng(seed)
    cells = _cells(rng, 6)
    rank, mol, length = [], [], []
    m = 0
    while len(rank) < n:
        k, c, u = int(rng.integers(1, 10)), cells[int(rng.integers(0, 6))], 11 << 28 | m
        empty = m % 2 == 0
        for _ in range(k):
            rank.append(c); mol.append(u); length.append(0 if empty else int(rng.integers(0, 3)) * 50)
        m += 1
    order = rng.permutation(len(rank))
    return Case("no_cdna", cells, np.array(rank)[order], np.ones(len(rank)), np.array(mol, dtype=np.uint32)[order], np.array(length)[order])


def long_lengths(seed=4, n=500):
    """lengths at 2^16 - 1, 2^16, 2^16 + 1, 2^31 and 2^32 - 1 beside short ones, in molecules of about ten reads with ties"""
    rng = np.random.default_rng(seed)
    cells = _cells(rng, 3)
    pool = np.array([65535, 65536, 65537, 1 << 31, 0xFFFFFFFF, 300, 0], dtype=np.uint64)
    length = pool[rng.integers(0, len(pool), size=n)]
    rank = np.array([cells[int(x)] for x in rng.integers(0, 3, size=n)], dtype=np.uint32)
    mol = (np.uint32(12 << 28) | rng.integers(0, n // 30 + 1, size=n).astype(np.uint32))
    return Case("long_lengths", cells, rank, np.ones(n), mol, length)


def two_cells_one_code(seed=5):
    """one molecule code in two cells (and in a rank that is no cell): two molecules, each with its own count and read"""
    rng = np.random.default_rng(seed)
    a, b, stranger = _cells(rng, 3)
    u = code(rng)
    rank = [a, b, a, b, b, stranger, a, b]
    length = [10, 10, 30, 5, 40, 99, 30, 40]
    return Case("two_cells_one_code", [a, b], rank, np.ones(8), np.full(8, u), length)


def distinct_keys(n, seed, n_cells=3):
    """n reads, every one its own molecule (all keys distinct): 512 reads fill half of a 1,024-slot table, 1,024 half of a
    2,048-slot one"""
    rng = np.random.default_rng(seed)
    cells = _cells(rng, n_cells)
    keys = set()
    while len(keys) < n:
        keys.add((int(rng.integers(0, n_cells)), code(rng)))
    keys = sorted(keys)
    order = rng.permutation(n)
    rank = np.array([cells[keys[i][0]] for i in order], dtype=np.uint32)
    mol = np.array([keys[i][1] for i in order], dtype=np.uint32)
    return Case("distinct_%d_%d" % (n, seed), cells, rank, np.ones(n), mol, rng.integers(0, 4, size=n).astype(np.uint32) * 9)


def slot_of(keys, mask):
    """slot_of of csrc/umi_kernels.hip (the 64-bit mix), on a uint64 array"""
    k = keys.astype(np.uint64)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xff51afd7ed558ccd)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xc4ceb9fe1a85ec53)
    k = k ^ (k >> np.uint64(33))
    return (k & np.uint64(0xFFFFFFFF)).astype(np.uint32) & np.uint32(mask)


def occupied(case, P):
    """the slots linear probing fills with the case's distinct keys (the same set in any insertion order), and how many keys
    sit below their home slot: they went past the last slot"""
    ok, key = mr.members(case.rank, case.has, case.mol, case.cells)
    keys = np.unique(key[ok])
    used = np.zeros(P, bool)
    wrapped = 0
    for h in slot_of(keys, P - 1).tolist():
        s = h
        while used[s]:
            s = (s + 1) & (P - 1)
        used[s] = True
        wrapped += s < h
    return used, wrapped


GENERATORS = {
    "mixed_1": lambda: mixed(1, 101), "mixed_63": lambda: mixed(63, 163), "mixed_64": lambda: mixed(64, 164),
    "mixed_65": lambda: mixed(65, 165), "mixed_4097": lambda: mixed(4097, 197),
    "wave_ties": wave_ties, "no_cdna": no_cdna, "long_lengths": long_lengths, "two_cells_one_code": two_cells_one_code,
}

_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = GENERATORS[name]()
    return _CASES[name]
