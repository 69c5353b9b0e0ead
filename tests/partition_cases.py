"""Inputs that reach every path of the bucket partition and the block scan (csrc/bdg_partition.hpp) through its consumers'
public entry points: the distinct count (bdg_distinct_dev), the deletion-variant joins (bdg_graph_edges, paths 5 and 6) and the
piece places of the chimera split (bdg_split_batch).  A helper module (imported like umi_cases.py), no test itself and no GPU:
tests/test_partition_cases.py checks that every generator delivers the property its case is named for, and
tests/test_partition_paths_gpu.py holds the device to numpy, the oracle and the Python split rule on them.

The launchers' geometry is restated here in plain functions, each constant with the place it is copied from.  Every case
carries `reaches()`: assertions, in numpy on the case's own input, that the input takes the path the case is for.  When a
constant moves in the source and is moved here, a case that no longer reaches its path fails there and says what it missed."""
import numpy as np

import split_cases as sc
from badger_amd import _native

# ---- csrc/distinct_kernels.hip
DS_CAP = 1024                    # DS_CAP: pairs a fine bucket should hold (bdg_distinct_launch sizes l1 and l2 by it)
DS_DCAP = 1536                   # DS_DCAP: different ranks k_distinct_buckets takes directly; more go to the cold path
DS_L1 = (8, 10)                  # bdg_distinct_launch: l1 = 8, raised to 10 while (n >> l1) > DS_CAP
DS_L2_MAX = 10                   # bdg_distinct_launch: l2_max of a call with two levels
DS_ROUND = 65536 // 8            # k_part_split<unsigned long long>: CHK = 64 KB of 8-byte entries a round
DS_TILE_ROWS = 256               # bdg_distinct_launch: per_tile is a multiple of k_distinct_rows' 256 threads,
DS_TILES_PER_CU = 8              # chosen so that there are about 8 tiles a compute unit
# ---- csrc/graph_deljoin.hip, csrc/dj_codec.hpp
DJ_ROUND = 65536 // 4            # k_part_split<uint32_t>: CHK = 64 KB of 4-byte entries a round
DJ_KEYBITS = {2: 28, 1: 30}      # a 14-mer (two deletions, thr 2) / a 15-mer (one deletion, thr 1)
DJ_PER_ROW_EST = {2: 72, 1: 12}  # per_row_est of bdg_graph_deljoin_launch (sizes rounds and l1)
DJ_PER_ROW = {2: 71, 1: 12}      # "about 71 entries per row on random barcodes", "about 12 of 16": the estimate used here
DJ_ROUND_ENTRIES = 1000000000    # D2_ROUND_ENTRIES
DJ_MUL_A, DJ_MUL_B = 0x9E3779B1, 0x85EBCA6B      # djc::mix
# ---- csrc/bdg_partition.hpp
SCAN_SPAN = 16384                # words a block of k_scan_blocks takes; bdg_split_launch: nblocks = ceil(n / SCAN_SPAN)

RANK_A16, RANK_T16 = 0, 0xFFFFFFFF               # sixteen A, sixteen T: the two values k_distinct_buckets uses for an empty slot


# ----------------------------------------------------------------------------- geometry, as the launchers compute it
def distinct_geometry(n, n_usable):
    """bdg_distinct_launch on n records (l1, two_levels) and k_part_bases on the n_usable pairs it finds (l2)"""
    l1 = DS_L1[0]
    while l1 < DS_L1[1] and (n >> l1) > DS_CAP:
        l1 += 1
    two_levels = (n >> l1) > DS_CAP
    l2 = 0
    while two_levels and l2 < DS_L2_MAX and (n_usable >> l2) > (1 << l1) * DS_CAP:
        l2 += 1
    return dict(l1=l1, two_levels=two_levels, l2=l2)


def distinct_tiles(n, cus):
    """bdg_distinct_launch: (per_tile, ntiles) of the two runs of k_distinct_rows on a device with `cus` compute units"""
    want = cus * DS_TILES_PER_CU
    per_tile = ((n + want - 1) // want + DS_TILE_ROWS - 1) // DS_TILE_ROWS * DS_TILE_ROWS
    return per_tile, (n + per_tile - 1) // per_tile


def join_geometry(n, thr, nparts=1):
    """bdg_graph_deljoin_launch: rounds and l1 of a call over n rows"""
    rounds = max(1, (n * DJ_PER_ROW_EST[thr] // nparts + DJ_ROUND_ENTRIES - 1) // DJ_ROUND_ENTRIES)
    est = n * DJ_PER_ROW_EST[thr] // (nparts * rounds) + 1
    fine_bits = 0
    while fine_bits < 24 and (est >> fine_bits) > 160:
        fine_bits += 1
    return dict(rounds=rounds, l1=min(12, fine_bits - 12) if fine_bits > 20 else 8)


def join_expected_per_bucket(n, thr):
    """entries a coarse bucket of the join expects: the mixed key spreads them evenly"""
    return n * DJ_PER_ROW[thr] / (1 << join_geometry(n, thr)["l1"])


def _mix(k, keybits):
    """djc::mix<keybits>: the one-to-one map of a variant whose top l1 bits name the entry's coarse bucket"""
    m = np.uint64((1 << keybits) - 1)
    x = (k.astype(np.uint64) * np.uint64(DJ_MUL_A)) & m
    x ^= x >> np.uint64(15)
    return (x * np.uint64(DJ_MUL_B)) & m


def _without(r, p):
    """r (letters of 2 bits, letter 0 lowest) without its letter p"""
    lo = r & np.uint64((1 << (2 * p)) - 1)
    return lo | ((r >> np.uint64(2 * p + 2)) << np.uint64(2 * p))


def join_bucket_sizes(ranks, thr):
    """the entries of every coarse bucket of a join over `ranks`, exactly: a row's entries are its DIFFERENT deletion variants
    (k_d1_rows: the 15-mers without one letter; d2_row: the 14-mers without two), an entry's bucket the top l1 bits of the
    variant's mixed key"""
    r = np.asarray(ranks).astype(np.uint64)
    if thr == 1:
        var = np.stack([_without(r, p) for p in range(16)], axis=1)
    else:
        var = np.stack([_without(_without(r, q), p) for p in range(16) for q in range(p + 1, 16)], axis=1)
    var.sort(axis=1)
    keep = np.ones(var.shape, bool)
    keep[:, 1:] = var[:, 1:] != var[:, :-1]
    kb, l1 = DJ_KEYBITS[thr], join_geometry(len(r), thr)["l1"]
    z = _mix(var[keep], kb)
    return np.bincount((z >> np.uint64(kb - l1)).astype(np.int64), minlength=1 << l1)


def scan_blocks(n):
    return (n + SCAN_SPAN - 1) // SCAN_SPAN


# ----------------------------------------------------------------------------- case group 1: the distinct count
class DistinctCase:
    """ranks of n records; `usable` records take part (valid, FLAG_RANK_OK | FLAG_BC16), `bc16_only` ones are valid with
    FLAG_BC16 alone (a 16-base barcode with a non-ACGT base: counted in d_n[1]), the rest are invalid"""

    def __init__(self, name, ranks, usable=None, bc16_only=None, reaches=None):
        self.name, self.ranks, self.n = name, np.ascontiguousarray(ranks, dtype=np.uint32), len(ranks)
        self.usable = np.ones(self.n, bool) if usable is None else usable
        self.bc16_only = np.zeros(self.n, bool) if bc16_only is None else bc16_only
        assert not (self.usable & self.bc16_only).any()
        self.geom = distinct_geometry(self.n, int(self.usable.sum()))
        self._reaches = reaches

    def __repr__(self):
        return "DistinctCase(%s, n = %d, %s)" % (self.name, self.n, self.geom)

    def records(self):
        """as _records_of of test_hip_parity.py, with the records that hold a 16-base barcode without a rank"""
        recs = np.zeros(self.n, dtype=_native.REC_DTYPE)
        recs["bc_rank"] = self.ranks
        recs["valid"] = self.usable | self.bc16_only
        recs["flags"] = np.where(self.usable, _native.FLAG_RANK_OK | _native.FLAG_BC16, np.where(self.bc16_only, _native.FLAG_BC16, 0))
        return recs

    def want(self):
        """numpy's answer: (distinct ranks ascending, counts, index of the first record of each, d_n[1])"""
        u, f, c = np.unique(self.ranks[self.usable], return_index=True, return_counts=True)
        return u, c, np.nonzero(self.usable)[0][f], int(self.bc16_only.sum())

    # what the kernels see
    def coarse_sizes(self):
        l1 = self.geom["l1"]
        return np.bincount(self.ranks[self.usable] >> np.uint32(32 - l1), minlength=1 << l1)

    def sub_sizes(self, bucket):
        """the sub-bucket sizes k_part_split counts in one coarse bucket"""
        l1, l2 = self.geom["l1"], self.geom["l2"]
        r = self.ranks[self.usable]
        r = r[(r >> np.uint32(32 - l1)) == bucket]
        return np.bincount((r >> np.uint32(32 - l1 - l2)) & np.uint32((1 << l2) - 1), minlength=1 << l2)

    def fine_distinct(self):
        """different ranks per fine bucket (the top l1 + l2 bits)"""
        bits = self.geom["l1"] + self.geom["l2"]
        u = np.unique(self.ranks[self.usable])
        return np.bincount(u >> np.uint32(32 - bits), minlength=1 << bits)

    def reaches(self):
        self._reaches(self)
        return self


ROUND_SIZES = (0, 1, DS_ROUND - 1, DS_ROUND, DS_ROUND + 1, 2 * DS_ROUND, 2 * DS_ROUND + 1, 3 * DS_ROUND + 1)
# which coarse bucket (of 1,024) gets which of the sizes; the first and the last bucket span rounds too
_ROUND_AT = {5: 0, 1: 1, 2: DS_ROUND - 1, 3: DS_ROUND, 4: DS_ROUND + 1, 6: 2 * DS_ROUND, 700: 2 * DS_ROUND + 1, 1022: 3 * DS_ROUND + 1,
             0: DS_ROUND + 1, 1023: 2 * DS_ROUND + 1}
_ROUND_HUGE, _ROUND_ONE_SUB, _ROUND_SPREAD = 512, 700, 1022


def _pool_draw(rng, pool, k):
    return pool[rng.integers(0, len(pool), k)]


def _rounds_case(name, n, l2, others, seed):
    """n usable records in 1,024 coarse buckets whose sizes are set through the top 10 bits (_ROUND_AT, `others` entries in every
    other bucket, the rest in bucket _ROUND_HUGE); inside a bucket the low 22 bits come from a small pool of values"""
    rng = np.random.default_rng(seed)
    sizes = np.full(1024, others, np.int64)
    for b, c in _ROUND_AT.items():
        sizes[b] = c
    sizes[_ROUND_HUGE] = 0
    sizes[_ROUND_HUGE] = n - sizes.sum()
    parts = []
    for b in range(1024):
        c = int(sizes[b])
        pool = rng.integers(0, 1 << 22, 3000 << l2 if b == _ROUND_HUGE else 1000, dtype=np.uint64).astype(np.uint32)
        low = _pool_draw(rng, pool, c)
        if l2 == 2 and b == _ROUND_ONE_SUB:                 # every entry in sub-bucket 2 of 4
            low = (low & np.uint32(0xFFFFF)) | np.uint32(2 << 20)
        if l2 == 2 and b == _ROUND_SPREAD:                  # 1 / 0 / all others / 1
            sub = np.full(c, 2, np.uint32)
            sub[0], sub[1] = 0, 3
            low = (low & np.uint32(0xFFFFF)) | (sub << np.uint32(20))
        if b == 0 and c:
            low[:100] = 0                                   # sixteen A, a hundred times
        if b == 1023 and c:
            low[:100] = 0x3FFFFF                            # sixteen T
        parts.append(np.uint32(b << 22) | low)
    ranks = np.concatenate(parts)
    rng.shuffle(ranks)

    def reaches(c):
        assert c.n == n and c.geom == dict(l1=10, two_levels=True, l2=l2), c.geom
        got = c.coarse_sizes()
        for b, want in _ROUND_AT.items():
            assert got[b] == want, ("coarse bucket", b, int(got[b]), want)
        assert set(ROUND_SIZES) <= set(got.tolist()) and got[0] > DS_ROUND and got[1023] > DS_ROUND
        assert got[_ROUND_HUGE] == got.max() >= 200000, int(got[_ROUND_HUGE])
        for b in (0, 3, 4, 6, _ROUND_HUGE):                 # more than one sub-bucket holds entries: a round is regrouped
            assert (c.sub_sizes(b) > 0).sum() > 1, b
        if l2 == 2:
            assert c.sub_sizes(_ROUND_ONE_SUB).tolist() == [0, 0, 2 * DS_ROUND + 1, 0]
            assert c.sub_sizes(_ROUND_SPREAD).tolist() == [1, 0, 3 * DS_ROUND - 1, 1]
        d = c.fine_distinct()
        huge = d[_ROUND_HUGE << l2:(_ROUND_HUGE + 1) << l2]
        assert huge.max() > DS_DCAP and huge.max() <= 4 * DS_DCAP, huge       # the cold path, one step deep
        assert np.delete(d, np.arange(_ROUND_HUGE << l2, (_ROUND_HUGE + 1) << l2)).max() <= DS_DCAP
        counts = dict(zip(*np.unique(c.ranks, return_counts=True)))
        assert counts[RANK_A16] >= 100 and counts[RANK_T16] >= 100

    return DistinctCase(name, ranks, reaches=reaches)


def _no_sub_buckets_case():
    """two levels by the number of records, but so few usable ones that k_part_bases picks l2 = 0: k_part_split runs with
    nb2 = 1 and mask = 0"""
    n = 1049600
    rng = np.random.default_rng(77)
    ranks = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    pool = rng.integers(0, 1 << 22, 1000, dtype=np.uint64).astype(np.uint32)
    at = rng.choice(n, 20000, replace=False)
    ranks[at] = np.uint32(333 << 22) | _pool_draw(rng, pool, len(at))
    off = rng.random(n) < 0.03
    bc16 = off & (rng.random(n) < 0.5)

    def reaches(c):
        assert c.geom == dict(l1=10, two_levels=True, l2=0), c.geom
        assert int(c.usable.sum()) <= (1 << 10) * DS_CAP < c.n
        got = c.coarse_sizes()
        assert got[333] > 2 * DS_ROUND and (got > DS_ROUND).sum() == 1
        assert c.bc16_only.sum() > 10000 and (~c.usable & ~c.bc16_only).sum() > 10000
        assert np.delete(c.fine_distinct(), 333).max() <= DS_DCAP

    return DistinctCase("second_level_without_sub_buckets", ranks, ~off, bc16, reaches)


def _sentinel_cases():
    rng = np.random.default_rng(78)
    out = []

    def single_level(c):
        assert c.geom == dict(l1=8, two_levels=False, l2=0), c.geom

    # both among random ranks
    ranks = np.concatenate([rng.integers(0, 1 << 32, 4800, dtype=np.uint64).astype(np.uint32),
                            np.full(100, RANK_A16, np.uint32), np.full(100, RANK_T16, np.uint32)])
    rng.shuffle(ranks)

    def among(c):
        single_level(c)
        assert c.n == 5000 and (c.ranks == RANK_A16).sum() >= 100 and (c.ranks == RANK_T16).sum() >= 100
        assert c.fine_distinct().max() <= DS_DCAP
    out.append(DistinctCase("sentinels/among_random", ranks, reaches=among))

    # a cold-path bucket under the all-ones prefix (its empty slot is 0), with rank 0 in the call
    ranks = np.concatenate([np.uint32(0xFFFFF000) | rng.integers(0, 1 << 12, 30000).astype(np.uint32), np.full(50, RANK_A16, np.uint32)])
    rng.shuffle(ranks)

    def ones(c):
        single_level(c)
        d = c.fine_distinct()
        assert d[255] > 2 * DS_DCAP and d[0] == 1 and (c.ranks == RANK_T16).any() and (c.ranks == RANK_A16).sum() == 50
    out.append(DistinctCase("sentinels/cold_under_all_ones", ranks, reaches=ones))

    # and the mirror image: a cold-path bucket under the prefix 0 (it holds rank 0), with rank 0xFFFFFFFF in the call
    ranks = np.concatenate([rng.integers(0, 1 << 12, 30000).astype(np.uint32), np.full(50, RANK_T16, np.uint32)])
    rng.shuffle(ranks)

    def zeros(c):
        single_level(c)
        d = c.fine_distinct()
        assert d[0] > 2 * DS_DCAP and d[255] == 1 and (c.ranks == RANK_A16).any() and (c.ranks == RANK_T16).sum() == 50
    out.append(DistinctCase("sentinels/cold_under_zero", ranks, reaches=zeros))
    return out


CAPACITY_EDGE = [(0x5A, DS_DCAP - 1), (0x5A, DS_DCAP), (0x5A, DS_DCAP + 1), (0xFF, DS_DCAP), (0xFF, DS_DCAP + 1)]


def _capacity_case(prefix, different):
    """`different` ranks that share their top 8 bits (one fine bucket of a single-level call), each 1 to 5 times, shuffled"""
    rng = np.random.default_rng(1000 * prefix + different)
    low = rng.choice(1 << 24, different, replace=False).astype(np.uint32)
    ranks = np.repeat(np.uint32(prefix << 24) | low, rng.integers(1, 6, different))
    rng.shuffle(ranks)

    def reaches(c):
        assert c.geom == dict(l1=8, two_levels=False, l2=0), c.geom
        d = c.fine_distinct()
        assert d[prefix] == different == d.sum()
        k = np.unique(c.ranks, return_counts=True)[1]
        assert k.min() == 1 and k.max() == 5

    return DistinctCase("capacity_edge/%02x/%d" % (prefix, different), ranks, reaches=reaches)


def tile_edge_sizes(cus):
    """record counts either side of a tile of k_distinct_rows and of the last of all tiles"""
    full = DS_TILE_ROWS * DS_TILES_PER_CU * cus
    return [1, DS_TILE_ROWS - 1, DS_TILE_ROWS, DS_TILE_ROWS + 1, full - 1, full, full + 1]


def _tile_case(n, cus):
    rng = np.random.default_rng(n)
    pool = rng.integers(0, 1 << 32, max(1, n // 3), dtype=np.uint64).astype(np.uint32)
    per_tile, ntiles = distinct_tiles(n, cus)
    full = DS_TILE_ROWS * DS_TILES_PER_CU * cus

    def reaches(c):
        assert not c.geom["two_levels"]
        if n <= DS_TILE_ROWS:
            assert (per_tile, ntiles) == (DS_TILE_ROWS, 1)
        elif n < full - 1:
            assert (per_tile, ntiles) == (DS_TILE_ROWS, 2) and n == DS_TILE_ROWS + 1                 # one record in the second tile
        elif n <= full:
            assert (per_tile, ntiles) == (DS_TILE_ROWS, full // DS_TILE_ROWS) and ntiles * per_tile - n == full - n
        else:
            assert per_tile == 2 * DS_TILE_ROWS and n - (ntiles - 1) * per_tile == 1                 # one record in the last tile
        assert n < 3 or len(np.unique(c.ranks)) < n

    return DistinctCase("tile_edges/%d" % n, _pool_draw(rng, pool, n), reaches=reaches)


DISTINCT_NAMES = ["rounds", "rounds_l2_2", "second_level_without_sub_buckets", "sentinels/among_random", "sentinels/cold_under_all_ones",
                  "sentinels/cold_under_zero"] + ["capacity_edge/%02x/%d" % pd for pd in CAPACITY_EDGE]
_DISTINCT = {}


def distinct_case(name, cus=None):
    """a case of DISTINCT_NAMES, or "tile_edges/<n>" with the device's compute units; built once"""
    key = (name, cus)
    if key not in _DISTINCT:
        if name == "rounds":
            c = _rounds_case(name, 1200000, 1, 700, 71)
        elif name == "rounds_l2_2":
            c = _rounds_case(name, 2200000, 2, 1500, 72)
        elif name == "second_level_without_sub_buckets":
            c = _no_sub_buckets_case()
        elif name.startswith("sentinels/"):
            for s in _sentinel_cases():
                _DISTINCT[(s.name, cus)] = s
            c = _DISTINCT[key]
        elif name.startswith("capacity_edge/"):
            c = _capacity_case(int(name.split("/")[1], 16), int(name.split("/")[2]))
        else:
            c = _tile_case(int(name.split("/")[1]), cus)
        _DISTINCT[key] = c
    return _DISTINCT[key]


def small_records():
    """a small call between two large ones (the workspace is reused, not grown): 300 records, 40 different ranks"""
    rng = np.random.default_rng(5)
    return DistinctCase("small", _pool_draw(rng, rng.integers(0, 1 << 32, 40, dtype=np.uint64).astype(np.uint32), 300), rng.random(300) < 0.9)


# ----------------------------------------------------------------------------- case group 2: the deletion-variant joins
JOIN_ROWS = {2: 70000, 1: 400000}        # the smallest round numbers whose coarse buckets pass a round by 10 % (join_expected_per_bucket)
JOIN_ALGO = {2: 5, 1: 6}                 # bdg_graph_set_algo: the join forced


class JoinCase:
    def __init__(self, name, thr, ranks):
        self.name, self.thr, self.ranks, self.n, self.algo = name, thr, ranks, len(ranks), JOIN_ALGO[thr]

    def __repr__(self):
        return "JoinCase(%s, thr %d, %d rows)" % (self.name, self.thr, self.n)

    def reaches(self):
        assert self.n == JOIN_ROWS[self.thr] and (np.diff(self.ranks.astype(np.int64)) > 0).all()
        assert join_geometry(self.n, self.thr) == dict(rounds=1, l1=8)
        # the condition on the input: by the estimate of entries per row a coarse bucket passes one round by 10 % at least
        assert join_expected_per_bucket(self.n, self.thr) >= 1.1 * DJ_ROUND, join_expected_per_bucket(self.n, self.thr)
        # and counted: every coarse bucket is streamed in two rounds, the second partial
        self.sizes = join_bucket_sizes(self.ranks, self.thr)
        assert DJ_ROUND < self.sizes.min() and self.sizes.max() < 2 * DJ_ROUND, (int(self.sizes.min()), int(self.sizes.max()))
        return self


_JOIN = {}


def join_case(thr, kind):
    """kind "random": JOIN_ROWS[thr] distinct random ranks, ascending.  kind "neighbours": half as many random ranks and, of
    each, a copy with one letter substituted - every row has an edge, so that entries all over every bucket decide one"""
    if (thr, kind) not in _JOIN:
        n = JOIN_ROWS[thr]
        rng = np.random.default_rng(100 * thr + len(kind))
        r = rng.integers(0, 1 << 32, n + 1000 if kind == "random" else n // 2 + 500, dtype=np.uint64).astype(np.uint32)
        if kind == "neighbours":
            r = np.concatenate([r, r ^ (rng.integers(1, 4, len(r)).astype(np.uint32) << (2 * rng.integers(0, 16, len(r))).astype(np.uint32))])
        r = np.unique(r)
        _JOIN[(thr, kind)] = JoinCase("%s/thr%d" % (kind, thr), thr, np.sort(rng.choice(r, n, replace=False)))
    return _JOIN[(thr, kind)]


# ----------------------------------------------------------------------------- case group 3: the piece places of the split
SPLIT_READS = 2 * SCAN_SPAN + 5
SPLIT_EVERY = 997
# reads of a call -> blocks of its scan.  With SCAN_SPAN + 1 reads the second block holds one read, whose place is still a sum of the
# first block; read SCAN_SPAN + 1 is the first whose place needs what k_scan_add adds
SPLIT_SIZES = {SPLIT_READS: 3, SCAN_SPAN: 1, SCAN_SPAN + 1: 2, SCAN_SPAN + 2: 2}


class SplitCase:
    def __init__(self, n, seed=31):
        """n reads, nearly all of ten bases (one piece each, never scanned); concatemers of 3 to 5 molecules on either side of
        every border between two blocks of the scan, at both ends, and at every 997th read (so that the blocks' sums differ)"""
        rng = np.random.default_rng(seed + n)
        self.n = n
        edges = [0, n - 1] + [b * SCAN_SPAN + d for b in range(1, scan_blocks(n) + 1) for d in (-1, 0, 1)]
        self.at = sorted({i for i in edges + list(range(SPLIT_EVERY, n, SPLIT_EVERY)) if 0 <= i < n})
        self.edges = sorted({i for i in edges if 0 <= i < n})
        short = rng.integers(0, 4, (n, 10))
        reads = ["".join("ACGT"[c] for c in row) for row in short]
        for i in self.at:
            reads[i] = sc.concatemer(rng, int(rng.integers(3, 6)))[0]
        self.reads = reads

    def __repr__(self):
        return "SplitCase(%d reads, %d concatemers)" % (self.n, len(self.at))

    def reaches(self, pieces):
        """pieces: the rule's piece records for these reads"""
        per_read = np.bincount(pieces["read"], minlength=self.n)
        nblocks = scan_blocks(self.n)
        assert nblocks == (self.n + SCAN_SPAN - 1) // SCAN_SPAN
        for b in range(nblocks):                            # reads with more than one piece in every block of the scan
            assert (per_read[b * SCAN_SPAN:(b + 1) * SCAN_SPAN] > 1).any(), b
        for i in self.edges:
            assert per_read[i] >= 3, (i, int(per_read[i]))
        assert (per_read[np.setdiff1d(np.arange(self.n), self.at)] == 1).all()
        assert len(pieces) > self.n
        sums = [int(per_read[b * SCAN_SPAN:(b + 1) * SCAN_SPAN].sum()) for b in range(nblocks)]
        assert nblocks < 3 or len(set(sums)) == nblocks, sums
        return nblocks


_SPLIT = {}


def split_case(n):
    if n not in _SPLIT:
        _SPLIT[n] = SplitCase(n)
    return _SPLIT[n]
