"""The clustering kernels (csrc/demux_kernels.hip) against the rule of badger_amd/donors.py, exactly: one iteration through
bdg_donor_cluster_counts_dev and bdg_donor_cluster_assign_dev (the count table, S, z', L and changed), the words and the clusters'
genotypes through bdg_donor_cluster_words_dev, and the whole fit through bdg_donor_cluster.  1, 2, 3, 31 and 32 clusters; cells of
0, 1, 2, 63, 64, 65 and 129 entries (the chunk border and the odd tail of the two-entries-a-step walk); 1, 2 and 3,000 cells; one
variant that every cell of one cluster shares; a pair that holds 2^31; winners in lane 0, lane K - 1 and in the upper half's
partner lanes; a cell alone in its cluster; the ties; every argument error over poisoned outputs, with nothing launched."""
import ctypes as C

import numpy as np
import pytest

import demux_cases as mc
import donor_cases as dc
from badger_amd import _native
from badger_amd import donors as dn

pytestmark = pytest.mark.gpu

CLUSTERS = (1, 2, 3, 31, 32)
BORDERS = [0, 1, 2, 63, 64, 65, 129]
POISON = 0xAB
T = dc.TABLES_001


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _poisoned(n_bytes):
    return np.full(n_bytes + 16, POISON, np.uint8)


def _iteration(ctx, cells, z, n_variants, n_clusters, tables, what=""):
    """counts, assign and words over device arrays, every output poisoned first and 16 bytes longer than it need be, against
    the checker -> (z', L, changed) of the checker"""
    entries, off = dc.flatten(cells)
    z = np.asarray(z, dtype=np.uint32)
    n, k, e = len(cells), n_clusters, len(entries)
    gp = dn.pooled_genotypes(entries, n_variants, tables)
    sizes = dict(counts=8 * n_variants * k, z_out=4 * n, scores=8 * n * k, sums=16, words=8 * e, geno=n_variants * k)
    d_in = [_native.DeviceArray.from_host(ctx, a) for a in (entries.view(np.uint32) if e else np.zeros(4, np.uint32), off, z, gp)]
    d_out = {name: _native.DeviceArray.from_host(ctx, _poisoned(b)) for name, b in sizes.items()}
    try:
        ctx.donor_cluster_counts_dev(d_in[0], d_in[1], n, d_in[2], n_variants, k, d_out["counts"])
        ctx.donor_cluster_assign_dev(d_in[0], d_in[1], n, d_in[2], d_in[3], n_variants, k, tables, d_out["counts"], d_out["z_out"],
                                     d_out["sums"], d_out["scores"])
        ctx.donor_cluster_words_dev(d_in[0], d_in[1], n, d_in[2], d_in[3], n_variants, k, tables, d_out["counts"], d_out["words"],
                                    d_out["geno"])
        ctx.synchronize()
        got = {name: d.to_host() for name, d in d_out.items()}
    finally:
        for d in d_in + list(d_out.values()):
            d.free()
    for name, b in sizes.items():
        assert (got[name][b:] == POISON).all(), (what, name, "written behind its end")
    r, al = dn.cluster_counts(entries, off, z, n_variants, k)
    counts = got["counts"][:sizes["counts"]].view(np.uint32).reshape(n_variants, k, 2)
    assert counts[:, :, 0].tolist() == r.tolist() and counts[:, :, 1].tolist() == al.tolist(), (what, "counts")
    z1, total, changed, s = dn.cluster_step(entries, off, z, gp, k, tables)
    assert got["scores"][:sizes["scores"]].view(np.int64).reshape(n, k).tolist() == s.tolist(), (what, "S")
    assert got["z_out"][:sizes["z_out"]].view(np.uint32).tolist() == z1.tolist(), (what, "z'")
    assert got["sums"][:16].view(np.int64).tolist() == [total, changed], (what, "L, changed")
    assert got["words"][:sizes["words"]].view(np.uint64).tolist() == dn.entry_words(entries, off, z, gp, k, tables).tolist(), (what, "words")
    assert got["geno"][:sizes["geno"]].reshape(k, n_variants).tolist() == dn.cluster_genotypes(entries, off, z, n_variants, k, tables).tolist(), \
        (what, "G")
    return z1, total, changed


def test_dtypes_are_the_checkers():
    assert _native.CLUSTER_RESTART_DTYPE == dn.RESTART_DTYPE and _native.CLUSTER_RESTART_DTYPE.itemsize == 16
    assert _native.CLUSTER_NO_GENOTYPE == dn.NO_GENOTYPE


@pytest.mark.parametrize("n_clusters", CLUSTERS)
def test_chunk_borders(ctx, n_clusters):
    rng = np.random.default_rng(900 + n_clusters)
    sizes = BORDERS + BORDERS[::-1]
    cells = mc.random_cells(rng, sizes, 200)
    _iteration(ctx, cells, rng.integers(0, n_clusters, size=len(cells)), 200, n_clusters, dn.level_tables(0.02))
    for size in BORDERS:                                                      # one cell, then two
        _iteration(ctx, mc.random_cells(rng, [size], 200), [n_clusters - 1], 200, n_clusters, dn.level_tables(0.01), "one cell of %d" % size)
    _iteration(ctx, mc.random_cells(rng, [65, 2], 200), [0, n_clusters - 1], 200, n_clusters, dn.level_tables(0.2), "two cells")


@pytest.mark.parametrize("n_clusters", (3, 32))
def test_many_cells(ctx, n_clusters):
    """more cells than waves in flight: every wave strides over several cells and adds its sums once"""
    rng = np.random.default_rng(31 + n_clusters)
    cells = mc.random_cells(rng, rng.integers(0, 6, size=3000).tolist(), 50)
    z1, total, changed = _iteration(ctx, cells, rng.integers(0, n_clusters, size=3000), 50, n_clusters, dn.level_tables(0.02))
    assert changed > 1000 and total < 0


def test_one_variant_shared_by_a_whole_cluster(ctx):
    """every atomic add of the counts goes to one pair"""
    rng = np.random.default_rng(12)
    cells = [[(0, int(r), int(a))] for r, a in zip(rng.integers(0, 4, size=3000), rng.integers(1, 4, size=3000))]
    _iteration(ctx, cells, np.ones(3000, dtype=np.uint32), 1, 2, dn.level_tables(0.02))
    _iteration(ctx, cells, np.arange(3000) % 2, 1, 2, dn.level_tables(0.02))


def test_a_pair_of_2_to_the_31_and_64_bit_products(ctx):
    tables = dn.level_tables(1e-4)
    cells = [[(0, 1 << 30, 1 << 29), (1, 3, 0), (2, 1 << 29, 5)], [(0, 1 << 30, (1 << 29) - 1), (1, 0, 2)], [(0, 0, 1 << 29), (2, 7, 1 << 30)],
             [(1, 1, 1)]]                                      # variant 0 holds 2^32 - 2^29 - 1 molecules, below the limit
    for z in ([0, 0, 1, 1], [1, 1, 1, 0], [0, 0, 0, 0]):
        z1, total, changed = _iteration(ctx, cells, z, 3, 2, tables)
        assert total < -(1 << 45)
    r, al = dn.cluster_counts(*dc.flatten(cells), [0, 0, 1, 1], 3, 2)
    assert r[0, 0] == 1 << 31 and al[0, 0] == (1 << 30) - 1


@pytest.mark.parametrize("n_clusters", (2, 31, 32))
def test_winners_in_chosen_lanes(ctx, n_clusters):
    """Variant 0 is hom-ref in every cluster, variant 1 + k hom-alt in cluster k alone (four base cells per cluster say so).  A
    probe (v0, 1, 0), (1 + w, 0, 3) is decided by its second entry, which the upper half of the wave scores: the winning sum sits in
    lane 32 + w until the halves are added.  A probe of the one entry (1 + w, 0, 3) is decided in lane w.  w = 0 and w = K - 1."""
    k = n_clusters
    base = [[(0, 4, 0)] + [(1 + j, 0 if j == c else 4, 4 if j == c else 0) for j in range(k)] for c in range(k) for _ in range(4)]
    z_base = [c for c in range(k) for _ in range(4)]
    probes, want = [], []
    for w in (0, k - 1):
        probes += [[(0, 1, 0), (1 + w, 0, 3)], [(1 + w, 0, 3)], sorted([(0, 1, 0), (1 + w, 0, 3), (1 + (w + 1) % k, 2, 0)])]
        want += [w, w, w]
    z = z_base + [(w + 1) % k for w in want]
    z1, total, changed = _iteration(ctx, base + probes, z, 1 + k, k, T)
    assert z1.tolist() == z_base + want and changed == len(probes)


def test_cells_alone_in_their_clusters_and_the_ties(ctx):
    alone = [[(0, 2, 0), (1, 0, 1)], [(0, 0, 1), (1, 0, 3)]]
    z1, total, changed = _iteration(ctx, alone, [0, 1], 2, 2, T)
    assert (z1.tolist(), total, changed) == ([0, 1], -138914, 0)
    z1, total, changed = _iteration(ctx, alone, [0, 1], 2, 3, T)                     # the empty cluster ties with the cell's own
    assert (z1.tolist(), total, changed) == ([0, 1], -138914, 0)
    z1, total, changed = _iteration(ctx, [alone[0], [], alone[1]], [0, 2, 1], 2, 3, T)   # a cell without entries
    assert (z1.tolist(), total, changed) == ([0, 0, 1], -138914, 1)
    # genotype ties (tables made for them): (2, 1) ties g 0 with g 1, (1, 2) g 1 with g 2
    ties = [-1, 0, -2, 0, -4, -4, 0, -2, 0, -1]
    cells = [[(0, 2, 1), (1, 1, 2), (2, 1, 1)], [(0, 1, 0), (1, 0, 1)], [(0, 2, 1), (1, 1, 2)]]
    for z in ([0, 1, 0], [0, 0, 1], [1, 1, 1]):
        _iteration(ctx, cells, z, 4, 2, ties)
    # three clusters hold the same cells and 29 hold none: rows of equal scores
    rng = np.random.default_rng(4)
    cells = mc.random_cells(rng, [5, 64, 3], 70)
    z1, total, changed = _iteration(ctx, cells + cells + cells, [0, 0, 0, 1, 1, 1, 31, 31, 31], 70, 32, T)
    # the two-cycle of the CPU tests
    cycle = [[(0, 1, 0), (1, 0, 2)], [(0, 1, 0), (1, 2, 2)], [(1, 0, 2)]]
    z1, total, changed = _iteration(ctx, cycle, [1, 0, 0], 2, 2, T)
    assert (z1.tolist(), total, changed) == ([0, 0, 1], -698414, 2)
    z1, total, changed = _iteration(ctx, cycle, [0, 0, 1], 2, 2, T)
    assert (z1.tolist(), total, changed) == ([1, 0, 0], -698414, 2)


# ---------------------------------------------------------------- the fit ----
def _same(got, want, what=""):
    assert got["restarts"].tolist() == want["restarts"].tolist(), what
    assert got["chosen"] == want["chosen"] and got["z"].tolist() == want["z"].tolist(), what
    assert got["recs"].tolist() == want["recs"].tolist(), what
    assert got["genotypes"].tolist() == want["genotypes"].tolist(), what


@pytest.fixture(scope="module")
def pool():
    rng = np.random.default_rng(100)
    genotypes = rng.integers(0, 3, size=(80, 3))
    cells = mc.haplotype_cells(rng, genotypes, rng.integers(0, 3, size=60).tolist(), 20)
    tables = dn.level_tables(0.02)
    entries, off = dc.flatten(cells)
    z0 = dn.start_assignments(60, 3, 5, 1)
    want = {m: dn.checker_cluster(entries, off, 80, 3, tables, z0, m) for m in (6, 8)}
    return dict(cells=cells, entries=entries, off=off, tables=tables, z0=z0, want=want)


def test_the_fit_uses_both_stop_conditions(ctx, pool):
    for max_iter in (6, 8):
        want = pool["want"][max_iter]
        assert set(want["restarts"]["converged"].tolist()) == {0, 1}, "the pool was chosen so that both ends occur"
        got = ctx.donor_cluster(pool["entries"], pool["off"], 80, 3, pool["tables"], pool["z0"], max_iter, with_scores=True)
        _same(got, want, max_iter)
        words = dn.entry_words(pool["entries"], pool["off"], want["z"], dn.pooled_genotypes(pool["entries"], 80, pool["tables"]), 3, pool["tables"])
        assert got["scores"].tolist() == dn.scores(dn.renumbered(pool["entries"]), pool["off"], words, 3, pool["tables"]).tolist()
    assert pool["want"][6]["restarts"]["converged"][pool["want"][6]["chosen"]] == 0
    assert pool["want"][8]["restarts"]["converged"][pool["want"][8]["chosen"]] == 1


def test_the_fit_twice_and_shuffled(ctx, pool):
    want = pool["want"][8]
    for _ in range(2):
        _same(ctx.donor_cluster(pool["entries"], pool["off"], 80, 3, pool["tables"], pool["z0"], 8), want)
    order = np.random.default_rng(2).permutation(60)
    entries, off = dc.flatten([pool["cells"][c] for c in order])
    got = ctx.donor_cluster(entries, off, 80, 3, pool["tables"], pool["z0"][:, order], 8)
    assert got["restarts"].tolist() == want["restarts"].tolist() and got["chosen"] == want["chosen"]
    assert got["z"].tolist() == want["z"][order].tolist() and got["recs"].tolist() == want["recs"][order].tolist()
    assert got["genotypes"].tolist() == want["genotypes"].tolist()


def test_a_small_fit_after_a_large_one_and_the_scores_call_behind_them(ctx, pool):
    rng = np.random.default_rng(6)
    genotypes = rng.integers(0, 3, size=(300, 32))
    cells = mc.haplotype_cells(rng, genotypes, rng.integers(0, 32, size=1500).tolist(), 12)
    entries, off = dc.flatten(cells)
    z0 = dn.start_assignments(1500, 32, 1, 3)
    _same(ctx.donor_cluster(entries, off, 300, 32, T, z0, 2), dn.checker_cluster(entries, off, 300, 32, T, z0, 2), "large")
    alone, off_a = dc.flatten([[(0, 2, 0), (1, 0, 1)], [(0, 0, 1), (1, 0, 3)]])
    got = ctx.donor_cluster(alone, off_a, 2, 3, T, [[0, 1]], 50)
    _same(got, dn.checker_cluster(alone, off_a, 2, 3, T, [[0, 1]], 50), "small")
    assert got["restarts"].tolist() == [(-138914, 1, 1)] and got["genotypes"].tolist() == [[0, 2], [2, 2], [3, 3]]
    # offsets that do not start at 0, one cluster, no cells
    _same(ctx.donor_cluster(pool["entries"], pool["off"][7:], 80, 1, T, np.zeros((2, 53), np.uint32), 4),
          dn.checker_cluster(pool["entries"], pool["off"][7:], 80, 1, T, np.zeros((2, 53), np.uint32), 4), "one cluster")
    got = ctx.donor_cluster(np.zeros(0, dn.ENTRY_DTYPE), np.zeros(1, np.uint64), 4, 2, T, np.zeros((3, 0), np.uint32), 5)
    assert got["restarts"].tolist() == [(0, 1, 1)] * 3 and got["chosen"] == 0 and got["genotypes"].tolist() == [[3] * 4] * 2
    # the unchanged bdg_donor_scores over the staging buffers the fits have used
    geno = dc.pack(dc.random_genotypes(rng, 80, 5))
    assert ctx.donor_scores(pool["entries"], pool["off"], geno, 5, T).tolist() == \
        dn.checker_records(pool["entries"], pool["off"], geno, 5, T).tolist()


# ---------------------------------------------------------------- argument errors ----
def _raw_fit(ctx, entries, off, n_variants, n_clusters, tables, z0, max_iter, null=()):
    """bdg_donor_cluster itself over poisoned outputs -> (return code, message, True if every output is still poisoned)"""
    entries, off = np.ascontiguousarray(entries, dtype=dn.ENTRY_DTYPE), np.ascontiguousarray(off, dtype=np.uint64)
    tables, z0 = np.ascontiguousarray(tables, dtype=np.int32), np.ascontiguousarray(z0, dtype=np.uint32)
    n = len(off) - 1
    outs = dict(z=_poisoned(4 * n), restarts=_poisoned(16 * len(z0)), chosen=_poisoned(4), recs=_poisoned(40 * n), scores=_poisoned(8 * n * 528),
                genotypes=_poisoned(n_variants * 32))
    ptr = lambda name, a: None if name in null else a.ctypes.data
    rc = ctx.lib.bdg_donor_cluster(ctx.h, ptr("entries", entries), ptr("off", off), n, n_variants, n_clusters, ptr("tables", tables),
                                   ptr("z0", z0), len(z0), max_iter, ptr("z", outs["z"]), ptr("restarts", outs["restarts"]),
                                   C.cast(ptr("chosen", outs["chosen"]), C.POINTER(C.c_uint32)), ptr("recs", outs["recs"]),
                                   ptr("scores", outs["scores"]), ptr("genotypes", outs["genotypes"]))
    return rc, ctx.lib.bdg_last_error(ctx.h).decode(), all((a == POISON).all() for a in outs.values())


def test_argument_errors_launch_nothing_and_write_nothing(ctx):
    entries, off = dc.flatten([[(0, 1, 0)], [(1, 0, 1)]])
    z0 = [[0, 1], [1, 0]]
    deep, off_d = dc.flatten([[(v % 2, 1 << 31, 1 << 31) for v in range(256)]])
    wide, off_w = dc.flatten([[(0, 1 << 31, 0)], [(0, 1 << 30, 1 << 30)]])
    ctx.profile(True)
    ctx.profile_reset()
    try:
        for args, null, message in (((entries, off, 2, 0, T, z0, 5), (), "the number of clusters must be 1 .. 32"),
                                    ((entries, off, 2, 33, T, z0, 5), (), "the number of clusters must be 1 .. 32"),
                                    ((entries, off, 2, 2, T, [[0, 2]], 5), (), "a start cluster is not below the number of clusters"),
                                    ((entries, off[::-1].copy(), 2, 2, T, z0, 5), (), "cell offsets must be non-decreasing"),
                                    ((entries, off, 1, 2, T, z0, 5), (), "an entry's variant is not below n_variants"),
                                    ((deep, off_d, 2, 2, T, [[0]], 5), (), "the counts of a cell sum to 2^40 or more"),
                                    ((wide, off_w, 1, 2, T, [[0, 1]], 5), (), "the counts of a variant sum to 2^32 or more"),
                                    ((entries, off, 2, 2, T, z0, 0), (), "at least one restart and one iteration"),
                                    ((entries, off, 2, 2, T, np.zeros((0, 2), np.uint32), 5), (), "at least one restart and one iteration")) + \
                tuple(((entries, off, 2, 2, T, z0, 5), (name,), "null pointer")
                      for name in ("entries", "off", "tables", "z0", "z", "restarts", "chosen", "recs", "genotypes")):
            rc, text, untouched = _raw_fit(ctx, *args, null=null)
            assert rc == _native.E_ARG and message in text and untouched, (message, null, rc, text)
            if not null and args[6] and len(args[5]):
                with pytest.raises(ValueError):                                 # the checker refuses the same
                    dn.cluster_restarts(*args)
        with pytest.raises(ValueError, match="z0 is restarts x cells"):
            ctx.donor_cluster(entries, off, 2, 2, T, [[0, 1, 0]], 5)
        with pytest.raises(_native.BadgerHipError, match="the number of clusters must be 1 .. 32"):
            ctx.donor_cluster(entries, off, 2, 33, T, z0, 5)
        d = [_native.DeviceArray.from_host(ctx, a) for a in (np.zeros(16, np.uint32), off, np.zeros(2, np.uint32), np.zeros(2, np.uint8),
                                                             _poisoned(64), _poisoned(64))]
        try:
            calls = (lambda e, k, out: ctx.donor_cluster_counts_dev(e, d[1], 2, d[2], 2, k, out),
                     lambda e, k, out: ctx.donor_cluster_assign_dev(e, d[1], 2, d[2], d[3], 2, k, T, d[4], d[2], out),
                     lambda e, k, out: ctx.donor_cluster_words_dev(e, d[1], 2, d[2], d[3], 2, k, T, out, d[5]))
            for call in calls:
                for k in (0, 33):
                    with pytest.raises(_native.BadgerHipError, match="the number of clusters must be 1 .. 32"):
                        call(d[0], k, d[4])
                with pytest.raises(_native.BadgerHipError, match="the entries must be aligned to 16 bytes"):
                    call(d[0].data_ptr() + 8, 2, d[4])
                with pytest.raises(_native.BadgerHipError, match="null pointer"):
                    call(d[0], 2, 0)
            ctx.synchronize()
            assert (d[4].to_host() == POISON).all() and (d[5].to_host() == POISON).all()
        finally:
            for a in d:
                a.free()
        times = ctx.profile_read()
        assert not [name for name, (launches, _) in times.items() if launches and (name.startswith("k_cluster") or name == "k_donor_scores")], times
        # one molecule below the variant's limit is taken, and it is the first launch
        wide["alt"][1] -= 1
        _same(ctx.donor_cluster(wide, off_w, 1, 2, T, [[0, 1]], 5), dn.checker_cluster(wide, off_w, 1, 2, T, [[0, 1]], 5))
        assert ctx.profile_read()["k_cluster_assign"][0] >= 1
    finally:
        ctx.profile(False)
