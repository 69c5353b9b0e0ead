"""k_donor_scores (csrc/donors_kernels.hip) against the rule of badger_amd/donors.py: the records and the full score matrix equal
the checker's exactly, through bdg_donor_scores and through bdg_donor_scores_dev.  1, 2, 11 (66 hypotheses: one in the second
round), 12 and 32 donors (528: nine rounds, the last partial); cells of 0, 1, 63, 64, 65, 128 and 129 entries, the chunk borders;
5,000 cells of 0 .. 3 entries, so that every wave strides over several cells; counts near 2^31 at e = 1e-4 and a cell one below the
2^40 bound; winners in lane 0, lane 63 and the last round; the tie rules; every argument error, with nothing launched."""
import numpy as np
import pytest

import donor_cases as dc
from badger_amd import _native
from badger_amd import donors as dn

pytestmark = pytest.mark.gpu

DONORS = (1, 2, 11, 12, 32)
BORDERS = [0, 1, 63, 64, 65, 128, 129]
POISON = 0xAB


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _dev(ctx, entries, off, geno, n_donors, tables, with_scores=True):
    """bdg_donor_scores_dev over device arrays, the outputs poisoned first and one row longer than they need be"""
    n, h = len(off) - 1, n_donors + n_donors * (n_donors - 1) // 2
    arrays = (entries.view(np.uint32) if len(entries) else np.zeros(4, np.uint32), off, geno if len(geno) else np.zeros(1, np.uint64),
              np.full((n + 1) * _native.DONOR_DTYPE.itemsize, POISON, np.uint8), np.full((n + 1) * h * 8, POISON, np.uint8))
    d = [_native.DeviceArray.from_host(ctx, np.ascontiguousarray(a)) for a in arrays]
    try:
        ctx.donor_scores_dev(d[0], d[1], n, d[2], len(geno), n_donors, tables, d[3], d[4] if with_scores else None)
        ctx.synchronize()
        recs, scores = d[3].to_host(), d[4].to_host()
        assert (recs[n * _native.DONOR_DTYPE.itemsize:] == POISON).all(), "a record behind the last cell"
        assert (scores[n * h * 8 if with_scores else 0:] == POISON).all(), "a score behind the last cell"
        return recs[:n * _native.DONOR_DTYPE.itemsize].view(_native.DONOR_DTYPE), scores[:n * h * 8].view(np.int64).reshape(n, h)
    finally:
        for a in d:
            a.free()


def _check(ctx, cells, genotypes, n_donors, tables, what=""):
    """both entry points against the checker -> the checker's records"""
    entries, off = dc.flatten(cells)
    geno = dc.pack(genotypes)
    want_scores = dn.scores(entries, off, geno, n_donors, tables)
    want = dn.records(want_scores, n_donors)
    recs, scores = ctx.donor_scores(entries, off, geno, n_donors, tables, with_scores=True)
    assert scores.tolist() == want_scores.tolist(), what
    assert recs.tolist() == want.tolist(), what
    assert ctx.donor_scores(entries, off, geno, n_donors, tables).tolist() == want.tolist(), what        # without the matrix
    recs, scores = _dev(ctx, entries, off, geno, n_donors, tables)
    assert scores.tolist() == want_scores.tolist() and recs.tolist() == want.tolist(), what
    assert _dev(ctx, entries, off, geno, n_donors, tables, with_scores=False)[0].tolist() == want.tolist(), what
    return want


def test_dtypes_are_the_checkers():
    assert _native.DONOR_ENTRY_DTYPE == dn.ENTRY_DTYPE and _native.DONOR_DTYPE == dn.REC_DTYPE
    assert _native.DONOR_DTYPE.itemsize == 40 and _native.DONOR_ENTRY_DTYPE.itemsize == 16 and _native.DONOR_NONE == dn.NONE


def test_the_cell_written_out_by_hand(ctx):
    entries, off = dc.flatten(dc.HAND["cells"])
    recs, scores = ctx.donor_scores(entries, off, dc.pack(dc.HAND["genotypes"]), 2, dc.TABLES_001, with_scores=True)
    assert scores.tolist() == dc.HAND["scores"] and recs.tolist() == [dc.HAND["record"]]


@pytest.mark.parametrize("n_donors", DONORS)
def test_chunk_borders(ctx, n_donors):
    rng = np.random.default_rng(600 + n_donors)
    genotypes = dc.random_genotypes(rng, 200, n_donors)
    sizes = BORDERS + BORDERS[::-1]
    _check(ctx, dc.random_cells(rng, sizes, 200), genotypes, n_donors, dn.level_tables(0.01))
    _check(ctx, dc.random_cells(rng, [129], 200, high=1000), genotypes, n_donors, dn.level_tables(0.2), "one cell")


@pytest.mark.parametrize("n_donors", (3, 32))
def test_many_small_cells(ctx, n_donors):
    """more cells than waves in flight at one round; at nine rounds, 5,000 cells are still several per wave"""
    rng = np.random.default_rng(77 + n_donors)
    genotypes = dc.random_genotypes(rng, 50, n_donors)
    want = _check(ctx, dc.random_cells(rng, rng.integers(0, 4, size=5000).tolist(), 50), genotypes, n_donors, dn.level_tables(0.01))
    assert len(want) == 5000


@pytest.mark.parametrize("n_donors", (2, 32))
def test_sums_are_64_bit(ctx, n_donors):
    rng = np.random.default_rng(8 + n_donors)
    genotypes = dc.random_genotypes(rng, 256, n_donors)
    near = lambda: int(rng.integers((1 << 31) - 5, 1 << 31))
    cells = [[(v, near(), near()) for v in range(m)] for m in (1, 65, 129)]
    # and one molecule short of the bound: 255 entries of 2^31 + 2^31 and one of 2^31 + 2^31 - 1
    cells.append([(v, 1 << 31, (1 << 31) - (v == 200)) for v in range(256)])
    want = _check(ctx, cells, genotypes, n_donors, dn.level_tables(1e-4))
    assert int(want["best_score"].min()) < -(1 << 55)


def test_winners_in_chosen_lanes(ctx):
    """32 donors: the best singlet in lane 0 and in lane 31, the second beside it; the best pair at h = 63 (lane 63 of round 0),
    h = 64 (lane 0 of round 1), h = 512 (lane 0 of the last round) and h = 527 (the last hypothesis, lane 15 of the last round)"""
    rng = np.random.default_rng(5)
    genotypes = dc.random_genotypes(rng, 129, 32)
    hyp = dn.hypotheses(32)
    placed = [(0,), (31,), hyp[63], hyp[64], hyp[512], hyp[527], hyp[32]]
    assert hyp[527] == (30, 31) and hyp[32] == (0, 1) and hyp[63][0] == 1
    want = _check(ctx, [dc.cell_of_levels(genotypes, who) for who in placed], genotypes, 32, dn.level_tables(0.01))
    assert want["donor1"][:2].tolist() == [0, 31]
    assert want["pair"][2:].tolist() == [a | b << 16 for a, b in placed[2:]]
    # the second singlet in lane 31 and lane 0: a donor one variant away from the best
    genotypes[:, 31] = genotypes[:, 0]
    genotypes[0, 31] = (genotypes[0, 0] + 1) % 3
    want = _check(ctx, [dc.cell_of_levels(genotypes, (0,)), dc.cell_of_levels(genotypes, (31,))], genotypes, 32, dn.level_tables(0.01))
    assert want["donor1"].tolist() == [0, 31] and want["donor2"].tolist() == [31, 0]
    # 11 donors: the one hypothesis of the second round wins
    genotypes = dc.random_genotypes(rng, 129, 11)
    want = _check(ctx, [dc.cell_of_levels(genotypes, (9, 10)), dc.cell_of_levels(genotypes, (8, 10))], genotypes, 11, dn.level_tables(0.01))
    assert want["pair"].tolist() == [9 | 10 << 16, 8 | 10 << 16]


@pytest.mark.parametrize("n_donors", (5, 32))
def test_tie_rules(ctx, n_donors):
    rng = np.random.default_rng(21)
    genotypes = dc.random_genotypes(rng, 70, n_donors)
    last = n_donors - 1
    genotypes[:, 3] = genotypes[:, 1]
    genotypes[:, last] = genotypes[:, 0]
    cells = [dc.cell_of_levels(genotypes, (1,)), [], dc.cell_of_levels(genotypes, (2, last)), dc.cell_of_levels(genotypes, (last,)),
             dc.cell_of_levels(genotypes, (3, last))]
    want = _check(ctx, cells, genotypes, n_donors, dn.level_tables(0.01))
    assert (want["donor1"][0], want["donor2"][0], want["pair"][0]) == (1, 3, 1 | 3 << 16) and want["best_score"][0] == want["second_score"][0]
    assert want[1].tolist() == (0, 0, 0, 0, 1, 0 | 1 << 16, 0)
    assert want["pair"][2] == 0 | 2 << 16 and (want["donor1"][3], want["donor2"][3]) == (0, last) and want["pair"][4] == 0 | 1 << 16
    # every donor the same: every singlet ties, every pair ties
    same = np.repeat(genotypes[:, :1], n_donors, axis=1)
    want = _check(ctx, [dc.cell_of_levels(same, (0,))], same, n_donors, dn.level_tables(0.01))
    assert want[["donor1", "donor2", "pair"]].tolist() == [(0, 1, 0 | 1 << 16)]


def test_no_cells_and_offsets_that_do_not_start_at_zero(ctx):
    geno = dc.pack([[0, 1], [2, 0]])
    assert len(ctx.donor_scores(np.zeros(0, dn.ENTRY_DTYPE), np.zeros(1, np.uint64), geno, 2, dc.TABLES_001)) == 0
    entries, off = dc.flatten([[(1, 7, 7)], [(0, 1, 0), (1, 0, 2)], [(0, 3, 3)]])
    want = dn.records(dn.scores(entries, off[1:], geno, 2, dc.TABLES_001), 2)
    assert len(want) == 2 and ctx.donor_scores(entries, off[1:], geno, 2, dc.TABLES_001).tolist() == want.tolist()


def test_argument_errors_launch_nothing(ctx):
    genotypes = [[0, 1], [2, 0]]
    entries, off = dc.flatten([[(0, 1, 0)], [(1, 0, 1)]])
    geno, t = dc.pack(genotypes), dc.TABLES_001
    at_bound, off_b = dc.flatten([[(v % 2, 1 << 31, 1 << 31) for v in range(256)]])
    ctx.profile(True)
    ctx.profile_reset()
    try:
        for args, message in (((entries, off, geno, 0, t), "the number of donors must be 1 .. 32"),
                              ((entries, off, geno, 33, t), "the number of donors must be 1 .. 32"),
                              ((entries, off[::-1].copy(), geno, 2, t), "cell offsets must be non-decreasing"),
                              ((entries, off, geno[:1], 2, t), "an entry's variant is not below n_variants"),
                              ((entries, off, dc.pack([[0, 3], [2, 0]]), 2, t), "a genotype field holds 3"),
                              ((at_bound, off_b, geno, 2, t), "the counts of a cell sum to 2\\^40 or more")):
            with pytest.raises(_native.BadgerHipError, match=message) as e:
                ctx.donor_scores(*args)
            assert e.value.code == _native.E_ARG
            with pytest.raises(ValueError):                                     # the checker refuses the same
                dn.scores(*args)
        with pytest.raises(ValueError, match="ten table values"):
            ctx.donor_scores(entries, off, geno, 2, t[:9])
        with pytest.raises(ValueError, match="the entries reach to its highest"):
            ctx.donor_scores(entries[:1], off, geno, 2, t)
        d = [_native.DeviceArray.from_host(ctx, a) for a in (np.zeros(16, np.uint32), off, geno, np.zeros(80, np.uint8))]
        try:
            for n_donors in (0, 33):
                with pytest.raises(_native.BadgerHipError, match="the number of donors must be 1 .. 32"):
                    ctx.donor_scores_dev(d[0], d[1], 2, d[2], 2, n_donors, t, d[3])
            with pytest.raises(_native.BadgerHipError, match="the entries must be aligned to 16 bytes"):
                ctx.donor_scores_dev(d[0].data_ptr() + 8, d[1], 2, d[2], 2, 2, t, d[3])
            with pytest.raises(_native.BadgerHipError, match="null pointer"):
                ctx.donor_scores_dev(d[0], d[1], 2, d[2], 2, 2, t, 0)
            ctx.donor_scores_dev(d[0], d[1], 0, d[2], 2, 2, t, 0)                     # no cells: valid, nothing to write
        finally:
            for a in d:
                a.free()
        ctx.synchronize()
        assert ctx.profile_read().get("k_donor_scores", (0, 0.0))[0] == 0
        # a field of a donor that is not there is not looked at, and the call below is the first launch
        assert ctx.donor_scores(entries, off, dc.pack([[0, 3], [2, 0]]), 1, t).tolist() == \
            dn.records(dn.scores(entries, off, dc.pack([[0, 3], [2, 0]]), 1, t), 1).tolist()
        assert ctx.profile_read()["k_donor_scores"][0] == 1
    finally:
        ctx.profile(False)
