"""What bdg_donor_scores and bdg_donor_cluster share on the host (csrc/donors_kernels.hip: the entry check and the staged call),
through Context.donor_scores and Context.donor_cluster: offsets that do not start at 0, behind entries that must not be looked
at; one context whose staging buffers serve both calls in turn, growing and shrinking; and the three refusals the two calls have
in common, over poisoned outputs, with nothing launched."""
import ctypes as C

import numpy as np
import pytest

import demux_cases as mc
import donor_cases as dc
from badger_amd import _native
from badger_amd import donors as dn

pytestmark = pytest.mark.gpu

LEAD, SIZES, VARIANTS, POISON = 37, [0, 1, 63, 64, 65, 129], 200, 0xAB
T = dc.TABLES_001


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _same_fit(got, want, what):
    for name in ("restarts", "z", "recs", "genotypes"):
        assert got[name].tolist() == want[name].tolist(), (what, name)
    assert got["chosen"] == want["chosen"], what


def _behind_unused(entries, off):
    """the same cells behind LEAD entries of a variant that no call may look at"""
    lead = np.zeros(LEAD, dtype=dn.ENTRY_DTYPE)
    lead["variant"], lead["ref"], lead["alt"] = 0xFFFFFFFF, 1 << 31, 1 << 31
    return np.concatenate([lead, entries]), off + np.uint64(LEAD)


@pytest.mark.parametrize("n", (1, 3, 32))
def test_offsets_that_do_not_start_at_zero(ctx, n):
    rng = np.random.default_rng(370 + n)
    entries, off = dc.flatten(mc.random_cells(rng, SIZES, VARIANTS))
    moved, off_m = _behind_unused(entries, off)
    assert off_m[0] == LEAD and len(moved) == len(entries) + LEAD
    geno = dc.pack(dc.random_genotypes(rng, VARIANTS, n))
    want = dn.checker_records(entries, off, geno, n, T)
    recs, scores = ctx.donor_scores(entries, off, geno, n, T, with_scores=True)
    recs_m, scores_m = ctx.donor_scores(moved, off_m, geno, n, T, with_scores=True)
    assert recs_m.tolist() == recs.tolist() == want.tolist()
    assert scores_m.tolist() == scores.tolist() == dn.scores(entries, off, geno, n, T).tolist()
    z0 = dn.start_assignments(len(SIZES), n, 2, 9)
    want = dn.checker_cluster(entries, off, VARIANTS, n, T, z0, 3)
    _same_fit(dn.checker_cluster(moved, off_m, VARIANTS, n, T, z0, 3), want, "the checker itself")
    fit, fit_m = (ctx.donor_cluster(e, o, VARIANTS, n, T, z0, 3, with_scores=True) for e, o in ((entries, off), (moved, off_m)))
    _same_fit(fit, want, "from 0")
    _same_fit(fit_m, want, "from %d" % LEAD)
    assert fit_m["scores"].tolist() == fit["scores"].tolist()


def test_one_context_serves_both_calls_growing_and_shrinking(ctx):
    rng = np.random.default_rng(41)
    entries, off = dc.flatten(mc.random_cells(rng, rng.integers(0, 6, size=3000).tolist(), 50))
    few, off_f = dc.flatten(mc.random_cells(rng, [2, 0, 5], 50))
    two, off_t = dc.flatten([[(0, 2, 0), (1, 0, 1)], [(0, 0, 1), (1, 0, 3)]])
    geno = dc.pack(dc.random_genotypes(rng, 50, 3))
    z0 = dn.start_assignments(3000, 3, 2, 1)
    _same_fit(ctx.donor_cluster(entries, off, 50, 3, T, z0, 3), dn.checker_cluster(entries, off, 50, 3, T, z0, 3), "3,000 cells")
    assert ctx.donor_scores(few, off_f, geno, 3, T).tolist() == dn.checker_records(few, off_f, geno, 3, T).tolist()
    _same_fit(ctx.donor_cluster(two, off_t, 2, 3, T, [[0, 1], [1, 1]], 3), dn.checker_cluster(two, off_t, 2, 3, T, [[0, 1], [1, 1]], 3), "2 cells")
    recs, scores = ctx.donor_scores(entries, off, geno, 3, T, with_scores=True)
    assert recs.tolist() == dn.checker_records(entries, off, geno, 3, T).tolist()
    assert scores.tolist() == dn.scores(entries, off, geno, 3, T).tolist()


def _raw(ctx, which, entries, off, n_variants):
    """bdg_donor_scores or bdg_donor_cluster itself (2 donors or clusters, valid but for the entries and offsets) over poisoned
    outputs -> (return code, message, True if every output is still poisoned)"""
    entries, off = np.ascontiguousarray(entries, dtype=dn.ENTRY_DTYPE), np.ascontiguousarray(off, dtype=np.uint64)
    n, tables = len(off) - 1, np.array(T, dtype=np.int32)
    outs = {name: np.full(b + 16, POISON, np.uint8)
            for name, b in dict(recs=40 * n, scores=8 * n * 3, z=4 * n, restarts=16, chosen=4, genotypes=2 * n_variants).items()}
    p = {name: a.ctypes.data for name, a in outs.items()}
    if which == "scores":
        geno = np.zeros(max(n_variants, 1), dtype=np.uint64)
        rc = ctx.lib.bdg_donor_scores(ctx.h, entries.ctypes.data, off.ctypes.data, n, geno.ctypes.data, n_variants, 2, tables.ctypes.data,
                                      p["recs"], p["scores"])
    else:
        z0 = np.zeros(n, dtype=np.uint32)
        rc = ctx.lib.bdg_donor_cluster(ctx.h, entries.ctypes.data, off.ctypes.data, n, n_variants, 2, tables.ctypes.data, z0.ctypes.data, 1, 5,
                                       p["z"], p["restarts"], C.cast(p["chosen"], C.POINTER(C.c_uint32)), p["recs"], p["scores"], p["genotypes"])
    return rc, ctx.lib.bdg_last_error(ctx.h).decode(), all((a == POISON).all() for a in outs.values())


def test_the_shared_refusals_say_the_same_and_touch_nothing(ctx):
    try:
        entries, off = dc.flatten([[(0, 1, 0)], [(1, 0, 1)], [(1, 2, 2)]])
        disorder = off.copy()
        disorder[1], disorder[2] = off[2], off[1]
        half = 1 << 31
        deep, off_d = dc.flatten([[(0, 1, 1)], [(v % 2, half, half) for v in range(256)]])
        ctx.profile(True)
        ctx.profile_reset()
        for what, (e, o, v) in {"cell offsets must be non-decreasing": (entries, disorder, 2),
                                "an entry's variant is not below n_variants": (entries, off, 1),
                                "the counts of a cell sum to 2^40 or more": (deep, off_d, 2)}.items():
            for which in ("scores", "cluster"):
                rc, text, untouched = _raw(ctx, which, e, o, v)
                assert rc == _native.E_ARG and text.split(": ", 1) == ["donors", what] and untouched, (which, what, rc, text)
        ctx.synchronize()
        assert not [name for name, (launches, _) in ctx.profile_read().items() if launches], "a refusal launched something"
        # one molecule less and both calls take the cell, unused entries of any variant in front
        deep["alt"][-1] -= 1
        moved, off_m = _behind_unused(deep, off_d)
        geno = dc.pack([[0, 1], [2, 0]])
        assert ctx.donor_scores(moved, off_m, geno, 2, T).tolist() == dn.checker_records(deep, off_d, geno, 2, T).tolist()
        rc, text, untouched = _raw(ctx, "cluster", moved, off_m, 2)
        assert rc == _native.E_ARG and "the counts of a variant sum to 2^32 or more" in text and untouched      # (the cluster call's own bound)
        assert ctx.profile_read()["k_donor_scores"][0] == 1
    finally:
        ctx.profile(False)
