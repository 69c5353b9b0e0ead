"""The graph joins and the whitelist match on complete edit neighbourhoods (tests/edit_neighbourhoods.py): every single
edit at every place of a centre, every pair of them in the second shell, around centres whose runs sit on the seams of
the position arithmetic (places 0 and 15, the 4-base blocks of the probe tables, the groups of four deletions, runs across
them, rank 0 and rank 0xFFFFFFFF).  Everything is an integer and compared exactly: edge lists and best-hit answers with the
oracle, the k nearest with the restatement of tests/test_nearest_topk_gpu.py, and every (centre, member) pair with the
helper's own plain recurrence, which owes nothing to the oracle."""
import functools
import time

import numpy as np
import pytest

import edit_neighbourhoods as en
from badger_amd import _native, synth
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
GRAPH_ALGOS = {1: (0, 1, 2, 3, 4, 5, 6), 2: (0, 1, 3, 4, 5)}          # 2 and 6 serve threshold 1 only
ALL_A, ALL_T = "A" * 16, "T" * 16
# the centres that meet every list of the whitelist match; the others meet list A with the best-hit call
FULL = (ALL_T, "AAAACCCCGGGGTTTT", "ACGTTTTTTTTTACGT", en.CENTRES[0])
GRAPH_CASES = [(c, k) for c in en.CENTRES for k in range(len(en.slice_members(c)))]


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _ranks(xs):
    return np.array([en.rank(x) for x in xs], dtype=np.uint32)


# ---- graph ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _expected(c, k, thr):
    """ranks of slice k of c, the q-gram threshold and the oracle's edge list: once for all algorithms"""
    ranks = list(en.slices(c))[k]
    T = orc.qgram_threshold(thr)
    return ranks, T, orc.graph_edges(ranks, thr, T, threads=8)


def _pairs_of(c, members, thr, T):
    """{rank of x: dmin(c, x)} for the members x that the helper's recurrence and the q-gram count make an edge of c"""
    rc = en.rank(c)
    d = en.dmin_many(c, members).tolist()
    return {en.rank(x): dd for x, dd in zip(members, d) if dd <= thr and orc.qgram_S(rc, en.rank(x)) >= T}


def _edges_at(e, rc):
    """{other end: dist} of the rows of an edge list that touch rank rc; a pair listed twice fails here"""
    rows = e[(e["a"] == rc) | (e["b"] == rc)]
    other = np.where(rows["a"] == rc, rows["b"], rows["a"])
    got = dict(zip(other.tolist(), rows["dist"].tolist()))
    assert len(got) == len(rows)
    return got


@pytest.mark.parametrize("c,k", GRAPH_CASES, ids=["%s-%d" % ck for ck in GRAPH_CASES])
def test_graph_on_a_slice_of_the_closure(ctx, c, k):
    """the centre, its whole first shell and a stride slice of the second under every algorithm: the oracle's list row for
    row, and for every member x the pair (c, x) listed exactly when the plain recurrence says dmin <= thr (and the q-gram
    count reaches T), with that distance"""
    t0 = time.time()
    members = en.closure(c)[1] + en.slice_members(c)[k]
    rc = en.rank(c)
    ran = set()
    try:
        for thr in (1, 2):
            ranks, T, want = _expected(c, k, thr)
            pairs = _pairs_of(c, members, thr, T)
            assert _edges_at(want, rc) == pairs
            # both outcomes among the (c, x) pairs.  At thr 1 the first shell is in and the second out.  At thr 2 the second
            # shell of all-A / all-T lies at exactly two edits throughout (two letters of the run replaced, whatever the
            # script), so there only the q-gram count keeps a pair out; elsewhere the padding pushes members to dmin 3.
            assert 0 < len(pairs) < len(members), (thr, len(pairs))
            if thr == 1:
                assert len(pairs) == len(en.closure(c)[1])
            elif c in (ALL_A, ALL_T):
                assert (en.dmin_many(c, en.slice_members(c)[k]) == 2).all()
            else:
                assert (en.dmin_many(c, en.slice_members(c)[k]) > 2).any()
            for algo in GRAPH_ALGOS[thr]:
                ctx.graph_set_algo(algo)
                e = ctx.graph_edges(ranks, thr, T)
                assert len(e) == len(want) and (e == want).all(), (algo, thr, len(e), len(want))
                assert _edges_at(e, rc) == pairs, (algo, thr)
                ran.add((thr, algo))
            print("%s slice %d thr %d: %d rows, %d edges, %d of %d (c, x) pairs" % (c, k, thr, len(ranks), len(want), len(pairs), len(members)))
    finally:
        ctx.graph_set_algo(0)
    assert ran == {(thr, a) for thr, algos in GRAPH_ALGOS.items() for a in algos}
    print("%s slice %d: %.2f s" % (c, k, time.time() - t0))


def test_graph_cases_cover_every_slice():
    for c in en.CENTRES:
        assert [k for cc, k in GRAPH_CASES if cc == c] == list(range(len(list(en.slices(c)))))


def _isolated_pairs():
    """about 40 random bases, each with up to 256 partners, one per (script, places): both places of a two-substitution
    pair, and (deleted place, place the insertion goes in front of); the scripts go round the bases, so a base's partners
    are spread over all places and a 14-mer group holds few rows.  Plus all-T and all-A with their first shells."""
    rng = np.random.default_rng(404)
    bases = ["".join(en.LETTERS[int(x)] for x in rng.integers(0, 4, 16)) for _ in range(40)]
    todo = [("ss", i, j) for i in range(16) for j in range(i + 1, 16)] + [("di", i, j) for i in range(16) for j in range(16)]
    pairs, load, n = [], [0] * len(bases), 0
    for kind, i, j in todo:
        for _ in range(26):
            b = n % len(bases)
            n += 1
            s = bases[b]
            if kind == "ss":
                x = list(s)
                for p in (i, j):
                    x[p] = en.LETTERS[(en.LETTERS.index(s[p]) + int(rng.integers(1, 4))) % 4]
                x = "".join(x)
            else:
                t = s[:i] + s[i + 1:]
                first = int(rng.integers(0, 4))
                x = next(y for y in (t[:j] + en.LETTERS[(first + a) % 4] + t[j:] for a in range(4)) if y != s)
            pairs.append((s, x))
            load[b] += 1
    assert max(load) <= 256
    for s in (ALL_T, ALL_A):
        pairs += [(s, x) for x in en.n1(s)]
    return pairs


def test_graph_isolated_pairs(ctx):
    """pairs that stand almost alone: here a miss cannot hide behind a neighbouring row of the same group"""
    t0 = time.time()
    pairs = _isolated_pairs()
    ranks = np.unique(_ranks([x for p in pairs for x in p]))
    assert 9000 < len(ranks) < 11000
    d = en.dmin_pairs([a for a, _ in pairs], [b for _, b in pairs]).tolist()
    try:
        for thr, algos in ((1, (5, 6, 3)), (2, (5, 3))):
            T = orc.qgram_threshold(thr)
            want = orc.graph_edges(ranks, thr, T, threads=8)
            expect = {}
            for (a, b), dd in zip(pairs, d):
                ra, rb = en.rank(a), en.rank(b)
                key = (min(ra, rb), max(ra, rb))
                expect[key] = dd if dd <= thr and orc.qgram_S(ra, rb) >= T else None
            n_in = sum(v is not None for v in expect.values())
            assert 0 < n_in < len(expect)
            for algo in algos:
                ctx.graph_set_algo(algo)
                e = ctx.graph_edges(ranks, thr, T)
                assert len(e) == len(want) and (e == want).all(), (algo, thr, len(e), len(want))
                got = dict(zip(zip(e["a"].tolist(), e["b"].tolist()), e["dist"].tolist()))
                assert len(got) == len(e)
                assert all(got.get(key) == v for key, v in expect.items()), (algo, thr)
            print("isolated pairs thr %d: %d rows, %d edges, %d of %d built pairs are edges" % (thr, len(ranks), len(want), n_in, len(expect)))
    finally:
        ctx.graph_set_algo(0)
    print("isolated pairs: %.2f s" % (time.time() - t0))


def test_graph_shares_and_rounds_on_a_run_rich_slice(ctx):
    """a slice around ACGTTTTTTTTTACGT through bdg_graph_edges_part_dev: the deletion-variant joins in three rounds and
    without the second bucket level, as 1 and 3 shares (algorithm 5, thr 2) and as 2 shares (algorithm 6, thr 1): the shares
    are disjoint and their union is the oracle's list (equal length and equal rows once sorted leave room for neither a
    missing nor a doubled edge)"""
    from test_hip_parity import _GraphOnDevice, _parts_union_is
    c = "ACGTTTTTTTTTACGT"
    for algo, thr, parts, knobs in ((5, 2, (1, 3), (("d2_rounds", 3), ("dj_l2max", 0))), (6, 1, (2,), (("dj_l2max", 0), ("dj_l2max", -1)))):
        ranks, T, want = _expected(c, 1, thr)
        want = want[np.lexsort((want["b"], want["a"]))]
        assert len(want) > 1000
        dev = _GraphOnDevice(ctx, ranks, len(want) + 1024)
        ctx.graph_set_algo(algo)
        try:
            for knob, value in knobs:
                ctx.graph_set_knob(knob, value)
                for nparts in parts:
                    assert _parts_union_is(ctx, dev, nparts, thr, T, want, status=True), (algo, knob, value, nparts)
                ctx.graph_set_knob(knob, -1)
        finally:
            ctx.graph_set_knob("d2_rounds", -1)
            ctx.graph_set_knob("dj_l2max", -1)
            ctx.graph_set_algo(0)


# ---- nearest ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fillers():
    return synth.make_whitelist(4096, seed=4096)


def _shuffled(ranks, seed):
    """distinct ranks in an order that is not rank order: indices must refer to the caller's order"""
    ranks = np.unique(np.asarray(ranks, dtype=np.uint32))
    return ranks[np.random.default_rng(seed).permutation(len(ranks))]


@functools.lru_cache(maxsize=None)
def _queries(c):
    """c, both shells, and the first shells of the first 300 members of the second (up to six edits from c): distinct
    strings, in that order"""
    _, first, second = en.closure(c)
    return list(dict.fromkeys([c] + first + second + [y for x in second[:300] for y in en.n1(x)]))


def _list_a(c):
    return _shuffled(np.concatenate([_ranks([c] + en.closure(c)[1]), _fillers()]), 1)


def _list_c(c):
    return _shuffled(_ranks(en.closure(c)[2]), 3)


def _oracle_best_hit(q, wl):
    """the exhaustive scan's answers for max_ed 0, 1 and 2 from one scan at 2: the nearest entry and its ties do not depend on
    the bound, which only decides whether they are reported; every 8th query is scanned at 0 and at 1 as well to hold that"""
    i2, e2, t2 = orc.nearest16(q, wl, 2, threads=8)
    out = {2: (i2, e2, t2)}
    for max_ed in (0, 1):
        hit = e2 <= max_ed
        out[max_ed] = (np.where(hit, i2, NONE).astype(np.uint32), np.where(hit, e2, 255).astype(np.uint8), np.where(hit, t2, 0).astype(np.uint16))
        for a, b in zip(out[max_ed], orc.nearest16(q[::8], wl, max_ed, threads=8)):
            assert a.dtype == b.dtype and (a[::8] == b).all()
    return out


def _best_hit_equals_oracle(ctx, q, wl, algos=(1, 2, 3)):
    want = _oracle_best_hit(q, wl)
    try:
        for max_ed in (0, 1, 2):
            wi, we, wt = want[max_ed]
            for algo in algos:
                ctx.nearest16_set_algo(algo)
                gi, ge, gt = ctx.nearest16(q, wl, max_ed)
                for g, w, name in ((ge, we, "ed"), (gi, wi, "idx"), (gt, wt, "ties")):
                    assert (g == w).all(), (algo, max_ed, name, np.argwhere(g != w)[:4].ravel(), len(q), len(wl))
    finally:
        ctx.nearest16_set_algo(0)
    return want


@pytest.mark.parametrize("c", en.CENTRES)
def test_best_hit_list_a(ctx, c):
    """the list holds the centre and its first shell among 4,096 random entries; the queries are the whole closure and a
    third shell: index, distance and tie count of the oracle's exhaustive scan on every path"""
    t0 = time.time()
    qs = _queries(c)
    q, wl = _ranks(qs), _list_a(c)
    want = _best_hit_equals_oracle(ctx, q, wl)
    # against the plain recurrence: a member of the first shell is in the list, the centre one substitution from it
    n = 1 + len(en.closure(c)[1])
    assert (want[0][1][:n] == 0).all() and (want[2][1][:n] == 0).all() and (want[0][1][n:n + 300] == 255).all()
    assert {0, 1, 2} <= set(want[2][1].tolist()) and {0, 1, 255} <= set(want[1][1].tolist())
    print("%s list A: %d queries, %d entries, %.2f s" % (c, len(q), len(wl), time.time() - t0))


@pytest.mark.parametrize("c", FULL)
def test_best_hit_list_b(ctx, c):
    """the centre alone among the random entries: wherever the plain recurrence puts it within max_ed and no random entry
    is as near, the answer is the centre at that distance; where nothing lies within max_ed it is 'none'"""
    qs = _queries(c)
    q = _ranks(qs)
    wl = _shuffled(np.concatenate([_ranks([c]), _fillers()]), 2)
    at = int(np.nonzero(wl == en.rank(c))[0][0])
    others = np.delete(wl, at)
    lev_c = en.lev_many(c, qs)
    nearest_other = orc.nearest16(q, others, 2, threads=8)[1]
    try:
        for max_ed in (0, 1, 2):
            fe = np.where(nearest_other <= max_ed, nearest_other, 255)
            centre = (lev_c <= max_ed) & (lev_c < fe)
            nothing = (lev_c > max_ed) & (fe == 255)
            assert centre.any() and nothing.any() and (centre | nothing).sum() > 0.99 * len(q)
            for algo in (1, 2, 3):
                ctx.nearest16_set_algo(algo)
                gi, ge, gt = ctx.nearest16(q, wl, max_ed)
                assert (ge[centre] == lev_c[centre]).all() and (gi[centre] == at).all() and (gt[centre] == 1).all(), (algo, max_ed)
                assert (ge[nothing] == 255).all() and (gi[nothing] == NONE).all() and (gt[nothing] == 0).all(), (algo, max_ed)
    finally:
        ctx.nearest16_set_algo(0)


@pytest.mark.parametrize("c", FULL)
def test_best_hit_list_c_dense(ctx, c):
    """the second shell itself is the list, the centre and the first shell ask: thousands of entries at one distance, so
    a lane of the probe path holds more than four hits and hands the query to the cooperative kernel.  Around all-T the
    best-hit call cannot get there: a query of the first shell has an entry one substitution away and never asks the
    deletion variants, and the centre's own variant is fifteen T, whose re-insertions hold one other letter and are
    not in the list; there the hand-over is taken by the top-k call (test_topk_list_c_dense), which asks them always."""
    qs = [c] + en.closure(c)[1]
    q, wl = _ranks(qs), _list_c(c)
    want = _best_hit_equals_oracle(ctx, q, wl)
    lev_c = en.lev_many(c, en.closure(c)[2])
    assert want[2][1][0] == 2 and want[2][2][0] == (lev_c == 2).sum() >= 1000          # the centre's ties, by the recurrence
    assert want[1][1][0] == 255 and (want[1][1][1:] == 1).any()
    try:
        ctx.nearest16_set_algo(2)
        ctx.nearest16(q, wl, 2)
        handed_over = ctx.nearest16_overflow_count()
        assert handed_over > 0 or c == ALL_T
    finally:
        ctx.nearest16_set_algo(0)
    print("%s list C: %d queries, %d entries, most ties %d, %d queries handed over" % (c, len(q), len(wl), int(want[2][2].max()), handed_over))


def _topk_equals_restatement(ctx, q, wl):
    from test_nearest_topk_gpu import Restated
    want = Restated(q, wl)
    handed_over = 0
    try:
        for max_ed in (1, 2, 3):
            for algo in (0, 2, 3):
                if algo == 2 and max_ed > 2:
                    continue
                ctx.nearest16_set_algo(algo)
                bi, be, _ = ctx.nearest16(q, wl, max_ed)
                for k in (1, 8):
                    wi, we, wn = want.answer(max_ed, k)
                    gi, ge, gn = ctx.nearest16_topk(q, wl, max_ed, k)
                    for g, w, name in ((gi, wi, "idx"), (ge, we, "ed"), (gn, wn, "n_within")):
                        assert g.shape == w.shape and (g == w).all(), (algo, max_ed, k, name, np.argwhere(g != w)[:4].ravel())
                    assert (gi[:, 0] == bi).all() and (ge[:, 0] == be).all(), (algo, max_ed, k)
                    if algo == 2 and max_ed == 2:
                        handed_over = max(handed_over, ctx.nearest16_overflow_count())
    finally:
        ctx.nearest16_set_algo(0)
    return want, handed_over


@pytest.mark.parametrize("c", FULL)
def test_topk_list_a(ctx, c):
    """the k nearest on list A.  The restatement holds a whole distance matrix, so the queries are the centre, the whole
    first shell (every edit at every place), and every n-th member of the second and third, about 1,000 in all."""
    t0 = time.time()
    _, first, second = en.closure(c)
    qs = _queries(c)
    rest = qs[1 + len(first):]
    q = _ranks([c] + first + rest[::-(-len(rest) // 900)])
    want, _ = _topk_equals_restatement(ctx, q, _list_a(c))
    assert {0, 1, 2} <= set(want.answer(3, 1)[1][:, 0].tolist()) and {0, 1, 255} <= set(want.answer(1, 1)[1][:, 0].tolist())
    print("%s top-k list A: %d queries, %.2f s" % (c, len(q), time.time() - t0))


@pytest.mark.parametrize("c", FULL)
def test_topk_list_c_dense(ctx, c):
    qs = [c] + en.closure(c)[1]
    want, handed_over = _topk_equals_restatement(ctx, _ranks(qs), _list_c(c))
    assert want.answer(2, 8)[2].max() >= 1000                       # n_within: far more candidates than slots
    assert handed_over > 0                                          # the probe path's call at max_ed 2 went on to the cooperative kernel
    print("%s top-k list C: %d queries handed over" % (c, handed_over))
