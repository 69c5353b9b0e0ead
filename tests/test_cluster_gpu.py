"""The stage-2 clustering kernels (csrc/distinct_kernels.hip) called directly.  bdg_cluster_dev on the packed union of
tests/cluster_cases.py - every graph of at most five vertices with every centre set and a sample of larger ones, in one launch,
plain, with every edge doubled and with self-loops - against the reference walk; on the scale and boundary shapes; with its
workspace reused.  bdg_touched_count_dev, bdg_assign_reads_dev and bdg_keep_observed against plain numpy around the block size,
with the indices and ranks at both ends of 32 bits.  Stage2.cluster's device path with centres that were never observed.
Integers only: every comparison is exact.  Edge indices at or above nu are never passed to bdg_cluster_dev (its callers cannot
produce them and k_cluster_offer does not check them)."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

import cluster_cases as cc
from badger_amd import _native
from badger_amd.common import unrank
from badger_amd.stage2 import EdgeRows, Stage2

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
OK16 = _native.FLAG_RANK_OK | _native.FLAG_BC16


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _up(ctx, arr):
    return _native.DeviceArray.from_host(ctx, arr)


def _cluster(ctx, nu, ea, eb, owner_in):
    """bdg_cluster_dev over host arrays -> owner int32 [nu]; no edges: null edge pointers"""
    m = len(ea)
    held = [_up(ctx, owner_in)] + ([_up(ctx, ea), _up(ctx, eb)] if m else [])
    try:
        ctx.cluster_dev(held[1] if m else 0, held[2] if m else 0, m, nu, held[0])
        return held[0].to_host()[:nu]
    finally:
        for d in held:
            d.free()


# ---- 1. the packed union ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", cc.VARIANTS)
def test_every_small_graph_in_one_launch(ctx, variant):
    pk = cc.packed(variant)
    got = _cluster(ctx, pk.nu, pk.ea, pk.eb, pk.owner_in)
    assert got.dtype == np.int32 and len(got) == pk.nu
    assert (got == pk.owner_want).all(), cc.describe_first_difference(pk, got)


# ---- 2. scale and boundary shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s.name for s in cc.shapes()])
def test_shape(ctx, name):
    s = next(s for s in cc.shapes() if s.name == name)
    got = _cluster(ctx, s.nu, s.ea, s.eb, s.owner_in)
    bad = np.flatnonzero(got != s.owner_want)
    assert not len(bad), (name, len(bad), [(int(v), int(got[v]), int(s.owner_want[v])) for v in bad[:8]])
    for v, o in s.pins:
        assert got[v] == o, (name, v, o, int(got[v]))


def test_nothing_to_do(ctx):
    # no barcode at all: nothing is launched, nothing is read, null pointers are fine
    ctx.cluster_dev(0, 0, 0, 0, 0)
    # barcodes and no edge, null edge pointers: the centres stay, nobody joins them
    owner_in = np.array([-2, 1, -2, 3, -2], dtype=np.int32)
    assert (_cluster(ctx, 5, np.zeros(0, np.uint32), np.zeros(0, np.uint32), owner_in) == owner_in).all()
    # edges without their arrays are refused, and the context goes on working
    d = _up(ctx, owner_in)
    with pytest.raises(_native.BadgerHipError):
        ctx.cluster_dev(0, 0, 3, 5, d)
    assert (d.to_host() == owner_in).all()
    d.free()
    assert _cluster(ctx, 2, np.array([1], np.uint32), np.array([0], np.uint32), np.array([0, -2], np.int32)).tolist() == [0, 0]


# ---- 3. the workspace, shared with the other stage-2 calls ------------------------------------------------------------------
def test_workspace_reuse(ctx):
    pk = cc.packed("plain")
    tri_ea, tri_eb, tri_in = np.array([1, 2], np.uint32), np.array([0, 1], np.uint32), np.array([-2, -2, 2], np.int32)
    first = _cluster(ctx, pk.nu, pk.ea, pk.eb, pk.owner_in)
    assert (first == pk.owner_want).all(), cc.describe_first_difference(pk, first)
    # (the other scratch buffer: the flags of bdg_touched_count_dev)
    d_a, d_b, d_c = _up(ctx, pk.ea), _up(ctx, pk.eb), _up(ctx, np.flatnonzero(pk.owner_in >= 0).astype(np.uint32))
    touched = ctx.touched_count_dev(d_a, d_b, len(pk.ea), pk.nu, d_c, d_c.shape[0])
    want_touched = len(np.unique(np.concatenate([pk.ea, pk.eb, d_c.to_host()])))
    assert touched == want_touched
    small = _cluster(ctx, 3, tri_ea, tri_eb, tri_in)
    assert small.tolist() == [2, 2, 2]                                # 2 is the centre, 1 beside it, 0 beside 1
    assert ctx.touched_count_dev(d_a, d_b, len(pk.ea), pk.nu, d_c, d_c.shape[0]) == want_touched
    third = _cluster(ctx, pk.nu, pk.ea, pk.eb, pk.owner_in)
    assert (third == pk.owner_want).all(), cc.describe_first_difference(pk, third)
    assert first.tobytes() == third.tobytes()
    for d in (d_a, d_b, d_c):
        d.free()


# ---- 4. bdg_touched_count_dev -----------------------------------------------------------------------------------------------
def _touched(ctx, ea, eb, nu, extra):
    held = [_up(ctx, np.asarray(a, dtype=np.uint32)) for a in (ea, eb, extra)]
    try:
        return ctx.touched_count_dev(held[0], held[1], len(ea), nu, held[2], len(extra))
    finally:
        for d in held:
            d.free()


@pytest.mark.parametrize("nu", (1, 63, 64, 65, 255, 256, 257, 4096 * 256 + 300))
def test_touched_count(ctx, nu):
    """against the size of the set of indices below nu; indices equal to nu and to 2^32 - 1 are in all three arrays and count
    for nothing; above 4096 x 256 barcodes k_count_flags goes round its loop twice, and the flags it meets there are set"""
    rng = np.random.default_rng(nu)
    none = np.zeros(0, np.uint32)

    def indices(n, top):
        a = rng.integers(0, min(nu, top), n).astype(np.uint32)
        if n >= 4:
            a[rng.choice(n, 2, replace=False)] = [nu, NONE]           # no barcodes: the kernel must pass them over
        return a

    def want(*arrays):
        u = np.unique(np.concatenate(arrays).astype(np.uint32))
        return int((u < nu).sum())

    big, few = 5000 if nu > 4096 else 300, 40
    for m, n_extra in ((big, few), (few, big), (0, few), (few, 0), (0, 0), (256, 256), (257, 255), (1, 0), (0, 1)):
        # the edge ends from the lower half, the centres from everywhere: neither array alone gives the count
        ea, eb, extra = indices(m, max(nu // 2, 1)), indices(m, max(nu // 2, 1)), indices(n_extra, nu)
        if n_extra >= 8:
            extra[5:8] = extra[2:5]                                   # the same centre more than once
        got = _touched(ctx, ea, eb, nu, extra)
        assert got == want(ea, eb, extra), (nu, m, n_extra, got)
    if nu > 4096 * 256:
        last = np.arange(4096 * 256 - 2, nu, dtype=np.uint32)         # both sides of where the second round starts
        assert _touched(ctx, last[::2], last[1::2], nu, none) == len(last)
        assert _touched(ctx, none, none, nu, last) == len(last)
        assert _touched(ctx, last[:1], last[:1], nu, last[-1:]) == 2
    assert _touched(ctx, none, none, 0, none) == 0
    assert _touched(ctx, [nu, NONE], [NONE, nu], nu, [nu, NONE, nu]) == 0


# ---- 5. bdg_assign_reads_dev ------------------------------------------------------------------------------------------------
def _uniq_arrays():
    rng = np.random.default_rng(31)
    mid = np.unique(rng.integers(1000, NONE - 1000, 3000, dtype=np.uint64)).astype(np.uint32)
    return {"none": np.zeros(0, np.uint32), "zero": np.array([0], np.uint32), "last": np.array([NONE], np.uint32),
            "one": np.array([77], np.uint32), "both_ends": np.array([0, NONE], np.uint32), "two": np.array([7, 900], np.uint32),
            "thousands": mid, "thousands_with_both_ends": np.concatenate([[0], mid, [NONE]]).astype(np.uint32)}


def _records(uniq, has, n, turn):
    """n records that go round the kinds of record there are, starting at kind `turn` -> (records, the kind of each)"""
    rng = np.random.default_rng(n * 8 + turn)
    L = len(uniq)
    recs = np.zeros(n, dtype=_native.REC_DTYPE)
    recs["polyT"], recs["r1_end"] = rng.integers(-1, 200, n), rng.integers(-1, 200, n)           # (fields the kernel must not care about)
    recs["valid"], recs["flags"] = 1, OK16
    kinds = []
    with_has, without = (np.flatnonzero(has), np.flatnonzero(has == 0)) if L else (np.zeros(0, np.intp),) * 2
    for i in range(n):
        kind = ("present", "below", "between", "above", "not_valid", "no_rank_flag", "has_not", "present_reverse_strand")[(i + turn) % 8]
        pick = lambda idx: int(uniq[idx[rng.integers(0, len(idx))]])                              # noqa: E731
        r = None
        if kind in ("present", "not_valid", "no_rank_flag", "present_reverse_strand") and len(with_has):
            r = pick(with_has)
        elif kind == "has_not" and len(without):
            r = pick(without)
        elif kind == "below" and L and uniq[0] > 0:
            r = int(rng.integers(0, uniq[0]))
        elif kind == "above" and L and uniq[-1] < NONE:
            r = int(rng.integers(int(uniq[-1]) + 1, NONE + 1))
        elif kind == "between" and L >= 2:
            j = int(rng.integers(0, L - 1))
            r = int(uniq[j]) + 1 if uniq[j + 1] - uniq[j] > 1 else None
        if r is None:                                                 # this array has no such rank: any rank, whatever it meets
            kind, r = "any", int(rng.integers(0, NONE + 1))
        recs["bc_rank"][i] = r
        if kind == "not_valid":
            recs["valid"][i] = 0
        elif kind == "no_rank_flag":
            recs["flags"][i] = _native.FLAG_BC16 | _native.FLAG_REV
        elif kind == "present_reverse_strand":
            recs["flags"][i] = OK16 | _native.FLAG_REV
            recs["valid"][i] = 1 + int(rng.integers(0, 2)) * 254      # (valid is a byte that is zero or not)
        kinds.append(kind)
    return recs, kinds


def _assigned_by_numpy(recs, uniq, assigned, has):
    L = len(uniq)
    pos = np.searchsorted(uniq, recs["bc_rank"])
    hit = (recs["valid"] != 0) & ((recs["flags"] & _native.FLAG_RANK_OK) != 0) & (pos < L)
    at = np.minimum(pos, max(L - 1, 0))
    if L:
        hit &= (uniq[at] == recs["bc_rank"]) & (has[at] != 0)
    else:
        hit[:] = False
    return np.where(hit, assigned[at] if L else 0, 0).astype(np.uint32), hit.astype(np.uint8)


@pytest.mark.parametrize("which", sorted(_uniq_arrays()))
def test_assign_reads(ctx, which):
    uniq = _uniq_arrays()[which]
    L = len(uniq)
    rng = np.random.default_rng(L)
    assigned = rng.integers(1, NONE + 1, L, dtype=np.uint64).astype(np.uint32)
    has = (rng.random(L) < 0.6).astype(np.uint8) if L > 2 else np.ones(L, np.uint8)
    d_uniq, d_assigned = _up(ctx, uniq), _up(ctx, assigned)
    seen = set()
    pad = 64                                                          # behind the n outputs: must stay as it was
    for has_now in ([has, np.zeros(L, np.uint8)] if 0 < L <= 2 else [has]):
        d_has = _up(ctx, has_now)
        for n in (1, 255, 256, 257):
            for turn in (range(8) if n == 1 else (0, 3)):
                recs, kinds = _records(uniq, has_now, n, turn)
                want_rank, want_has = _assigned_by_numpy(recs, uniq, assigned, has_now)
                d_recs = _up(ctx, recs.view(np.uint8).reshape(-1, 32))
                d_rank, d_got = _up(ctx, np.full(n + pad, 0xA5A5A5A5, np.uint32)), _up(ctx, np.full(n + pad, 0xA5, np.uint8))
                ctx.assign_reads_dev(d_recs, n, d_uniq, L, d_assigned, d_has, d_rank, d_got)
                got_rank, got_has = d_rank.to_host(), d_got.to_host()
                for d in (d_recs, d_rank, d_got):
                    d.free()
                assert (got_rank[n:] == 0xA5A5A5A5).all() and (got_has[n:] == 0xA5).all(), (which, n, "written behind the end")
                bad = np.flatnonzero((got_rank[:n] != want_rank) | (got_has[:n] != want_has))
                assert not len(bad), (which, n, turn, [(int(i), kinds[i], int(recs["bc_rank"][i]), int(got_rank[i]), int(got_has[i]),
                                                        int(want_rank[i]), int(want_has[i])) for i in bad[:6]])
                # every "no" is rank 0 and has 0 (what the writer relies on), every "yes" the barcode's assignment
                for i, kind in enumerate(kinds):
                    if kind in ("present", "present_reverse_strand"):
                        assert want_has[i] == 1 and want_rank[i] == assigned[np.searchsorted(uniq, recs["bc_rank"][i])] != 0
                    elif kind != "any":
                        assert want_has[i] == 0 and want_rank[i] == 0, kind
                seen.update(kinds)
        d_has.free()
    for d in (d_uniq, d_assigned):
        d.free()
    need = {"none": {"any"}, "zero": {"present", "above", "not_valid", "no_rank_flag"}, "last": {"present", "below"},
            "one": {"present", "below", "above"}, "both_ends": {"present", "between"}, "two": {"present", "below", "between", "above"},
            "thousands": {"present", "below", "between", "above", "not_valid", "no_rank_flag", "has_not", "present_reverse_strand"},
            "thousands_with_both_ends": {"present", "between", "has_not"}}[which]
    assert need <= seen, (which, need - seen)


# ---- 6. bdg_keep_observed ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 1, 257))
def test_keep_observed_records(n):
    """k_records_of_observed writes whole records: all 32 bytes of each as documented, whatever the buffer held before; and
    the distinct barcodes counted from them are numpy's"""
    rng = np.random.default_rng(n)
    ctx = _native.Context(0)
    try:
        # (something else first, so that the kept buffer has held other bytes)
        ctx.keep_observed(np.full(300, 0xDEADBEEF, np.uint32), np.ones(300, np.uint8))
        assert ctx.kept_records()[1] == 300
        for turn in range(2 if n == 1 else 1):
            rank = rng.integers(0, NONE + 1, n, dtype=np.uint64).astype(np.uint32)
            usable = rng.random(n) < 0.6
            if n == 1:
                usable[0] = turn == 0
                rank[0] = NONE
            if n > 8:
                rank[[0, 3, 5, 200, 256]] = [0, NONE, 0, NONE, 7]
                rank[100:120] = rank[130:150]                         # (barcodes seen more than once)
                usable[[0, 1, 3, 5, 6, 256]] = [True, False, True, False, True, True]
            ctx.keep_observed(rank, usable)
            ptr, kept = ctx.kept_records()
            assert kept == n and (ptr != 0 or n == 0)
            want = np.zeros(n, dtype=_native.REC_DTYPE)
            want["polyT"] = want["r1_end"] = -1
            want["bc_rank"] = np.where(usable, rank, 0)
            want["valid"] = usable
            want["flags"] = np.where(usable, OK16, 0)
            got = ctx.kept_records_to_host()
            assert got.dtype == _native.REC_DTYPE and got.itemsize == 32 and got.tobytes() == want.tobytes()
            d_uniq, d_cnt, d_first = (_native.DeviceArray(ctx, max(n, 1), np.uint32) for _ in range(3))
            d_n = _up(ctx, np.array([12345, 678], np.uint32))
            ctx.distinct_dev(ptr, n, d_uniq, d_cnt, d_first, d_n)
            nu, nbad = (int(x) for x in d_n.to_host())
            wu, wf, wc = np.unique(rank[usable], return_index=True, return_counts=True)
            assert nbad == 0 and nu == len(wu)
            if nu:
                assert (d_uniq.to_host(nu) == wu).all() and (d_cnt.to_host(nu) == wc).all()
                assert (d_first.to_host(nu) == np.flatnonzero(usable)[wf]).all()
            for d in (d_uniq, d_cnt, d_first, d_n):
                d.free()
    finally:
        ctx.close()


# ---- 7. the driver's device path with centres that were never observed ---------------------------------------------------
def test_driver_with_absent_and_repeated_true_barcodes(ctx):
    """Stage2.cluster / disconnected() with the edges on the device only, --true_barcodes naming barcodes below, between and
    above the observed ones and one observed barcode twice: the owners and the printed count of the host path"""
    rng = np.random.default_rng(17)
    nu, m = 5000, 9000
    uniq = np.unique(rng.integers(1000, NONE - 1000, nu + 50, dtype=np.uint64))[:nu].astype(np.uint32)
    ea = rng.integers(0, nu, m).astype(np.uint32)
    eb = ((ea + rng.integers(1, nu, m)) % nu).astype(np.uint32)
    ea[:40], eb[:40] = np.arange(40), np.arange(40) + 2000            # (barcodes 0 .. 39 have an edge for certain)
    seen = rng.choice(nu, 400, replace=False)
    seen[:3] = [0, nu - 1, 17]
    absent = [5, int(uniq[100]) + 1, NONE - 3, NONE]
    assert not np.isin(absent, uniq).any() and uniq[101] != uniq[100] + 1
    true_bcs = [unrank(int(uniq[i]), 16) for i in seen[:200]] + [unrank(a, 16) for a in absent[:2]] + \
               [unrank(int(uniq[i]), 16) for i in seen[200:]] + [unrank(a, 16) for a in absent[2:]] + \
               [unrank(int(uniq[seen[9]]), 16), unrank(absent[1], 16)]                           # one observed and one absent: twice

    def stage2():
        st = Stage2(1)
        st.uniq, st.count, st.first = uniq, np.ones(nu, np.int64), np.arange(nu, dtype=np.int64)
        return st

    ref = stage2()
    ref.ea, ref.eb = ea, eb
    with redirect_stdout(io.StringIO()):
        ref.cluster(true_bcs, None, 10, 16, 100)
    assert len(ref.centers) == len(true_bcs) == 406
    dev = stage2()
    dev.ea = dev.eb = None                                           # (the edges exist on the device only, as after build_edges)
    dev._edges = EdgeRows(ctx, dev._own(_up(ctx, np.stack([ea, eb]))), m)
    with redirect_stdout(io.StringIO()) as o:
        dev.cluster(true_bcs, None, 10, 16, 100)
    assert o.getvalue() == "1\n2\n" and dev._ea is None
    assert dev.owner.dtype == np.int64 and (dev.owner == ref.owner).all()
    # and the walk's, so that the two paths are not merely wrong together
    walked = cc.walk(nu, zip(ea.tolist(), eb.tolist()), np.searchsorted(uniq, [c for c in ref.centers if c not in absent]).tolist())
    assert walked == ref.owner.tolist()
    assert (ref.owner[seen] == seen).all() and (ref.owner == -1).sum() > 50 and ((ref.owner >= 0) & (ref.owner != np.arange(nu))).sum() > 300
    # the count: barcodes without an edge that are no centre, less one for every distinct centre that was never observed
    touched = len(np.unique(np.concatenate([ea, eb, seen])))
    assert ref.disconnected() == nu - (touched + 4)
    assert dev.disconnected() == ref.disconnected() and dev._ea is None
    dev.release_device()
