"""bdg_umi_dedup_genes_dev and its host twin (csrc/umi_kernels.hip) against the rule (umi_dedup.dedup_per_gene): every read's
molecule code and every field of every group record after sorting, on the inputs of tests/umi_gene_cases.py; group tables at
load 0.5, with probes that wrap past the last slot, one hot group, groups of one read, the extreme ordinals, every clause of the
rule, shuffled order, the workspace reused and shared with bdg_umi_dedup_dev, a second context, a cap one short, the argument
checks.  Integers only: every comparison is exact."""
import numpy as np
import pytest

import umi_cases as uc
import umi_gene_cases as ug
from badger_amd import _native
from badger_amd import umi_dedup as ud
from test_umi_kernels_gpu import _device as _cell_device, _same as _cell_same, _slot_of

pytestmark = pytest.mark.gpu

POISON = 0xAB
POISON32 = POISON * 0x01010101


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _poisoned(ctx, n):
    return _native.DeviceArray.from_host(ctx, np.full(max(n, 1), POISON32, dtype=np.uint32))


def _device(ctx, case, umi_len, dist, cap=None):
    """bdg_umi_dedup_genes_dev on the case, outputs poisoned first -> (molecule code per read, group records sorted)"""
    n = case.n
    cap = n if cap is None else cap
    d = [_native.DeviceArray.from_host(ctx, a if len(a) else np.zeros(1, a.dtype)) for a in (case.cell, case.recs, case.umi)]
    d_mol, d_groups, d_n = _poisoned(ctx, n), _poisoned(ctx, 6 * (cap + 4)), _poisoned(ctx, 1)
    try:
        ctx.umi_dedup_genes_dev(d[0], d[1], d[2], n, umi_len, dist, d_mol, d_groups, cap, d_n)
        count = int(d_n.to_host()[0])
        raw = d_groups.to_host()
        assert count <= cap and (raw[6 * count:] == POISON32).all()       # nothing behind the records was touched
        groups = raw[:6 * count].view(_native.GENE_GROUP_DTYPE)
        return d_mol.to_host()[:n], _native.sort_gene_groups(groups)
    finally:
        for a in d + [d_mol, d_groups, d_n]:
            a.free()


def _same(case, got, want, what):
    (gm, gg), (wm, wg) = got, want
    bad = np.nonzero(gm != wm)[0]
    if len(bad):
        rows = ["read %d cell %d feature %d flags %d UMI %r: got %#x want %#x" % (
            i, case.cell[i], case.recs["feature"][i], case.recs["flags"][i], case.umi_text[i], gm[i], wm[i]) for i in bad[:6].tolist()]
        raise AssertionError("%s %s: %d of %d molecules differ from the rule\n  %s" % (case.name, what, len(bad), case.n, "\n  ".join(rows)))
    assert len(gg) == len(wg), "%s %s: %d group records, the rule has %d" % (case.name, what, len(gg), len(wg))
    bad = np.nonzero(gg != wg)[0]
    if len(bad):
        rows = ["got %s want %s" % (gg[j], wg[j]) for j in bad[:6].tolist()]
        raise AssertionError("%s %s: %d of %d group records differ from the rule (feature, cell, molecules, umis, umi_reads, own)\n  %s"
                             % (case.name, what, len(bad), len(wg), "\n  ".join(rows)))


def _both(ctx, case, umi_len, dist, what):
    want = ug.rule(case, umi_len, dist)
    _same(case, _device(ctx, case, umi_len, dist), want, what + " (device arrays)")
    _same(case, ctx.umi_dedup_genes(case.cell, case.recs, case.umi, umi_len, dist), want, what + " (host arrays)")
    return want


_GENE_CASES = {}


def _gene_case(name, umi_len):
    if (name, umi_len) not in _GENE_CASES:
        base = uc.dense(umi_len, n=12000) if name == "dense" else uc.case(name, umi_len)
        _GENE_CASES[(name, umi_len)] = ug.from_umi_case(base)
    return _GENE_CASES[(name, umi_len)]


# ---- 1. the generators of umi_cases.py, features dealt over each cell ------------------------------------------------------
@pytest.mark.parametrize("name", ("dense", "ladders", "runs", "codes", "cells3000"))
@pytest.mark.parametrize("umi_dist", (0, 1))
@pytest.mark.parametrize("umi_len", (3, 10, 12))
def test_device_equals_the_rule(ctx, umi_len, umi_dist, name):
    case = _gene_case(name, umi_len)
    want = _both(ctx, case, umi_len, umi_dist, "umi_len %d dist %d" % (umi_len, umi_dist))
    if name in ("dense", "ladders") and umi_dist:
        assert want[1]["molecules"].sum() < ug.rule(case, umi_len, 0)[1]["molecules"].sum()      # (distance 1 merges here)
    if name == "dense":
        assert len(want[1]) > len(np.unique(case.cell))                                         # (several genes per cell)


# ---- 2. group tables as full as they get, and probes that wrap ---------------------------------------------------------------
@pytest.mark.parametrize("n", (512, 1024))
def test_group_table_at_load_one_half(ctx, n):
    case = ug.distinct_groups(n, seed=n)
    for dist in (0, 1):
        want = _both(ctx, case, 12, dist, "n %d dist %d" % (n, dist))
        assert len(want[1]) == n and (want[1]["molecules"] == 1).all()


def _occupied(case, P):
    """the slots linear probing fills with the case's group keys (the same set in any insertion order), and how many keys
    sit below their home slot: they went past the last slot"""
    keys = case.cell.astype(np.uint64) << np.uint64(32) | case.recs["feature"].astype(np.uint64)
    assert len(np.unique(keys)) == case.n
    used = np.zeros(P, bool)
    wrapped = 0
    for h in _slot_of(keys, P - 1).tolist():
        s = h
        while used[s]:
            s = (s + 1) & (P - 1)
        used[s] = True
        wrapped += s < h
    return used, wrapped


def test_group_probe_wrap(ctx):
    """forty sets of 512 distinct group keys: the 1,024-slot group table is half full, and in some of them the occupied slots
    run from the last slot on to the first, so claims and lookups go round the end"""
    spanning = wrapping = 0
    for seed in range(40):
        case = ug.distinct_groups(512, seed=9000 + seed, umi_len=10 if seed % 2 else 12)
        used, wrapped = _occupied(case, 1024)
        assert used.sum() == 512
        spanning += bool(used[1023] and used[0])
        wrapping += wrapped > 0
        _same(case, _device(ctx, case, 10 if seed % 2 else 12, 1), ug.rule(case, 10 if seed % 2 else 12, 1), "wrap seed %d" % seed)
    print("sets with slots 1023 and 0 both taken: %d, with a key stored past the end: %d" % (spanning, wrapping))
    assert spanning >= 5 and wrapping >= 1


# ---- 3. one address, many addresses, the extreme ordinals --------------------------------------------------------------------
@pytest.mark.parametrize("umi_len", (3, 10, 12))
def test_one_hot_group(ctx, umi_len):
    case = ug.hot_group(umi_len)
    want = _both(ctx, case, umi_len, 1, "hot group")
    assert len(want[1]) == 1 and want[1]["umi_reads"][0] + want[1]["own"][0] == 20000 and want[1]["own"][0] == 400
    ctx.umi_dedup_genes_set_aggregate(False)                         # every lane for itself: the same answers
    try:
        _same(case, _device(ctx, case, umi_len, 1), want, "hot group, lanes on their own")
        mixed = _gene_case("ladders", umi_len)
        _same(mixed, _device(ctx, mixed, umi_len, 1), ug.rule(mixed, umi_len, 1), "ladders, lanes on their own")
    finally:
        ctx.umi_dedup_genes_set_aggregate(True)


def test_groups_of_one_read(ctx):
    case = ug.single_read_groups(3000)
    for dist in (0, 1):
        want = _both(ctx, case, 12, dist, "singles dist %d" % dist)
        assert len(want[1]) == 3000 and (want[1]["molecules"] == 1).all() and want[1]["own"].sum() == len(range(0, 3000, 7))


def test_extreme_ordinals(ctx):
    case = ug.extremes()
    for dist in (0, 1):
        want = _both(ctx, case, 12, dist, "extremes dist %d" % dist)
        assert [(int(g["cell"]), int(g["feature"])) for g in want[1]] == [(0, 0), (0, 0xFFFFFFFE), (0xFFFFFFFE, 0), (0xFFFFFFFE, 0xFFFFFFFE)]
        assert len(set(want[1]["molecules"].tolist())) == 1          # (the same family in each: nothing crossed over)


@pytest.mark.parametrize("k", range(len(ug.CLAUSES)))
def test_every_clause(ctx, k):
    case, _, _ = ug.clause_case(k)
    want = ug.clause_arrays(k)
    _same(case, _device(ctx, case, 10, 1), want, "by hand (device arrays)")
    _same(case, ctx.umi_dedup_genes(case.cell, case.recs, case.umi, 10, 1), want, "by hand (host arrays)")


def test_no_reads_and_one_read(ctx):
    empty = ug.GeneCase("nothing", [])
    mol, groups = _device(ctx, empty, 12, 1)
    assert len(mol) == 0 and len(groups) == 0
    mol, groups = ctx.umi_dedup_genes(empty.cell, empty.recs, empty.umi, 12, 1)
    assert len(mol) == 0 and len(groups) == 0
    one = ug.GeneCase("one", [(7, 3, ug.A, "ACGTACGTACGT")])
    want = _both(ctx, one, 12, 1, "one read")
    assert want[0].tolist() == [ud.umi_code("ACGTACGTACGT")] and want[1].tolist() == [(3, 7, 1, 1, 1, 0)]
    lone = ug.GeneCase("one outside", [(7, 3, ug.gn.TIE, "ACGTACGTACGT")])
    want = _both(ctx, lone, 12, 1, "one read that takes no part")
    assert want[0].tolist() == [ug.NONE] and len(want[1]) == 0


# ---- 4. order, reuse, contexts, the shared workspace -------------------------------------------------------------------------
def test_same_answer_in_any_order_on_any_context_in_any_workspace(ctx):
    case = _gene_case("dense", 12)
    want = ug.rule(case, 12, 1)
    first = _device(ctx, case, 12, 1)
    _same(case, first, want, "first")
    shuffled, perm = case.shuffled(21)
    got = _device(ctx, shuffled, 12, 1)
    assert (got[0] == first[0][perm]).all() and got[1].tobytes() == first[1].tobytes()
    # a small call in the workspace a large call left behind, and the large one again
    big = ug.from_umi_case(uc.dense(12, n=1 << 16, seed=9), seed=4)
    want_big = ug.rule(big, 12, 1)
    _same(big, _device(ctx, big, 12, 1), want_big, "large call")
    small = ug.distinct_groups(300, seed=300)
    _same(small, _device(ctx, small, 12, 1), ug.rule(small, 12, 1), "small call after a large one")
    _same(big, _device(ctx, big, 12, 1), want_big, "large call again")
    other = _native.Context(0)
    try:
        again = _device(other, case, 12, 1)
    finally:
        other.close()
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()


def test_the_shared_workspace_does_not_leak(ctx):
    """bdg_umi_dedup_dev on the context the per-gene call just used, and the per-gene call after it"""
    gene = _gene_case("ladders", 12)
    cell = uc.case("dense", 12)
    _same(gene, _device(ctx, gene, 12, 1), ug.rule(gene, 12, 1), "before")
    _cell_same(cell, _cell_device(ctx, cell, 12, 1), uc.rule(cell, 12, 1), "bdg_umi_dedup_dev after the per-gene call")
    _same(gene, _device(ctx, gene, 12, 1), ug.rule(gene, 12, 1), "after bdg_umi_dedup_dev")
    small = uc.distinct_keys(12, 300, seed=300)
    _cell_same(small, _cell_device(ctx, small, 12, 1), uc.rule(small, 12, 1), "a small bdg_umi_dedup_dev after it")


# ---- 5. rejections -----------------------------------------------------------------------------------------------------------
def test_cap_one_short(ctx):
    case = ug.single_read_groups(700)
    want = ug.rule(case, 12, 1)
    assert len(want[1]) == 700
    d = [_native.DeviceArray.from_host(ctx, a) for a in (case.cell, case.recs, case.umi)]
    d_mol, d_groups, d_n = _poisoned(ctx, case.n), _poisoned(ctx, 6 * 700), _poisoned(ctx, 1)
    try:
        with pytest.raises(_native.BadgerHipError, match="700 groups"):
            ctx.umi_dedup_genes_dev(d[0], d[1], d[2], case.n, 12, 1, d_mol, d_groups, 699, d_n)
        assert int(d_n.to_host()[0]) == 700                          # the number needed
        raw = d_groups.to_host()
        assert (raw[6 * 699:] == POISON32).all() and not (raw[:6 * 699] == POISON32).any()     # 699 records, none past them
        with pytest.raises(_native.BadgerHipError, match="700 groups"):
            ctx.umi_dedup_genes(case.cell, case.recs, case.umi, 12, 1, cap=699)
        with pytest.raises(_native.BadgerHipError, match="700 groups"):
            ctx.umi_dedup_genes_dev(d[0], d[1], d[2], case.n, 12, 1, d_mol, 0, 0, d_n)       # no room at all, and no array
        ctx.umi_dedup_genes_dev(d[0], d[1], d[2], case.n, 12, 1, d_mol, d_groups, 700, d_n)  # exactly enough
        assert int(d_n.to_host()[0]) == 700
        groups = _native.sort_gene_groups(d_groups.to_host().view(_native.GENE_GROUP_DTYPE))
        _same(case, (d_mol.to_host(), groups), want, "cap equal to the need")
    finally:
        for a in d + [d_mol, d_groups, d_n]:
            a.free()


def test_rejections_launch_nothing(ctx):
    case = _gene_case("codes", 12)
    n = case.n
    d = [_native.DeviceArray.from_host(ctx, a) for a in (case.cell, case.recs, case.umi)]
    d_mol, d_groups, d_n = _poisoned(ctx, n), _poisoned(ctx, 6 * n), _poisoned(ctx, 1)
    good = dict(d_cell=d[0], d_gene_recs=d[1], d_umi=d[2], n=n, umi_len=12, umi_dist=1, d_molecule=d_mol, d_groups=d_groups, cap=n,
                d_n_groups=d_n)
    bad = [dict(umi_dist=2), dict(umi_len=2), dict(umi_len=13), dict(d_cell=0), dict(d_gene_recs=0), dict(d_umi=0), dict(d_molecule=0),
           dict(d_groups=0), dict(d_n_groups=0), dict(n=(1 << 30) + 1)]
    try:
        for change in bad:
            with pytest.raises(_native.BadgerHipError):
                ctx.umi_dedup_genes_dev(**dict(good, **change))
            # nothing ran: the outputs still hold the poison
            assert all((a.to_host() == POISON32).all() for a in (d_mol, d_groups, d_n)), change
        ctx.umi_dedup_genes_dev(**good)                              # the context still works
        count = int(d_n.to_host()[0])
        groups = _native.sort_gene_groups(d_groups.to_host()[:6 * count].view(_native.GENE_GROUP_DTYPE))
        _same(case, (d_mol.to_host(), groups), ug.rule(case, 12, 1), "after the rejections")
    finally:
        for a in d + [d_mol, d_groups, d_n]:
            a.free()
    lib = _native.load()
    assert lib.bdg_umi_dedup_genes_dev(None, None, None, None, 0, 12, 1, None, None, 0, None) == _native.E_ARG
    assert lib.bdg_umi_dedup_genes(None, None, None, None, 0, 12, 1, None, None, 0, None) == _native.E_ARG
    for kw in (dict(umi_len=2), dict(umi_len=13), dict(umi_dist=2)):
        with pytest.raises(_native.BadgerHipError):
            ctx.umi_dedup_genes(case.cell, case.recs, case.umi, **dict(dict(umi_len=12, umi_dist=1), **kw))
