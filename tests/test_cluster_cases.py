"""The inputs of tests/cluster_cases.py hold what they are for, checked without a GPU: the reference walk
(badger_amd.barcode_graph.BarcodeGraph.cluster) equals the rule as the kernels state it on every case; the walk itself does not
depend on the order of the centre list or of the edges; Stage2.cluster's host array path gives the walk's owners on the packed
union and on every scale shape; every wrong variant of the rule in MUTANTS is told from the walk by the case set; and every
decision the kernels have to get right occurs in it.  A generator that stops producing the hard cases fails here, before
tests/test_cluster_gpu.py quietly stops testing them.

This file takes about 25 s on one CPU core: the walk over the case set 1.6 s, the order checks 2.5 s, the seven mutants 5 s, the
walk over each of the three unions 3 to 4 s, the shapes 2 s."""
from collections import Counter
from itertools import permutations

import numpy as np
import pytest

import cluster_cases as cc


def _centres(pk):
    return np.flatnonzero(pk.owner_in >= 0)


# ---- rule and model ---------------------------------------------------------------------------------------------------------
def test_the_case_set_is_every_small_graph_and_a_sample():
    small = cc.small_graph_cases(5)
    # per vertex count: 2^(pairs) graphs x 2^n centre sets
    assert Counter(c.n for c in small) == {n: 2 ** (n * (n - 1) // 2 + n) for n in range(1, 6)}
    assert len(set(small)) == len(small) == 33866
    assert len(cc.small_graph_cases(3)) == 2 + 8 + 64
    sample = cc.sampled_cases()
    assert {c.n for c in sample} == {6, 7, 8, 9} and sample == cc.sampled_cases(cc.SAMPLE_SEED) and sample[:50] != cc.sampled_cases(1)[:50]
    cases, owners = cc.gpu_cases()
    assert cases == small + sample and len(owners) == len(cases) and all(len(o) == c.n for c, o in zip(cases, owners))


def test_walk_equals_the_rule_model_on_every_case():
    cases, owners = cc.gpu_cases()
    bad = [(c, o, cc.rule_model(*c)) for c, o in zip(cases, owners) if cc.rule_model(*c) != o]
    assert not bad, (len(bad), bad[0])


# ---- the walk does not depend on an order ---------------------------------------------------------------------------------
def test_walk_gives_the_same_for_every_centre_order_up_to_four_vertices():
    cases, owners = cc.gpu_cases()
    orders = 0
    for c, want in zip(cases, owners):
        if c.n > 4:
            continue
        for order in permutations(c.centres):
            orders += 1
            assert cc.walk(c.n, c.edges, order) == want, (c, order)
    assert orders > 4000


def test_walk_gives_the_same_for_both_centre_and_edge_orders_on_five_vertices():
    cases, owners = cc.gpu_cases()
    n = 0
    for c, want in zip(cases, owners):
        if c.n != 5:
            continue
        n += 1
        back = tuple(reversed(c.edges))
        assert c.centres == tuple(sorted(c.centres))
        for cen in (c.centres, c.centres[::-1]):
            for edges in (c.edges, back):
                assert cc.walk(5, edges, cen) == want, (c, cen, edges)
    assert n == 32768


# ---- the packed union -------------------------------------------------------------------------------------------------------
def test_pack_numbers_the_union_at_random_with_owning_centres_first_and_last():
    cases, owners = cc.gpu_cases()
    pk = cc.packed("plain")
    nu = pk.nu
    assert nu == sum(c.n for c in cases) and sorted(pk.perm.tolist()) == list(range(nu))
    assert pk.ea.dtype == pk.eb.dtype == np.uint32 and pk.owner_in.dtype == pk.owner_want.dtype == np.int32
    assert len(pk.ea) == sum(len(c.edges) for c in cases) and pk.ea.max() < nu and pk.eb.max() < nu
    # owner_in: a centre holds its own index, everything else -2; owner_want is the walk's answer, renumbered
    cen = _centres(pk)
    assert (pk.owner_in[cen] == cen).all() and (pk.owner_in[pk.owner_in < 0] == -2).all() and len(cen) == sum(len(c.centres) for c in cases)
    for i in (0, 1, 40000, len(cases) - 1):
        verts = pk.perm[pk.base[i]:pk.base[i + 1]]
        want = [int(verts[o]) if o >= 0 else o for o in owners[i]]
        assert pk.owner_want[verts].tolist() == want and cc.case_of(pk, int(verts[-1]))[0] == i
    # the edges are the cases' edges: every edge stays inside its case
    inv = np.argsort(pk.perm)
    ca, cb = np.searchsorted(pk.base, inv[pk.ea], side="right"), np.searchsorted(pk.base, inv[pk.eb], side="right")
    assert (ca == cb).all()
    # turned at random, in no order, and a centre's index says nothing about its case
    turned = (pk.ea > pk.eb).mean()
    assert 0.45 < turned < 0.55 and 0.45 < (np.diff(pk.ea.astype(np.int64)) > 0).mean() < 0.55
    assert abs(np.corrcoef(cen, inv[cen])[0, 1]) < 0.02
    # vertex 0 and the last vertex: centres with a neighbour that they alone reach
    for v in (0, nu - 1):
        assert pk.owner_in[v] == v
        nb = np.concatenate([pk.eb[pk.ea == v], pk.ea[pk.eb == v]])
        assert len(nb) and ((pk.owner_want[nb] == v) & (pk.owner_in[nb] == -2)).any()
    # another seed is another numbering; a few cases pack without the walk handed in
    other = cc.pack(cases[:3000], 8)
    assert other.nu == sum(c.n for c in cases[:3000]) and (other.owner_in[[0, other.nu - 1]] == [0, other.nu - 1]).all()
    with pytest.raises(ValueError):
        cc.pack(cases[:2], 1)                                        # (one vertex, no edge: no centre owns a neighbour)


def test_the_variants_hold_the_same_graph():
    plain, doubled, loops = (cc.packed(v) for v in cc.VARIANTS)
    key = lambda a, b: np.sort(a.astype(np.uint64) << np.uint64(32) | b.astype(np.uint64))       # noqa: E731
    for pk in (doubled, loops):
        assert (pk.owner_in == plain.owner_in).all() and (pk.owner_want == plain.owner_want).all() and (pk.perm == plain.perm).all()
    # doubled: every edge once in each orientation
    assert len(doubled.ea) == 2 * len(plain.ea) and (key(doubled.ea, doubled.eb) == key(doubled.eb, doubled.ea)).all()
    assert (key(doubled.ea, doubled.eb) == np.sort(np.concatenate([key(plain.ea, plain.eb), key(plain.eb, plain.ea)]))).all()
    # loops: the plain edges and an edge (v, v) on a third of the vertices, each once
    self_edge = loops.ea == loops.eb
    assert self_edge.sum() == plain.nu // 3 == len(np.unique(loops.ea[self_edge])) and not (plain.ea == plain.eb).any()
    assert (key(loops.ea[~self_edge], loops.eb[~self_edge]) == key(plain.ea, plain.eb)).all()
    looped = np.zeros(plain.nu, bool)
    looped[loops.ea[self_edge]] = True
    for what in (plain.owner_in >= 0, plain.owner_want == -2, plain.owner_want == -1, (plain.owner_want >= 0) & (plain.owner_in < 0)):
        assert (looped & what).sum() > 1000                          # on centres, on members, on nobody's, on the unreached


@pytest.mark.parametrize("variant", cc.VARIANTS)
def test_walk_and_host_array_path_give_owner_want_on_the_union(variant):
    """The walk over the whole union - the centres in the order of the random numbering, every vertex's neighbours in the order
    of the shuffled edges, doubled edges and self-loops as they come - gives what the cases gave one by one; so does
    Stage2.cluster's host array path."""
    pk = cc.packed(variant)
    cen = _centres(pk)
    got = np.array(cc.walk(pk.nu, zip(pk.ea.tolist(), pk.eb.tolist()), cen.tolist()))
    assert (got == pk.owner_want).all(), cc.describe_first_difference(pk, got)
    got = cc.host_owner(pk.nu, pk.ea, pk.eb, cen[::-1])
    assert got.dtype == np.int64 and (got == pk.owner_want).all(), cc.describe_first_difference(pk, got)


def test_first_difference_is_reported_in_the_cases_own_numbers():
    pk = cc.packed("plain")
    assert cc.describe_first_difference(pk, pk.owner_want) == ""
    v = int(pk.perm[pk.base[33000] + 2])
    got = pk.owner_want.copy()
    got[v] = -1 if got[v] != -1 else -2
    text = cc.describe_first_difference(pk, got)
    c = pk.cases[33000]
    assert "case 33000" in text and str(list(c.edges)) in text and "centres %s" % list(c.centres) in text and "1 of %d" % pk.nu in text


# ---- mutants ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", sorted(cc.MUTANTS))
def test_the_case_set_rejects_the_mutant(mutant):
    cases, owners = cc.gpu_cases()
    sizes = Counter(c.n for c, o in zip(cases, owners) if cc.rule_model(*c, mutant=mutant) != o)
    differ, five = sum(sizes.values()), sizes[5]
    print("%s: %d of %d cases differ from the walk, %d of them on five vertices" % (mutant, differ, len(cases), five))
    assert differ >= 1 and five >= 1


def test_mutants_are_the_named_ones():
    assert set(cc.MUTANTS) == {"one_direction", "hi_gt_0", "first_offer_wins", "count_offers", "conflict_node_retakes", "third_level",
                               "merged_levels"}
    with pytest.raises(KeyError):
        cc.rule_model(1, (), (), mutant="no_such_mutant")
    # the smallest graphs that tell them apart, by hand
    assert cc.rule_model(2, ((1, 0),), (0,)) == [0, 0] and cc.rule_model(2, ((1, 0),), (0,), "one_direction") == [0, -2]
    assert cc.rule_model(2, ((0, 1),), (0,), "hi_gt_0") == [0, -2]
    assert cc.rule_model(3, ((0, 1), (1, 2)), (0, 2)) == [0, -1, 2] and cc.rule_model(3, ((0, 1), (1, 2)), (0, 2), "first_offer_wins") == [0, 0, 2]
    square = ((0, 1), (0, 2), (1, 3), (2, 3))
    assert cc.rule_model(4, square, (0,)) == [0, 0, 0, 0] and cc.rule_model(4, square, (0,), "count_offers") == [0, 0, 0, -1]
    y = ((0, 1), (1, 2), (2, 3), (3, 4))                              # centres 0 and 2 meet at 1; 3 is 2's; 4 is 2's on level 2
    assert cc.rule_model(5, y, (0, 2)) == [0, -1, 2, 2, 2]
    tail = ((0, 1), (1, 2), (2, 3), (1, 4))                           # 1 is nobody's after level 1; 2 beside it is 3's
    assert cc.rule_model(5, tail, (0, 4, 3)) == [0, -1, 3, 3, 4] and cc.rule_model(5, tail, (0, 4, 3), "conflict_node_retakes") == [0, 3, 3, 3, 4]
    path = ((0, 1), (1, 2), (2, 3))
    assert cc.rule_model(4, path, (0,)) == [0, 0, 0, -2]
    assert cc.rule_model(4, path, (0,), "third_level") == [0, 0, 0, 0] and cc.rule_model(4, path, (0,), "merged_levels") == [0, 0, 0, 0]


# ---- what the case set holds ------------------------------------------------------------------------------------------------
def test_every_decision_occurs():
    cases, owners = cc.gpu_cases()
    small, sample = Counter(), Counter()
    for c, o in zip(cases, owners):
        (small if c.n <= 5 else sample).update(cc.coverage(*c, o))
    print("up to five vertices:", dict(small))
    print("sample:", dict(sample))
    for what in cc.COUNTERS:
        if what != "three_centres_l2":                                # (needs seven vertices)
            assert small[what] > 0, what
        assert sample[what] > 0, what
    # the sample is there for what five vertices cannot hold: a second level that meets three other clusters, long paths
    assert small["three_centres_l2"] == 0 and sample["three_centres_l2"] >= 10
    assert sum(1 for c, o in zip(cases, owners) if c.n >= 7 and sum(1 for x in o if x == -2) >= 3 and len(c.edges) >= c.n - 1) > 100
    # in the union: the centre at position 0 and the one at the last position each own a neighbour
    pk = cc.packed("plain")
    assert pk.owner_in[0] == 0 and (pk.owner_want[1:] == 0).sum() >= 1
    assert pk.owner_in[-1] == pk.nu - 1 and (pk.owner_want[:-1] == pk.nu - 1).sum() >= 1
    # by hand on one graph: 0 and 4 are centres, 1 is between them, 2 hangs on 1; 5 - 6 - 7 hang on centre 4, 8 on 7
    edges = ((0, 1), (1, 4), (1, 2), (4, 5), (5, 6), (6, 7), (7, 8))
    o = cc.walk(9, edges, (0, 4))
    assert o == [0, -1, -2, -2, 4, 4, 4, -2, -2]
    k = cc.coverage(9, edges, (0, 4), o)
    assert k == dict(l1_conflict=1, l2_conflict=0, l2_owned=1, edge_but_unreached=3, l1_conflict_beside_unreached=1, same_centre_twice=0,
                     three_centres_l1=0, three_centres_l2=0)


# ---- scale and boundary shapes ----------------------------------------------------------------------------------------------
def test_shapes_are_the_listed_ones_and_the_host_path_equals_the_walk_on_them():
    shapes = {s.name: s for s in cc.shapes()}
    for d in (2, 255, 256, 257, 100000):
        s = shapes["hub_%d" % d]
        assert s.nu == d + 1 and len(s.ea) == d and len(s.centres) == d and s.owner_want[d] == -1
    for d in (2, 257, 100000):
        assert shapes["fan_%d" % d].owner_want[d + 1] == 0 and shapes["fan_%d_second" % d].owner_want[d + 1] == -1
        s = shapes["fan_%d_conflict" % d]
        assert s.owner_want[d + 1] == 0 and s.owner_want[d + 4] == -1
    assert shapes["fan_257_second_flipped"].owner_want[2] == -1 and shapes["fan_257_conflict_flipped"].owner_want[3] == 261
    assert shapes["path_4_centres_0"].owner_want.tolist() == [0, 0, 0, -2]
    assert shapes["path_5_centres_0"].owner_want.tolist() == [0, 0, 0, -2, -2]
    assert shapes["path_5_centres_0_4"].owner_want.tolist() == [0, 0, -1, 4, 4]
    assert {(s.nu, len(s.ea)) for s in shapes.values()} >= {(nu, m) for nu in (255, 256, 257) for m in (0, 1, 255, 256, 257)} | {(1, 0)}
    assert not len(shapes["no_centre"].centres) and (shapes["no_centre"].owner_want == -2).all() and len(shapes["no_centre"].ea) == 600
    assert (shapes["all_centres"].owner_want == np.arange(300)).all()
    assert shapes["one_vertex_a_centre"].owner_want.tolist() == [0] and shapes["one_vertex_no_centre"].owner_want.tolist() == [-2]
    for s in shapes.values():
        assert s.owner_want.dtype == s.owner_in.dtype == np.int32 and len(s.owner_want) == s.nu and len(s.ea) == len(s.eb)
        assert not len(s.ea) or max(s.ea.max(), s.eb.max()) < s.nu
        for v, o in s.pins:
            assert s.owner_want[v] == o, (s.name, v, o)
        walked = cc.walk(s.nu, zip(s.ea.tolist(), s.eb.tolist()), s.centres)
        assert walked == s.owner_want.tolist(), s.name
