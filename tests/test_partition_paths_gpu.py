"""Every path of the bucket partition and the block scan (csrc/bdg_partition.hpp) through the public entry points of its
consumers, on the inputs of tests/partition_cases.py: the distinct count against numpy.unique, the deletion-variant joins
against the oracle's whole edge list, the piece places of the chimera split against the Python rule, bit for bit.  Each case
first asserts, on its own input, that it reaches the path it is named for (tests/test_partition_cases.py does the same
without a GPU).  Needs a real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

import partition_cases as pc
from badger_amd import _native, chimera_split as cs, synth
from test_hip_parity import _GraphOnDevice, _parts_union_is

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


# --------------------------------------------------------------------------- the distinct count
def _distinct_is_numpys(ctx, case, what):
    import torch
    dev = torch.device("cuda", 0)
    n = case.n
    d_recs = torch.from_numpy(case.records().view(np.int32).reshape(-1, 8).copy()).to(dev)
    uniq, cnt, first = (torch.full((n,), -1, dtype=torch.int32, device=dev) for _ in range(3))
    dn = torch.full((2,), -1, dtype=torch.int32, device=dev)
    ctx.set_stream(0)
    ctx.distinct_dev(d_recs, n, uniq, cnt, first, dn)
    torch.cuda.synchronize()
    wu, wc, wf, w16 = case.want()
    nu = int(dn[0])
    assert nu == len(wu), (what, nu, len(wu))
    for got, want, name in ((uniq[:nu].cpu().numpy().view(np.uint32), wu, "ranks"), (cnt[:nu].cpu().numpy(), wc, "counts"),
                            (first[:nu].cpu().numpy(), wf, "first index")):
        bad = np.nonzero(got != want)[0]
        assert not len(bad), (what, name, len(bad), bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist(), ["%08x" % r for r in wu[bad[:5]]])
    assert int(dn[1]) == w16, (what, int(dn[1]), w16)


def _twice_with_a_small_call_between(ctx, case):
    """the case, a small call that reuses the workspace, the case again"""
    case.reaches()
    _distinct_is_numpys(ctx, case, (case.name, "first"))
    _distinct_is_numpys(ctx, pc.small_records(), (case.name, "small call"))
    _distinct_is_numpys(ctx, case, (case.name, "again"))


@pytest.mark.parametrize("name", pc.DISTINCT_NAMES)
def test_distinct_count_on_every_partition_path(ctx, name):
    """bdg_distinct_dev where k_part_split<unsigned long long> streams coarse buckets of 0, 1, 8,191, 8,192, 8,193, 16,384,
    16,385 and 24,577 pairs and one of several hundred thousand in rounds of 8,192 (l2 = 1 and l2 = 2, one sub-bucket holding
    all of a bucket, sub-buckets of 1 / 0 / 24,575 / 1), where the second level runs without sub-buckets (l2 = 0), with the
    ranks 0 and 0xFFFFFFFF (the hash table's two empty values) in direct and in cold-path buckets, and with 1,535 / 1,536 /
    1,537 different ranks in one bucket - numpy's unique, counts and first indices, and d_n[1], twice on one context."""
    _twice_with_a_small_call_between(ctx, pc.distinct_case(name))


@pytest.mark.parametrize("which", range(7))
def test_distinct_count_at_the_tile_edges(ctx, which):
    """n = 1, 255, 256, 257 and, with T = 8 tiles a compute unit, 256 T - 1, 256 T, 256 T + 1 records: the last tile of
    k_distinct_rows full, short by one, and holding one record"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = pc.tile_edge_sizes(cus)[which]
    _twice_with_a_small_call_between(ctx, pc.distinct_case("tile_edges/%d" % n, cus))


# --------------------------------------------------------------------------- the joins
@pytest.mark.parametrize("thr,kind", [(2, "random"), (2, "neighbours"), (1, "random"), (1, "neighbours")])
def test_joins_with_coarse_buckets_of_two_rounds(ctx, orc, thr, kind):
    """bdg_graph_edges with the deletion-variant join forced (algo 5 at thr 2: n = 70,000 rows; algo 6 at thr 1: n = 400,000
    rows), where every coarse bucket of k_part_split<uint32_t> holds 18,600 .. 19,800 entries (counted by the case: 70.7 and
    12.25 entries a row) and so is streamed in one full round of 16,384 and a partial one: the oracle's whole list, from one
    call and as the union of three parts.  "random": distinct random ranks; "neighbours": half of the rows are a random rank,
    the other half copies with one letter substituted, so that tens of thousands of groups all over the buckets hold an edge."""
    case = pc.join_case(thr, kind).reaches()
    T = orc.qgram_threshold(thr)
    want = orc.graph_edges(case.ranks, thr, T, threads=8)
    assert len(want) > (case.n // 4 if kind == "neighbours" else 100)
    try:
        ctx.graph_set_algo(case.algo)
        e = ctx.graph_edges(case.ranks, thr, T)
        assert len(e) == len(want), (len(e), len(want))
        assert (e == want).all()
        dev = _GraphOnDevice(ctx, case.ranks, len(want) + 1024)
        assert _parts_union_is(ctx, dev, 3, thr, T, want, status=True)
    finally:
        ctx.graph_set_algo(0)


# --------------------------------------------------------------------------- the piece places of the split
def _same_pieces(got, want, what):
    assert len(got[0]) == len(want[0]) and (got[0] == want[0]).all(), (what, "off'")
    assert got[1].dtype == _native.SPLIT_DTYPE == cs.SPLIT_DTYPE
    bad = np.nonzero(got[1] != want[1])[0]
    assert not len(bad), (what, bad[:5].tolist(), got[1][bad[:5]].tolist(), want[1][bad[:5]].tolist())


@pytest.mark.parametrize("n", list(pc.SPLIT_SIZES))
def test_split_places_over_several_scan_blocks(ctx, n):
    """bdg_split_batch on 2 x 16,384 + 5 reads (three blocks of the scan: k_scan_sums and k_scan_add run), on 16,384 (one
    block), on 16,385 (two, the second with one read) and on 16,386 (the first size at which a place is read that k_scan_add
    wrote): reads of ten bases with concatemers of 3 to 5 molecules at the first and last read, either side of every border
    between blocks and at every 997th read - off' and the piece records of the Python rule.  Then the device form with
    off[0] != 0 into poisoned buffers, with exactly enough room and with more."""
    import torch
    case = pc.split_case(n)
    bases, off = synth.list_to_reads(case.reads)
    want_off, want_rows = cs.split_batch(bases, off)
    assert case.reaches(want_rows) == pc.SPLIT_SIZES[n]
    _same_pieces(ctx.split_batch(bases, off), (want_off, want_rows), n)

    dev = torch.device("cuda", 0)
    total, n_out, lead = int(off[-1]), len(want_rows), 3
    d_bases = torch.zeros(lead + total + 64, dtype=torch.uint8, device=dev)
    d_bases[lead:lead + total] = torch.from_numpy(bases).to(dev)
    d_off = torch.from_numpy((off + np.uint64(lead)).astype(np.int64)).to(dev)
    ctx.set_stream(0)
    for cap in (n_out, n_out + 50):
        d_off_out = torch.full(((cap + 1) * 8,), 0xAB, dtype=torch.uint8, device=dev)
        d_rows = torch.full((cap * 12 + 4,), 0xAB, dtype=torch.uint8, device=dev)
        d_count = torch.full((8,), 0xAB, dtype=torch.uint8, device=dev)
        ctx.split_batch_dev(d_bases, d_off, n, cs.MAX_ED_DEFAULT, d_off_out, d_rows, cap, d_count)
        torch.cuda.synchronize()
        o, r = d_off_out.cpu().numpy(), d_rows.cpu().numpy()
        assert int(d_count.cpu().numpy().view(np.uint64)[0]) == n_out
        assert (o[:(n_out + 1) * 8].view(np.uint64) == want_off + np.uint64(lead)).all() and (o[(n_out + 1) * 8:] == 0xAB).all()
        assert r[:n_out * 12].tobytes() == want_rows.tobytes() and (r[n_out * 12:] == 0xAB).all()
