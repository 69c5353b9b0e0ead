"""k_sw_clusters hands the clusters its tail certificate leaves OPEN to one wave of the block (tests/sw_bound_cases.py has the
certificate and the reads).  The batches below put a known number of open clusters into ONE block of 512 queue-A entries,
around every count at which the kernel takes another path: none (the tail pass is skipped), 1, the list's capacity of 32
and one either side of it (a wave whose clusters no longer fit runs its own tail), 127 / 128 / 129, and all 512.

Every read holds exactly one queue-A cluster (asserted on the host), whose strict window is whole (n_s = 39: every wave has
ten head words).  Where a cluster lands follows from the scan: read i belongs to task i // 16, task t to shard t % 8, and
entry k of shard s is entry s + 8 * k of the queue, so
  * a batch of up to 128 reads has one task a shard and its order is fixed: read 16 * s + k is cluster s & 1 of lane
    4 * k + s / 2 of wave 0 of block 0, and waves 1-3 of that block see only holes (the block-uniform loop);
  * a batch of 512 reads fills block 0 alone, four tasks a shard and one of them a wave - which one is the scan's race, so
    these batches state their counts for the block and hold for any order within it;
  * 640 reads leave 128 entries for block 1, whose waves 1-3 are empty;
  * one task of 16 reads with four clusters each is 64 entries of shard 0: entries 8 * k, sixteen a wave, in the task's
    order - the clusters of reads 12-15 are wave 3's.
Records are compared with oracle.pyoracle.extract_batch, the counters with the host model (the oracle's alignment of the
first hit's window and of the union decides a re-queue).  Needs a real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

import sw_bound_cases as sb
from badger_amd import _native, synth

pytestmark = pytest.mark.gpu

UMI_LEN = 12
TAIL_CAP = 32
CLOSED = ("no", "single", "yes")
OPEN = ("open_yes", "open_tie", "open_merged", "open_n", "open_clipped")


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _run(ctx, orc, reads, n_open, per_read=1):
    """host: the batch is what it claims; device: the oracle's records and the model's counters"""
    bases, off = synth.list_to_reads(reads)
    m = sb.host_model(orc, reads, off)
    assert m["queue_b_clusters"] == 0 and (m["per_read"] == per_read).all() and m["clusters"] == per_read * len(reads)
    assert int(m["open"].sum()) == n_open, (int(m["open"].sum()), n_open)
    want = orc.extract_batch(bases, off, UMI_LEN, threads=4)
    got = ctx.extract_batch(bases, off, UMI_LEN)
    c = ctx.extract_counters()
    print("open", n_open, "of", m["clusters"], "re-queue among the open", int((m["open"] & m["requeue"]).sum()), "model requeued", m["requeued"], "counters", c)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "read %d (%s): got %s want %s (%d differ)" % (bad[0], reads[bad[0]], got[bad[0]], want[bad[0]], len(bad))
    assert c["clusters"] == m["clusters"] and c["filter_in"] == 0
    assert c["requeued"] == m["requeued"]
    assert c["alignments"] == m["clusters"] + m["requeued"] + c["filter_kept"]
    return m


def _kinds(n, open_at, seed):
    """n kinds: an open one at every index of open_at (all five in turn), closed ones elsewhere"""
    rng = np.random.default_rng(seed)
    kinds = [CLOSED[int(x)] for x in rng.integers(0, len(CLOSED), n)]
    for j, at in enumerate(sorted(open_at)):
        kinds[at] = OPEN[j % len(OPEN)]
    return kinds


@pytest.mark.parametrize("n_open", (0, 1, TAIL_CAP - 1, TAIL_CAP, TAIL_CAP + 1, 127, 128, 129, 512))
def test_open_clusters_in_one_block(ctx, orc, n_open):
    rng = np.random.default_rng(100 + n_open)
    open_at = rng.permutation(512)[:n_open].tolist()
    reads, _, _ = sb.kind_batch(orc, _kinds(512, open_at, n_open), 200 + n_open)
    m = _run(ctx, orc, reads, n_open)
    if n_open >= 127:                                                  # both answers of the tail, N, merged and clipped unions among them
        o = [c for c, is_open in zip(m["list"], m["open"]) if is_open]
        assert sum(c["merged"] for c in o) >= 10 and sum(c["end_clipped"] for c in o) >= 10 and sum("N" in c["window"][sb.HEAD_COLS:] for c in o) >= 10
        assert 10 <= int((m["open"] & m["requeue"]).sum()) <= n_open - 10


@pytest.mark.parametrize("open_reads", ((0,), (16,), (111,), (127,), (0, 16, 111, 127)))
def test_open_clusters_at_the_ends_of_wave_0(ctx, orc, open_reads):
    """read 0: lane 0, low half; 16: lane 0, high half; 111: lane 63, low half; 127: lane 63, high half - and the
    block's waves 1-3 have no entries at all"""
    for kind in ("open_yes", "open_tie"):
        kinds = _kinds(128, (), 7)
        for at in open_reads:
            kinds[at] = kind
        reads, _, _ = sb.kind_batch(orc, kinds, 300 + sum(open_reads))
        _run(ctx, orc, reads, len(open_reads))


def test_open_clusters_in_wave_3_only(ctx, orc):
    """one task, 64 entries of one shard: sixteen a wave, the open ones last.  (Every cluster lies in one vector: with 64
    and more vectors of hits in a task the scan may leave a pair unmerged, and the counts would no longer be exact.)"""
    per_read = [["yes", "single", "yes", "single"]] * 12 + [["open_yes", "open_tie", "open_yes", "open_tie"]] * 4
    _run(ctx, orc, sb.composite_reads(orc, per_read, 41), 16, per_read=4)


@pytest.mark.parametrize("share", (0.05, 1.0))
def test_a_last_block_with_one_wave(ctx, orc, share):
    """640 reads: block 0 is full, block 1 holds 128 entries in wave 0 and holes in waves 1-3"""
    rng = np.random.default_rng(55)
    n_open = int(640 * share)
    reads, _, _ = sb.kind_batch(orc, _kinds(640, rng.permutation(640)[:n_open].tolist(), 56), 57)
    _run(ctx, orc, reads, n_open)
