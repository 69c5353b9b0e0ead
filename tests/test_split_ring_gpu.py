"""k_split_scan's cell ring and k_split_emit's stride loop on the GPU: every case wave of tests/split_ring_cases.py through
bdg_split_batch and the device form against badger_amd/chimera_split.py at the kernel's segment, bit for bit - off' and every
piece record - and against the boundaries the cases name by hand."""
import numpy as np
import pytest

import split_ring_cases as rc
from badger_amd import _native, chimera_split as cs, synth

pytestmark = pytest.mark.gpu

STRIDE = 2048 * 256                                                     # k_split_emit's grid at its cap: threads of one trip


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _same(got, want, what):
    assert len(got[0]) == len(want[0]) and (got[0] == want[0]).all(), (what, "off'")
    assert got[1].dtype == _native.SPLIT_DTYPE == cs.SPLIT_DTYPE
    bad = np.nonzero(got[1] != want[1])[0]
    assert not len(bad), (what, bad[:5].tolist(), got[1][bad[:5]].tolist(), want[1][bad[:5]].tolist())


def _cuts(rows):
    r = rows[rows["flags"] != 0]
    return list(zip(r["read"].tolist(), r["start"].tolist(), r["ed"].tolist(), r["kind"].tolist()))


_SETS = {}


def _batch(max_ed, order):
    """the case waves of one max_ed in one batch, a wave per block (the short wave last, in either order); the rule's answer,
    computed once, and the boundaries named by hand as (read, pos, D, kind)"""
    if (max_ed, order) not in _SETS:
        waves = [w for w in rc.waves() if w["max_ed"] == max_ed]
        full = [w for w in waves if len(w["reads"]) == rc.WAVE]
        full = full[::-1] if order == "reversed" else full
        waves = full + [w for w in waves if len(w["reads"]) < rc.WAVE]
        reads, hand = [], []
        for w in waves:
            hand += [(len(reads) + r, p, d, k) for r in sorted(w["bounds"]) for p, d, k in w["bounds"][r]]
            reads += w["reads"]
        bases, off = synth.list_to_reads(reads)
        _SETS[max_ed, order] = dict(n=len(reads), blocks=len(waves), bases=bases, off=off, hand=hand,
                                    want=cs.split_batch(bases, off, max_ed, segment=cs.SEGMENT))
    return _SETS[max_ed, order]


@pytest.mark.parametrize("order", ["as_listed", "reversed"])
def test_every_case_wave_in_one_call(ctx, order):
    """many blocks in one call, and again with the waves the other way round: no case depends on its block index"""
    for e in (1, 2):
        S = _batch(e, order)
        assert S["blocks"] >= 9 and _cuts(S["want"][1]) == S["hand"]     # (the rule's batch form names what the cases name)
        got = ctx.split_batch(S["bases"], S["off"], e)
        _same(got, S["want"], (order, e))
        assert _cuts(got[1]) == S["hand"]
        assert len(got[1]) == S["n"] + len(S["hand"])


def test_a_second_call_writes_the_same_bytes(ctx):
    S = _batch(1, "as_listed")
    one = ctx.split_batch(S["bases"], S["off"], 1)
    two = ctx.split_batch(S["bases"], S["off"], 1)
    assert one[0].tobytes() == two[0].tobytes() == S["want"][0].tobytes()
    assert one[1].tobytes() == two[1].tobytes() == S["want"][1].tobytes()


def test_device_form_over_poisoned_outputs(ctx):
    """cap exactly the piece count: every byte of off' and of the records is written, none behind them"""
    import torch
    S = _batch(1, "as_listed")
    dev = torch.device("cuda", 0)
    total = int(S["off"][-1])
    want_off, want_rows = S["want"]
    cap = len(want_rows)
    lead = 3                                                            # (bases that do not start the buffer: off[0] != 0)
    d_bases = torch.zeros(lead + total + 64, dtype=torch.uint8, device=dev)
    d_bases[lead:lead + total] = torch.from_numpy(S["bases"]).to(dev)
    d_off = torch.from_numpy((S["off"] + np.uint64(lead)).astype(np.int64)).to(dev)
    d_off_out = torch.full(((cap + 1) * 8 + 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_rows = torch.full((cap * 12 + 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_count = torch.full((8,), 0xAB, dtype=torch.uint8, device=dev)
    ctx.set_stream(0)
    ctx.split_batch_dev(d_bases, d_off, S["n"], 1, d_off_out, d_rows, cap, d_count)
    torch.cuda.synchronize()
    o, r, count = d_off_out.cpu().numpy(), d_rows.cpu().numpy(), int(d_count.cpu().numpy().view(np.uint64)[0])
    assert count == cap
    assert (o[:(cap + 1) * 8].view(np.uint64) == want_off + np.uint64(lead)).all() and (o[(cap + 1) * 8:] == 0xAB).all()
    assert r[:cap * 12].tobytes() == want_rows.tobytes() and (r[cap * 12:] == 0xAB).all()


def test_the_emit_grid_goes_round_its_stride_loop(ctx):
    """530,000 reads, more than the 524,288 threads of k_split_emit's capped grid: reads on both sides of the wrap (index 0,
    524,287, 524,288, the last) and 600 and more staged boundaries, which all lie behind it - several blocks reach them on their
    second trip.  All reads but 314 are empty; bases and off are built as arrays."""
    n = 530000
    assert n > STRIDE
    rank = next(w for w in rc.waves() if w["label"] == ("rank", 256, 0))
    long_read, long_bounds = next((rank["reads"][r], b) for r, b in rank["bounds"].items())
    two = rc.marked_read(768, [(5, 1), (8, 0)], 1)                      # 3 cells apart: both
    two_bounds = [(rc._pos(5), 1, 2), (rc._pos(8), 0, 2)]
    at = {i: (two, two_bounds) for i in range(1733, n, 1733)}
    at.update({i: (long_read, long_bounds) for i in (0, STRIDE, n - 1)})
    at.update({i: (rc.tail_read(768), [(768 - rc.MARGIN, 0, 2)]) for i in (STRIDE - 1, STRIDE + 1, n - 2)})
    lengths = np.zeros(n, np.int64)
    for i, (s, _) in at.items():
        lengths[i] = len(s)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lengths)
    bases = np.frombuffer("".join(at[i][0] for i in sorted(at)).encode("ascii"), dtype=np.uint8)
    hand = [(i, p, d, k) for i in sorted(at) for p, d, k in at[i][1]]
    assert len(hand) > 600 and len(bases) == int(off[-1])
    want = cs.split_batch(bases, off, 1, segment=cs.SEGMENT)
    assert _cuts(want[1]) == hand
    got = ctx.split_batch(bases, off, 1)
    _same(got, want, "stride")
    assert _cuts(got[1]) == hand and len(got[1]) == n + len(hand)
