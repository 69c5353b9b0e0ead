"""The chimera split on the GPU: bdg_split_batch and the device form against badger_amd/chimera_split.py, bit for bit - off' and
every piece record."""
import numpy as np
import pytest

import chimera_cases as cc
import split_cases as sc
from badger_amd import _native, chimera, chimera_split as cs, synth
from badger_amd.trim import revcomp

pytestmark = pytest.mark.gpu

E = cs.MAX_ED_DEFAULT
EDS = list(range(cs.MAX_ED_RANGE[1] + 1))


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


def _against_rule(ctx, reads, eds, what, segment=None):
    bases, off = synth.list_to_reads(reads)
    wants = cs.split_batch_multi(bases, off, eds, segment)
    for e, want in zip(eds, wants):
        got = ctx.split_batch(bases, off, e)
        _same(got, want, (what, e))
        again = ctx.split_batch(bases, off, e)
        assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()
    return wants


_SETS = {}


def _noisy(rng, s, p=0.07):
    """s with about p errors per base: substitutions, insertions and deletions alike"""
    out = []
    for ch, u in zip(s, rng.random(len(s))):
        if u < p / 3:
            continue
        out.append("ACGT"[int(rng.integers(0, 4))] if u < 2 * p / 3 else ch)
        if u > 1 - p / 3:
            out.append("ACGT"[int(rng.integers(0, 4))])
    return "".join(out)


def _random_set():
    """200 reads of 150 .. 1,500 bases with 0 .. 5 junctions and sequencing errors (more reads than a wave owns) and one clean
    concatemer of 6 molecules; the rule's answer at every max_ed, computed once"""
    if "random" not in _SETS:
        rng = np.random.default_rng(21)
        reads = []
        while len(reads) < 200:
            s = _noisy(rng, sc.concatemer(rng, int(rng.integers(1, 7)), junk=(0, 41))[0])
            if 150 <= len(s) <= 1500:
                reads.append(s)
            elif len(s) > 1500 and len(reads) % 3 == 0:
                reads.append(s[:1500])
        reads.append(sc.concatemer(rng, 6)[0])
        bases, off = synth.list_to_reads(reads)
        _SETS["random"] = dict(reads=reads, bases=bases, off=off, want=dict(zip(EDS, cs.split_batch_multi(bases, off, EDS))))
    return _SETS["random"]


def test_hand_derived_cases(ctx):
    by_ed = {}
    for label, read, e, bounds in sc.cases():
        by_ed.setdefault(e, []).append((read, bounds))
    for e, group in sorted(by_ed.items()):
        reads = [g[0] for g in group]
        bases, off = synth.list_to_reads(reads)
        off_out, rows = ctx.split_batch(bases, off, e)
        _same((off_out, rows), cs.split_batch(bases, off, e), ("cases", e))
        for i, (read, bounds) in enumerate(group):                      # (and, directly, what was derived by hand)
            mine = rows[(rows["read"] == i) & (rows["flags"] != 0)]
            assert [(int(r["start"]), int(r["ed"]), int(r["kind"])) for r in mine] == bounds, (e, i)


def test_short_and_empty_reads(ctx):
    rng = np.random.default_rng(3)
    for n in (0, 1, 127, 128, 129):
        s = (cc.clean(rng, 64) + chimera.R1 + cc.clean(rng, 64))[:n] if n < 128 else cc.clean(rng, 64) + chimera.R1 + cc.clean(rng, n - 64 - 22)
        off_out, rows = ctx.split_batch(*synth.list_to_reads([s]), 0)
        assert rows["start"].tolist() == ([0] if n < 128 else [0, 64]) and off_out.tolist() == ([0, n] if n < 128 else [0, 64, n]), n
    off_out, rows = ctx.split_batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert len(rows) == 0 and off_out.tolist() == [0]
    a, _ = sc.concatemer(rng, 2)
    b, _ = sc.concatemer(rng, 3)
    wants = _against_rule(ctx, [a, "", b, "", ""], [E], "an empty read between two others")
    assert len(wants[0][1]) == 8 and wants[0][1]["read"].tolist() == [0, 0, 1, 2, 2, 2, 3, 4]


def test_marks_on_either_side_of_a_segment_border(ctx):
    """a start mark (found by the backward scan) and an end mark (the forward scan) at every column of 250 .. 262 and 506 .. 518:
    either side of a border between segments and of where the next segment's automaton starts cold"""
    rng = np.random.default_rng(4)
    reads = []
    for pos in list(range(250, 263)) + list(range(506, 519)):
        reads.append(cc.clean(rng, pos) + cc.mutate(rng, chimera.R1, 1, "sub") + cc.clean(rng, 700 - pos))
        reads.append(cc.clean(rng, pos - 22) + cc.mutate(rng, chimera.PATTERNS[3], 1, "sub") + cc.clean(rng, 700 - pos))
        reads.append(cc.clean(rng, pos) + chimera.PATTERNS[1] + cc.clean(rng, 700 - pos))
        reads.append(cc.clean(rng, pos - 30) + chimera.TSO + cc.clean(rng, 700 - pos) + chimera.R1 + cc.clean(rng, 90))   # (a length no multiple of 4)
    wants = _against_rule(ctx, reads, [1, 6], "segment borders")
    starts = wants[0][1]["start"][wants[0][1]["flags"] != 0].tolist()
    assert len(starts) >= len(reads) and set(range(250, 263)) | set(range(506, 519)) <= set(starts)


def test_every_byte_alignment_of_a_unit(ctx):
    """the walk over a unit's words masks other bytes at every address mod 4 of the unit's first byte: the reads of the test
    above behind one more read of 0 .. 3 bases (shorter than 2 * MARGIN: no hit, one piece), against the one-read rule"""
    rng = np.random.default_rng(4)
    reads, marks = [], []                                               # marks: the (D, pos, kind) planted in each read
    for pos in list(range(250, 263)) + list(range(506, 519)):
        reads.append(cc.clean(rng, pos) + cc.mutate(rng, chimera.R1, 1, "sub") + cc.clean(rng, 700 - pos))
        reads.append(cc.clean(rng, pos - 22) + cc.mutate(rng, chimera.PATTERNS[3], 1, "sub") + cc.clean(rng, 700 - pos))
        reads.append(cc.clean(rng, pos) + chimera.PATTERNS[1] + cc.clean(rng, 700 - pos))
        reads.append(cc.clean(rng, pos - 30) + chimera.TSO + cc.clean(rng, 700 - pos) + chimera.R1 + cc.clean(rng, 90))
        marks += [[(1, pos, 2)], [(1, pos, 3)], [(0, pos, 1)], [(0, pos, 0), (0, 700, 2)]]
    for s, planted in zip(reads, marks):
        assert set(planted) <= set(cs.read_hits(s, 1)), planted
    for e in (1, 6):
        off0, rows0 = cs.split_reads(reads, e)
        assert len(rows0) >= 2 * len(reads)
        for shift in range(4):
            rows = np.concatenate([np.zeros(1, cs.SPLIT_DTYPE), rows0])
            rows["read"][1:] += 1
            want = np.concatenate([np.zeros(1, np.uint64), off0 + np.uint64(shift)]), rows
            _same(ctx.split_batch(*synth.list_to_reads(["ACG"[:shift]] + reads), e), want, ("shift", shift, e))


@pytest.mark.parametrize("max_ed", EDS)
def test_random_reads_equal_the_rule(ctx, max_ed):
    R = _random_set()
    got = ctx.split_batch(R["bases"], R["off"], max_ed)
    _same(got, R["want"][max_ed], max_ed)
    again = ctx.split_batch(R["bases"], R["off"], max_ed)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()
    if max_ed == E:
        per_read = np.bincount(got[1]["read"])
        assert per_read[-1] == 6 and (per_read == 1).sum() > 10 and len(got[1]) > 500
        assert set(got[1]["kind"][got[1]["flags"] != 0].tolist()) == {0, 1, 2, 3}


def test_reads_of_the_error_model_and_a_long_read(ctx):
    """3,000 reads of synth (a wave's 64 reads are more than a round of 32 segments), pairs of them, and one read of 40,000 bases
    with a junction every 1,000: many rounds of one wave's ring"""
    wl = synth.make_whitelist(3000)
    b, o = synth.make_reads(3000, wl, seed=12, tso=True)
    reads = synth.reads_to_list(b, o)
    reads += [reads[2 * k] + (revcomp(reads[2 * k + 1]) if k & 1 else reads[2 * k + 1]) for k in range(100)]
    rng = np.random.default_rng(9)
    reads.append("".join(cc.clean(rng, 1000 - 22) + chimera.R1 for _ in range(40)) + cc.clean(rng, 300))
    wants = _against_rule(ctx, reads, [E], "error model", cs.SEGMENT)    # (tests/test_chimera_split.py holds the segment form to the whole scan)
    per_read = np.bincount(wants[0][1]["read"])
    assert per_read[-1] == 41 and (per_read[3000:3100] >= 2).sum() >= 95 and (per_read[:3000] > 1).sum() <= 6


def test_device_form_cap_and_reuse(ctx):
    import torch
    R = _random_set()
    dev = torch.device("cuda", 0)
    n, total = len(R["reads"]), int(R["off"][-1])
    want_off, want_rows = R["want"][E]
    n_out = len(want_rows)
    lead = 3                                                            # (bases that do not start the buffer: off[0] != 0)
    d_bases = torch.zeros(lead + total + 64, dtype=torch.uint8, device=dev)
    d_bases[lead:lead + total] = torch.from_numpy(R["bases"]).to(dev)
    d_off = torch.from_numpy((R["off"] + np.uint64(lead)).astype(np.int64)).to(dev)
    ctx.set_stream(0)

    def run(cap, max_ed=E):
        d_off_out = torch.full(((cap + 1) * 8,), 0xAB, dtype=torch.uint8, device=dev)
        d_rows = torch.full((cap * 12 + 4,), 0xAB, dtype=torch.uint8, device=dev)
        d_count = torch.full((8,), 0xAB, dtype=torch.uint8, device=dev)
        ctx.split_batch_dev(d_bases, d_off, n, max_ed, d_off_out, d_rows, cap, d_count)
        torch.cuda.synchronize()
        return d_off_out.cpu().numpy(), d_rows.cpu().numpy(), int(d_count.cpu().numpy().view(np.uint64)[0])

    for cap in (n_out, n_out + 50):                                     # exactly enough, more than enough: the rest stays poisoned
        o, r, count = run(cap)
        assert count == n_out
        assert (o[:(n_out + 1) * 8].view(np.uint64) == want_off + np.uint64(lead)).all() and (o[(n_out + 1) * 8:] == 0xAB).all()
        assert r[:n_out * 12].tobytes() == want_rows.tobytes() and (r[n_out * 12:] == 0xAB).all()
    for cap in (n_out - 1, n):                                          # too small: the count, nothing else
        o, r, count = run(cap)
        assert count == n_out and (o == 0xAB).all() and (r == 0xAB).all()
    with pytest.raises(_native.BadgerHipError) as err:
        ctx.split_batch(R["bases"], R["off"], E, cap=n_out - 1)
    assert err.value.code == _native.E_CAPACITY and err.value.n_pieces == n_out
    # a smaller call on the same context behind the larger ones
    few = R["reads"][5:9]
    _same(ctx.split_batch(*synth.list_to_reads(few), E), cs.split_batch(*synth.list_to_reads(few), E), "a second, smaller call")
    _same(ctx.split_batch(R["bases"], R["off"], 6), R["want"][6], "and the larger one again")
    ctx.set_stream(0)


def test_argument_errors(ctx):
    import ctypes as C
    R = _random_set()
    bases, off = R["bases"], R["off"]
    n = len(off) - 1
    L = ctx.lib
    off_out, rows, count = np.zeros(4 * n + 1, np.uint64), np.zeros(4 * n, _native.SPLIT_DTYPE), C.c_uint64(7)
    args = lambda: [ctx.h, bases.ctypes.data, off.ctypes.data, n, E, off_out.ctypes.data, rows.ctypes.data, 4 * n, C.byref(count)]   # noqa: E731
    assert L.bdg_split_batch(*args()) == 0 and count.value == len(R["want"][E][1])
    for at, bad in ((0, None), (1, None), (2, None), (4, 7), (5, None), (6, None), (7, n - 1), (8, None)):
        a = args()
        a[at] = bad
        assert L.bdg_split_batch(*a) == _native.E_ARG, at
    d = _native.DeviceArray(ctx, 64, np.uint8)
    dargs = lambda: [ctx.h, d.ptr, d.ptr, 1, E, d.ptr, d.ptr, 1, d.ptr]   # noqa: E731
    for at, bad in ((0, None), (1, None), (2, None), (2, d.ptr + 4), (4, 7), (5, None), (5, d.ptr + 4), (6, None), (6, d.ptr + 2), (7, 0), (8, None),
                    (8, d.ptr + 4)):
        a = dargs()
        a[at] = bad
        assert L.bdg_split_batch_dev(*a) == _native.E_ARG, at
    with pytest.raises(_native.BadgerHipError):
        ctx.split_batch(bases, off, 7)
    # the 5' layout: an error with a message, whatever the arguments
    ctx.extract_set_layout(_native.LAYOUT_5P)
    try:
        with pytest.raises(_native.BadgerHipError, match="3'"):
            ctx.split_batch(bases, off, E)
        assert L.bdg_split_batch_dev(*dargs()) == _native.E_ARG
    finally:
        ctx.extract_set_layout(_native.LAYOUT_3P)
    assert len(ctx.split_batch(bases, off, E)[1]) == len(R["want"][E][1])
