"""The consensus kernels (csrc/consensus_kernels.hip) against the rule of badger_amd/consensus.py: bases, lengths, the number of
voters and every field of every record, bit for bit.  Around the wave's 64 lanes and the 256-position tiles of the call, at the
band's edges, at the acceptance boundary, at every tie rule, at the length limit, with more groups than waves in flight, with
the workspaces reused by smaller calls and behind another kernel family's call; the host-array entry point against the device
one; the argument errors."""
import numpy as np
import pytest

import consensus_cases as cc
import umi_cases as uc
from badger_amd import _native
from badger_amd import consensus as cs

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 31, 32, 33, 63, 64, 65, 127, 129)
ANCHOR_IDS = {cs.ANCHOR_START: "start", cs.ANCHOR_END: "end"}


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _arrays(groups):
    flat = [s.encode() if isinstance(s, str) else bytes(s) for g in groups for s in g]
    bases = np.frombuffer(b"".join(flat), dtype=np.uint8)
    seq_off = np.concatenate([[0], np.cumsum([len(s) for s in flat])]).astype(np.uint64)
    grp_off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.uint64)
    return bases, seq_off, grp_off


def _unpack(groups, out, out_off, out_len, voted, recs):
    res, at = [], 0
    for k, g in enumerate(groups):
        o = int(out_off[k])
        res.append((out[o:o + int(out_len[k])].tobytes(), int(voted[k]),
                    [(int(r["ed"]), int(r["span"]), int(r["flags"])) for r in recs[at:at + len(g)]]))
        at += len(g)
    return res


def _host(ctx, groups, anchor, pct):
    """bdg_consensus -> the checker's form"""
    return _unpack(groups, *ctx.consensus(*_arrays(groups), anchor, pct))


def _dev(ctx, groups, anchor, pct):
    """bdg_consensus_dev over device arrays, the outputs poisoned first -> the checker's form"""
    bases, seq_off, grp_off = _arrays(groups)
    out_off = _native.consensus_out_offsets(seq_off, grp_off)
    n_seqs, n_groups = len(seq_off) - 1, len(grp_off) - 1
    host = [bases, seq_off, grp_off, out_off, np.full(max(int(out_off[-1]), 1), 0xAB, np.uint8), np.full(max(n_groups, 1), 0xABABABAB, np.uint32),
            np.full(max(n_groups, 1), 0xABABABAB, np.uint32), np.full(max(n_seqs, 1) * 3, 0xABABABAB, np.uint32)]
    d = [_native.DeviceArray.from_host(ctx, a) for a in host]
    try:
        ctx.consensus_dev(d[0], d[1], n_seqs, d[2], n_groups, anchor, pct, d[3], d[4], d[5], d[6], d[7])
        return _unpack(groups, d[4].to_host(), out_off, d[5].to_host(), d[6].to_host(), d[7].to_host().view(_native.CONSENSUS_DTYPE))
    finally:
        for a in d:
            a.free()


def _same(groups, got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            raise AssertionError("%s: group %d %r\n  device  %r\n  checker %r" % (what, k, [s if len(s) < 80 else s[:77] + "..." for s in groups[k]], g, w))


def _check(ctx, groups, anchor, pct, what, run=_host):
    want = cs.consensus_groups(groups, anchor, pct)
    _same(groups, run(ctx, groups, anchor, pct), want, what)
    return want


def _size_grid():
    """backbone and member lengths independently over SIZES: members cut from the backbone's text and mutated, plus one unrelated"""
    rng = np.random.default_rng(12)
    text = cc.rand_seq(rng, 200, 0.01)
    groups = []
    for lb in SIZES:
        for lm in SIZES:
            groups.append([text[:lb], cc.mutate(rng, text[:lm + 8])[:lm].ljust(lm, "A")])
    groups.append([text[:129], text[:127], cc.rand_seq(rng, 65), cc.mutate(rng, text[:129])])
    return groups


@pytest.mark.parametrize("anchor", (cs.ANCHOR_START, cs.ANCHOR_END), ids=ANCHOR_IDS.get)
def test_lengths_around_the_lanes(ctx, anchor):
    groups = _size_grid()
    for pct in (20, 100):
        want = _check(ctx, groups, anchor, pct, "sizes, pct %d" % pct)
    flags = {r[2] for _, _, recs in want for r in recs[1:]}
    assert flags == {cs.ACCEPTED, cs.REJ_BAND}                      # (at 100 % only the band rejects; members longer than the backbone are in)
    assert sum(1 for g in groups if len(g[1]) > len(g[0])) >= 40


@pytest.mark.parametrize("anchor", (cs.ANCHOR_START, cs.ANCHOR_END), ids=ANCHOR_IDS.get)
def test_identical_all_n_and_tie_rules(ctx, anchor):
    s = cc.rand_seq(np.random.default_rng(3), 150)
    groups = [[s, s], [s, s, s], ["N" * 70, "N" * 70, "N" * 64], ["N" * 10], [s, "N" * 150], ["acgt" * 20, "ACGT" * 20]]
    groups += [c[1] for c in cc.TIES]
    for pct in (20, 40, 100):
        _check(ctx, groups, anchor, pct, "identical / N / ties, pct %d" % pct)
    # the tie cases at their own anchor and bound give their hand-derived answers on the device too
    for name, group, a, pct, want, voted, _ in cc.TIES:
        got = _host(ctx, [group], a, pct)[0]
        assert (got[0].decode(), got[1]) == (want, voted), name


def test_band_edges_and_acceptance_boundary(ctx):
    groups = [list(cc.band_pair(k)) for k in (31, 32, -32, -33)] + [["ACGT" * 5, "A" * 53], ["ACGT" * 5, "A" * 52]]
    want = _check(ctx, groups, cs.ANCHOR_START, 40, "band edges")
    assert [w[2][1][2] for w in want] == [cs.ACCEPTED, cs.REJ_DIST, cs.ACCEPTED, cs.REJ_DIST, cs.REJ_BAND, cs.REJ_DIST]
    _check(ctx, groups, cs.ANCHOR_END, 40, "band edges, mirrored")
    b, m = "ACGTTGCAAC" * 2, "ACGTTGCAAC" + "ACGTAGCAAC"              # ed 1, Lm 20: 1 * 100 == 5 * 20
    for pct, flag in ((5, cs.ACCEPTED), (4, cs.REJ_DIST), (0, cs.REJ_DIST), (100, cs.ACCEPTED)):
        want = _check(ctx, [[b, m], [b, b], [b, "T" * 20]], cs.ANCHOR_END, pct, "pct %d" % pct)
        assert want[0][2][1] == (1, 20, flag) and want[1][2][1] == (0, 20, cs.ACCEPTED)


@pytest.mark.parametrize("anchor", (cs.ANCHOR_START, cs.ANCHOR_END), ids=ANCHOR_IDS.get)
def test_group_sizes(ctx, anchor):
    rng = np.random.default_rng(21)
    groups = []
    for n in (1, 2, 3, 16):
        _, r = cc.molecule(rng, 300, n, anchor)
        groups.append(cc.elected(r))
    want = _check(ctx, groups, anchor, 20, "groups of 1, 2, 3, 16")
    assert [w[1] for w in want][0] == 1 and want[3][1] >= 14
    _, r = cc.molecule(rng, 60, 17, anchor)
    with pytest.raises(_native.BadgerHipError) as e:
        _host(ctx, [cc.elected(r)], anchor, 20)
    assert e.value.code == _native.E_ARG and "16" in str(e.value)


def test_length_limit(ctx):
    rng = np.random.default_rng(5)
    t = cc.rand_seq(rng, 9000)
    def low(x):                                                      # (few indels: over 8,000 bases the drift stays inside the band)
        return cc.mutate(rng, x, 0.02, 0.005, 0.005)
    m = low(t[:8500])
    groups = [[t[:8192], m[:8192]], [t[:8192], m[:8193]], [t[:8193], m[:8192]], [t[:8193], t[:8193]],
              [t, t[:5000], t[:100], cc.mutate(rng, t[:300])], [t[:8192], low(t[:8000]), low(t[:7000]), t[:40]]]
    want = _check(ctx, groups, cs.ANCHOR_START, 20, "length limit")
    assert [w[2][1][2] for w in want[:4]] == [cs.ACCEPTED, cs.REJ_LEN, cs.REJ_LEN, cs.REJ_LEN]
    assert want[4][0] == t.encode() and want[4][1] == 1 and want[2][0] == t[:8193].encode()
    assert want[5][1] == 4 and want[5][0] != groups[5][0].encode()
    _check(ctx, [[s[::-1] for s in g] for g in groups[1:2] + groups[4:]], cs.ANCHOR_END, 20, "length limit, anchor end")


@pytest.fixture(scope="module")
def many():
    groups = cc.random_groups(17, 5000, anchor=cs.ANCHOR_END)
    groups[100] = list(groups[7])                                    # two groups sharing identical sequences
    groups[101] = list(groups[7])
    return groups, cs.consensus_groups(groups, cs.ANCHOR_END, 20)


def test_more_groups_than_waves_then_small_calls(ctx, many):
    groups, want = many
    assert sum(len(g) for g in groups) > 20000
    _same(groups, _host(ctx, groups, cs.ANCHOR_END, 20), want, "5,000 groups")
    assert want[100] == want[7] == want[101]
    changed = sum(1 for g, w in zip(groups, want) if w[0] != g[0].encode())
    assert changed > 2500
    # a small call behind the large one: the counters, the trace and the staging buffers are reused
    _same(groups[:3], _host(ctx, groups[:3], cs.ANCHOR_END, 20), want[:3], "small call after the large one")
    _same(groups[40:41], _dev(ctx, groups[40:41], cs.ANCHOR_END, 20), want[40:41], "one group, device arrays")
    # ... and behind a call of the UMI kernels on the same context
    case = uc.case("dense", 12)
    d = [_native.DeviceArray.from_host(ctx, a) for a in (case.cells, case.rank, case.has, case.umi)]
    d_mol = _native.DeviceArray(ctx, max(case.n, 1), np.uint32)
    d_cnt = _native.DeviceArray(ctx, (max(len(case.cells), 1), 4), np.uint32)
    try:
        ctx.umi_dedup_dev(d[1], d[2], d[3], case.n, d[0], len(case.cells), 12, 1, d_mol, d_cnt)
        ctx.synchronize()
    finally:
        for a in d + [d_mol, d_cnt]:
            a.free()
    _same(groups[200:260], _host(ctx, groups[200:260], cs.ANCHOR_END, 20), want[200:260], "after bdg_umi_dedup_dev")
    # the same call twice gives the same bytes (the votes are sums: no order of the waves changes them)
    assert _host(ctx, groups[:500], cs.ANCHOR_END, 20) == _host(ctx, groups[:500], cs.ANCHOR_END, 20) == want[:500]


def test_device_arrays_against_host_arrays(ctx, many):
    groups, want = many
    part = groups[300:700] + _size_grid()
    for anchor in (cs.ANCHOR_START, cs.ANCHOR_END):
        dev = _dev(ctx, part, anchor, 20)
        assert dev == _host(ctx, part, anchor, 20)
        _same(part, dev, cs.consensus_groups(part, anchor, 20), "device arrays")
    assert _dev(ctx, [], cs.ANCHOR_END, 20) == [] and _host(ctx, [], cs.ANCHOR_END, 20) == []


def test_argument_errors(ctx):
    groups = cc.random_groups(2, 4)
    bases, seq_off, grp_off = _arrays(groups)
    lib, h = ctx.lib, ctx.h
    n_seqs, n_groups = len(seq_off) - 1, len(grp_off) - 1
    out_off = _native.consensus_out_offsets(seq_off, grp_off)
    out = np.zeros(int(out_off[-1]), np.uint8)
    ln, nv, recs = np.zeros(n_groups, np.uint32), np.zeros(n_groups, np.uint32), np.zeros(n_seqs, _native.CONSENSUS_DTYPE)

    def call(seq_off=seq_off, grp_off=grp_off, anchor=1, pct=20, out_off=out_off, n_seqs=n_seqs, n_groups=n_groups):
        return lib.bdg_consensus(h, bases.ctypes.data, seq_off.ctypes.data, n_seqs, grp_off.ctypes.data, n_groups, anchor, pct,
                                 out_off.ctypes.data, out.ctypes.data, ln.ctypes.data, nv.ctypes.data, recs.ctypes.data)

    def fails(word, **kw):
        assert call(**kw) == _native.E_ARG, word
        assert word in lib.bdg_last_error(h).decode(), (word, lib.bdg_last_error(h))

    fails("anchor", anchor=2)
    fails("anchor", anchor=-1)
    fails("max_ed_pct", pct=101)
    bad = seq_off.copy(); bad[3] = bad[2] - 1
    fails("non-decreasing", seq_off=bad)
    bad = grp_off.copy(); bad[2] = bad[1] - 1
    fails("non-decreasing", grp_off=bad)
    bad = grp_off.copy(); bad[2] = bad[1]
    fails("without a sequence", grp_off=bad)
    fails("more than 16", grp_off=np.array([0, 17], np.uint64), n_groups=1, n_seqs=17,
          seq_off=np.arange(18, dtype=np.uint64), out_off=np.array([0, 2], np.uint64))
    fails("cover", grp_off=np.array([0, n_seqs - 1], np.uint64), n_groups=1, out_off=np.array([0, 100000], np.uint64))
    bad = out_off.copy(); bad[1] -= 1
    fails("2 * Lb", out_off=bad)
    assert call() == 0                                                 # the context still works
    want = cs.consensus_groups(groups, cs.ANCHOR_END, 20)
    _same(groups, _unpack(groups, out, out_off, ln, nv, recs), want, "after the errors")
    # the device form checks the same things
    d = [_native.DeviceArray.from_host(ctx, a) for a in (bases, seq_off, grp_off, out_off, out, ln, nv, recs.view(np.uint32))]
    try:
        for anchor, pct in ((2, 20), (1, 101)):
            with pytest.raises(_native.BadgerHipError) as e:
                ctx.consensus_dev(d[0], d[1], n_seqs, d[2], n_groups, anchor, pct, d[3], d[4], d[5], d[6], d[7])
            assert e.value.code == _native.E_ARG
        short = _native.DeviceArray.from_host(ctx, np.zeros(n_groups + 1, np.uint64))
        with pytest.raises(_native.BadgerHipError) as e:
            ctx.consensus_dev(d[0], d[1], n_seqs, d[2], n_groups, 1, 20, short, d[4], d[5], d[6], d[7])
        assert e.value.code == _native.E_ARG and "2 * Lb" in str(e.value)
        short.free()
    finally:
        for a in d:
            a.free()
