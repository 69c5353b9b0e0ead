"""The consensus alignment in a band of 128 and 256 diagonals (k_cons_align_wide in csrc/consensus_kernels.hip, chosen by
bdg_consensus_set_band) against the rule of badger_amd/consensus.py: bases, the number of voters and every field of every record,
bit for bit.  A path on every diagonal of the band (every register of every lane and every hand-over between lanes), lengths
around H and W, a drift that 64 diagonals lose and 128 hold, the band switched on one context, the limits, the setter's errors,
the device-array entry point over poisoned outputs, and --consensus_band on both command lines."""
import io
import logging
import re
from contextlib import contextmanager, redirect_stdout

import numpy as np
import pytest

import consensus_band_cases as bc
import consensus_cases as cc
from badger_amd import _native, badger, common, synth
from badger_amd import consensus as cs

pytestmark = pytest.mark.gpu

WIDE = (128, 256)
ANCHOR_IDS = {cs.ANCHOR_START: "start", cs.ANCHOR_END: "end"}


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@contextmanager
def banded(ctx, band):
    before = ctx.consensus_band
    ctx.consensus_set_band(band)
    try:
        yield
    finally:
        ctx.consensus_set_band(before)


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


def _host(ctx, groups, anchor, pct, band):
    """bdg_consensus in `band` -> the checker's form"""
    with banded(ctx, band):
        return _unpack(groups, *ctx.consensus(*_arrays(groups), anchor, pct))


def _dev(ctx, groups, anchor, pct, band):
    """bdg_consensus_dev over device arrays in `band`, the outputs poisoned first -> the checker's form"""
    bases, seq_off, grp_off = _arrays(groups)
    out_off = _native.consensus_out_offsets(seq_off, grp_off)
    n_seqs, n_groups = len(seq_off) - 1, len(grp_off) - 1
    host = [bases, seq_off, grp_off, out_off, np.full(max(int(out_off[-1]), 1), 0xAB, np.uint8), np.full(max(n_groups, 1), 0xABABABAB, np.uint32),
            np.full(max(n_groups, 1), 0xABABABAB, np.uint32), np.full(max(n_seqs, 1) * 3, 0xABABABAB, np.uint32)]
    d = [_native.DeviceArray.from_host(ctx, a) for a in host]
    try:
        with banded(ctx, band):
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


def _check(ctx, groups, anchor, pct, band, what, run=_host):
    want = cs.consensus_groups(groups, anchor, pct, band=band)
    _same(groups, run(ctx, groups, anchor, pct, band), want, what)
    return want


def _flags(want):
    return [w[2][1][2] for w in want]


# ---- every diagonal ----
def diagonal_groups(band):
    """band_pair(k) for k = -H - 1 .. H over 4 * W bases: at 40 % every k of the band is accepted with ed = |k| (|k| <= W / 2, the
    bound is 1.6 * W at least), the two outside have only paths full of mismatches (about half of 4 * W bases)"""
    H = band // 2
    return [list(bc.band_pair(k, 4 * band)) for k in range(-H - 1, H + 1)]


@pytest.fixture(scope="module", params=WIDE)
def diagonals(request):
    band, H = request.param, request.param // 2
    groups = diagonal_groups(band)
    want = cs.consensus_groups(groups, cs.ANCHOR_START, 40, band=band)
    # the plain form first, at the band's edges and one diagonal outside each
    for at in (0, 1, len(groups) - 2, len(groups) - 1):
        assert (want[at][0].decode(), want[at][1], want[at][2]) == bc.plain_consensus(groups[at], cs.ANCHOR_START, 40, band)
    assert _flags(want) == [cs.REJ_DIST] + [cs.ACCEPTED] * band + [cs.REJ_DIST]
    assert [w[2][1][0] for w in want[1:-1]] == [abs(k) for k in range(-H, H)]
    return band, groups, want


@pytest.mark.parametrize("anchor", (cs.ANCHOR_START, cs.ANCHOR_END), ids=ANCHOR_IDS.get)
def test_every_diagonal(ctx, diagonals, anchor):
    band, groups, want = diagonals
    if anchor == cs.ANCHOR_END:                                        # the same pairs mirrored: anchor-first they are the same strings
        groups = [[s[::-1] for s in g] for g in groups]
        mirrored = cs.consensus_groups(groups[:3] + groups[-3:], anchor, 40, band=band)
        want = [(c[::-1], v, r) for c, v, r in want]
        assert mirrored == want[:3] + want[-3:]
    got = _host(ctx, groups, anchor, 40, band)
    _same(groups, got, want, "every diagonal, band %d" % band)
    assert _flags(got) == [cs.REJ_DIST] + [cs.ACCEPTED] * band + [cs.REJ_DIST]


# ---- lengths ----
def size_grid(band):
    """backbone and member lengths independently around H and W: members cut from the backbone's text and mutated, plus one unrelated"""
    H = band // 2
    sizes = (0, 1, H - 1, H, H + 1, band - 1, band, band + 1, 2 * band + 1)
    rng = np.random.default_rng(12 + band)
    text = cc.rand_seq(rng, 2 * band + 80, 0.01)
    groups = []
    for lb in sizes:
        for lm in sizes:
            groups.append([text[:lb], cc.mutate(rng, text[:lm + 8])[:lm].ljust(lm, "A")])
    groups.append([text[:2 * band + 1], text[:2 * band - 1], cc.rand_seq(rng, band + 1), cc.mutate(rng, text[:2 * band + 1])])
    return groups


@pytest.mark.parametrize("band", WIDE)
@pytest.mark.parametrize("anchor", (cs.ANCHOR_START, cs.ANCHOR_END), ids=ANCHOR_IDS.get)
def test_lengths_around_the_band(ctx, anchor, band):
    groups = size_grid(band)
    for pct in (20, 100):
        want = _check(ctx, groups, anchor, pct, band, "sizes, band %d, pct %d" % (band, pct))
    flags = {r[2] for _, _, recs in want for r in recs[1:]}
    assert flags == {cs.ACCEPTED, cs.REJ_BAND}                      # (at 100 % only the band rejects)
    H = band // 2
    assert all((r[2] == cs.REJ_BAND) == (len(g[1]) > len(g[0]) + H) for g, (_, _, recs) in zip(groups[:-1], want) for r in recs[1:2])


# ---- drift: what the band of 64 loses ----
def test_a_drift_of_40_is_rejected_at_64_and_accepted_at_128(ctx):
    groups = [list(bc.band_pair(40, 300)), list(bc.band_pair(-40, 300))]
    at64 = _check(ctx, groups, cs.ANCHOR_START, 20, 64, "drift 40, band 64")
    at128 = _check(ctx, groups, cs.ANCHOR_START, 20, 128, "drift 40, band 128")
    assert _flags(at64) == [cs.REJ_DIST] * 2
    assert [w[2][1] for w in at128] == [(40, len(g[0]) - 10, cs.ACCEPTED) for g in groups]
    assert _flags(_check(ctx, groups, cs.ANCHOR_START, 20, 256, "drift 40, band 256")) == [cs.ACCEPTED] * 2
    mirrored = [[s[::-1] for s in g] for g in groups]
    assert _flags(_check(ctx, mirrored, cs.ANCHOR_END, 20, 128, "drift 40, band 128, anchor end")) == [cs.ACCEPTED] * 2
    assert ctx.consensus_band == 64


# ---- switching the band on one context ----
def test_switching_the_band_on_one_context(ctx):
    rng = np.random.default_rng(33)
    large = []
    for _ in range(40):
        _, r = cc.molecule(rng, 1500, 4, cs.ANCHOR_END)
        large.append(cc.elected(r))
    small = cc.random_groups(44, 30) + [[s[::-1] for s in bc.band_pair(k, 300)] for k in (40, -40, 20)]
    fresh = _native.Context(0)
    try:
        want64 = _unpack(small, *fresh.consensus(*_arrays(small), cs.ANCHOR_END, 20))
    finally:
        fresh.close()
    _same(small, want64, cs.consensus_groups(small, cs.ANCHOR_END, 20), "a fresh context, band 64")
    _check(ctx, large, cs.ANCHOR_END, 20, 256, "the large call, band 256")
    _same(small, _host(ctx, small, cs.ANCHOR_END, 20, 64), want64, "band 64 behind 256")
    _check(ctx, small + large[:4], cs.ANCHOR_END, 20, 128, "band 128 behind 64")
    _same(small, _host(ctx, small, cs.ANCHOR_END, 20, 64), want64, "band 64 behind 128")
    assert _flags(want64[-3:]) == [cs.REJ_DIST, cs.REJ_DIST, cs.ACCEPTED]


# ---- limits ----
def test_length_limit(ctx):
    rng = np.random.default_rng(5)
    t = cc.rand_seq(rng, 8300)
    m = cc.mutate(rng, t[:8300], 0.02, 0.01, 0.01)
    groups = [[t[:8192], m[:8192]], [t[:8192], m[:8193]], [t[:8193], m[:8192]]]
    want = _check(ctx, groups, cs.ANCHOR_START, 20, 256, "8,192 / 8,193 bases, band 256")
    assert _flags(want) == [cs.ACCEPTED, cs.REJ_LEN, cs.REJ_LEN] and [w[1] for w in want] == [2, 1, 1]
    _check(ctx, [[s[::-1] for s in g] for g in groups[:2]], cs.ANCHOR_END, 20, 128, "8,192 / 8,193 bases, band 128, anchor end")


def test_more_groups_than_waves_in_flight(ctx):
    groups = cc.random_groups(17, 5000, anchor=cs.ANCHOR_END)
    assert sum(len(g) for g in groups) > 20000
    want = _check(ctx, groups, cs.ANCHOR_END, 20, 128, "5,000 groups, band 128")
    assert sum(1 for g, w in zip(groups, want) if w[0] != g[0].encode()) > 2500


@pytest.mark.parametrize("band", WIDE)
def test_group_sizes_and_device_arrays(ctx, band):
    rng = np.random.default_rng(21)
    groups = []
    for n in (1, 2, 16):
        _, r = cc.molecule(rng, 300, n, cs.ANCHOR_END)
        groups.append(cc.elected(r))
    want = _check(ctx, groups, cs.ANCHOR_END, 20, band, "groups of 1, 2, 16")
    assert want[0][1] == 1 and want[2][1] >= 14
    # once per width through bdg_consensus_dev, the outputs poisoned
    part = groups + size_grid(band)[::3] + [list(bc.band_pair(k, 300)) for k in (40, -40, band // 2 - 1, -band // 2)]
    for anchor in (cs.ANCHOR_START, cs.ANCHOR_END):
        _check(ctx, part, anchor, 40, band, "device arrays, band %d" % band, run=_dev)
    with banded(ctx, band):
        assert _unpack([], *ctx.consensus(*_arrays([]), cs.ANCHOR_END, 20)) == []


# ---- the setter ----
def test_setter_refuses_other_widths(ctx):
    groups = [list(bc.band_pair(40, 300))]
    ctx.consensus_set_band(128)
    try:
        for bad in (0, 32, 96, 512):
            assert ctx.lib.bdg_consensus_set_band(ctx.h, bad) == _native.E_ARG, bad
            assert "64, 128 or 256" in ctx.lib.bdg_last_error(ctx.h).decode()
            with pytest.raises(_native.BadgerHipError) as e:
                ctx.consensus_set_band(bad)
            assert e.value.code == _native.E_ARG and ctx.consensus_band == 128
        # the band is what it was: the drift of 40 is still accepted
        got = _unpack(groups, *ctx.consensus(*_arrays(groups), cs.ANCHOR_START, 20))
        assert got == cs.consensus_groups(groups, cs.ANCHOR_START, 20, band=128) and _flags(got) == [cs.ACCEPTED]
    finally:
        ctx.consensus_set_band(64)
    fresh = _native.Context(0)
    try:                                                               # a new context has band 64
        got = _unpack(groups, *fresh.consensus(*_arrays(groups), cs.ANCHOR_START, 20))
        assert fresh.consensus_band == 64 and _flags(got) == [cs.REJ_DIST]
    finally:
        fresh.close()
    assert _native.CONS_BAND_DEFAULT == 64 and _native.CONS_BAND_MAX == 256


# ---- the command lines ----
class _Messages(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _stage2(argv):
    """-> (what the run printed, its log messages)"""
    buf, seen = io.StringIO(), _Messages()
    log = logging.getLogger("BarcodeGraph")
    log.addHandler(seen)
    try:
        with redirect_stdout(buf):
            badger.main(argv)
    finally:
        log.removeHandler(seen)
    return buf.getvalue(), seen.lines


N_CELLS = 30
SUFFIXES = (".fa", "_output_file.tsv", "_molecules.tsv", "_cells.tsv")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """600 synthetic 3' reads; 16 of them get 1,500 .. 2,500 bases more cDNA and four copies with new errors in it, one of which
    lacks 40 bases a fifth of the way in from the polyA end: from there on it runs 40 diagonals off the others"""
    tmp = tmp_path_factory.mktemp("cons_band")
    wl = synth.make_whitelist(400)
    b, o, truth = synth.make_reads(600, wl, seed=5, umi_len=12, n_cells=N_CELLS, tso=True, with_truth=True)
    reads = synth.reads_to_list(b, o)
    rc = truth["revcomp"].numpy()
    rng = np.random.default_rng(8)
    long_ones = [i for i in range(len(reads)) if len(reads[i]) >= 420][:16]
    for i in long_ones:
        x, L = reads[i], int(rng.integers(1500, 2501))
        ins = cc.rand_seq(rng, L)
        cut = L // 5 if not rc[i] else L - L // 5 - 40               # (the barcode, and behind it the polyA end, is at the read's start unless reversed)
        head, tail = (x[:200], x[200:]) if not rc[i] else (x[:-200], x[-200:])
        reads[i] = head + ins + tail
        for k in range(4):
            mid = ins[:cut] + ins[cut + 40:] if k == 3 else ins
            reads.append(head + cc.mutate(rng, mid, 0.03, 0.002, 0.002) + tail)
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    fq = str(tmp / "reads.fastq")
    with open(fq, "w") as f:
        f.write("".join("@read_%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
    wl_path = str(tmp / "wl.txt")
    open(wl_path, "w").write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    args = ["-r", fq, "-d", "tenX_v3", "-l", wl_path, "-c", str(N_CELLS), "--umi_dedup"]
    out = {}
    for name, extra in (("plain", []), ("b64", ["--consensus_band", "64"]), ("b128", ["--consensus_band", "128"])):
        p = str(tmp / name)
        out[name] = (p, _stage2(args + ["-o", p, "--tagged_reads", p + ".fa", "--molecule_consensus", p + ".consensus.fa"] + extra))
    return dict(tmp=tmp, out=out)


def _cn(text):
    return [int(x) for x in re.findall(rb"\tCN:i:(\d+)", text)]


def test_command_line_band_128(run):
    p128, p64, plain = run["out"]["b128"][0], run["out"]["b64"][0], run["out"]["plain"][0]
    tagged = open(p128 + ".fa", "rb").read()
    got = open(p128 + ".consensus.fa", "rb").read()
    want, counts = cs.consensus_text(tagged, cs.ANCHOR_END, 3, 20, lambda g, a, p: cs.consensus_groups(g, a, p, band=128))
    assert got == want
    _, counts64 = cs.consensus_text(tagged, cs.ANCHOR_END, 3, 20, cs.consensus_groups)
    narrow = open(p64 + ".consensus.fa", "rb").read()
    differ = sum(1 for a, b in zip(_cn(got), _cn(narrow)) if a != b)
    print("molecules %d; members accepted at 128: %d, at 64: %d; CN differs in %d molecules" % (
        counts["molecules"], counts["accepted"], counts64["accepted"], differ))
    assert len(_cn(got)) == len(_cn(narrow)) == counts["molecules"] and differ >= 1
    assert counts["accepted"] > counts64["accepted"] and counts["rej_dist"] < counts64["rej_dist"]
    # 64 is the run without the option, byte for byte; nothing else moves with the band
    assert narrow == open(plain + ".consensus.fa", "rb").read()
    for suffix in SUFFIXES:
        assert open(p128 + suffix, "rb").read() == open(plain + suffix, "rb").read() == open(p64 + suffix, "rb").read(), suffix
    for name, band in (("b128", 128), ("b64", 64), ("plain", 64)):
        said = [m for m in run["out"][name][1][1] if "Consensus: " in m]
        assert len(said) == 1 and said[0].endswith("band of %d diagonals" % band), said
    line = "members: %d accepted, rejected %d by distance" % (counts["accepted"], counts["rej_dist"])
    assert any(line in m for m in run["out"]["b128"][1][1])


def test_stand_alone_module_band_128(run):
    p128, p64 = run["out"]["b128"][0], run["out"]["b64"][0]
    out = str(run["tmp"] / "alone.fa")
    cs.main(["-i", p128 + ".fa", "-o", out, "--consensus_band", "128"])
    assert open(out, "rb").read() == open(p128 + ".consensus.fa", "rb").read()
    cs.main(["-i", p128 + ".fa", "-o", out])
    assert open(out, "rb").read() == open(p64 + ".consensus.fa", "rb").read()
    cs.main(["-i", p128 + ".fa", "-o", out, "--consensus_band", "64"])
    assert open(out, "rb").read() == open(p64 + ".consensus.fa", "rb").read()
