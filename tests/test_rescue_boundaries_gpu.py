"""k_rescue_windows and k_rescue_resolve on the boundary cases of tests/rescue_boundary_cases.py: every family through
bdg_rescue_batch at each of its settings, every field of every record (umi as its 16 raw bytes) and the store's counts against
badger_amd/rescue.py; the device form over a poisoned output (two calls: W1 at U = 14, W1 at U = 12 with R2); the pipelined form
in uneven chunks, one store per U 1 .. 14 over all of W1, W2, W4 and R1, against the one-call form and the rule; both forms
twice on one context.

The `w >= nw` padding of k_rescue_resolve is not reached: the top-k match pads no slot that n_within counts, and the kernels
have no entry point of their own."""
import numpy as np
import pytest

import rescue_boundary_cases as bc
from badger_amd import _native, rescue, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx_of():
    """one context per whitelist, closed at the end"""
    made = {}

    def get(wl):
        key = wl.tobytes()
        if key not in made:
            made[key] = _native.Context(0)
            made[key].whitelist_load(wl)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def _raw(recs):
    return np.ascontiguousarray(recs).view(np.uint8).reshape(-1, _native.RESCUE_DTYPE.itemsize)


def _same(got, want, what, names):
    """every field, umi as raw bytes; the first difference by the case's name"""
    assert got.dtype == want.dtype == _native.RESCUE_DTYPE
    assert got["read"].tolist() == want["read"].tolist(), (what, [names[i] for i in sorted(set(got["read"].tolist()) ^ set(want["read"].tolist()))][:3])
    for f in rescue.FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert not len(bad), (what, names[int(want["read"][bad[0]])], f, got[bad[:3]].tolist(), want[bad[:3]].tolist())
    bad = np.nonzero((_raw(got) != _raw(want)).any(axis=1))[0]
    assert not len(bad), (what, names[int(want["read"][bad[0]])], "raw bytes", _raw(got)[bad[0]].tolist(), _raw(want)[bad[0]].tolist())


def _run(fam, ctx_of):
    n = 0
    for B in bc.family(fam):
        ctx = ctx_of(B.whitelist)
        bases, off = synth.list_to_reads(B.reads)
        elig = sum(1 for r in B.records if rescue.eligible(r))
        for s, want in bc.expected(B).items():
            got = ctx.rescue_batch(bases, off, B.records, B.U, B.support, s[0], s[1])
            _same(got, want, "%s max_ed %d min_support %d" % (B.name, s[0], s[1]), B.names)
            assert ctx.rescue_counts() == (len(want), elig), (B.name, s)
            n += len(want)
    assert n > 0


@pytest.mark.parametrize("fam", list(bc.FAMILIES))
def test_family_equals_the_rule(fam, ctx_of):
    _run(fam, ctx_of)


def _w1_r2():
    """W1 + R2 for the device form.  One call takes one U and one support array, so the batch is cut in two calls: all of W1 at
    U = 14 (the last record by `read` may be any, but the 16-letter UMI without a terminator is among the m records in front
    of the poison), and W1 at U = 12 with R2 under its first support array (every neighbour supported: rescued, ambiguous
    and truncated records in one output) -> [(U, reads, names, support)]"""
    W = {B.U: B for B in bc.family("W1")}
    R = bc.family("R2")[0]
    assert (W[12].support == R.support).all() and R.U == 12
    return [(14, W[14].reads, W[14].names, W[14].support), (12, W[12].reads + R.reads, W[12].names + R.names, R.support)]


def test_rescue_batch_dev_writes_m_records_and_nothing_behind_them(ctx_of):
    import torch
    dev = torch.device("cuda", 0)
    ctx = ctx_of(bc._Main.wl)
    ctx.set_stream(0)
    statuses, full = set(), 0
    for U, reads, names, support in _w1_r2():
        n = len(reads)
        bases, off = synth.list_to_reads(reads)
        recs = bc.records(n)
        want = rescue.rescue_batch(bases, off, recs, U, bc._Main.wl, support, 1, bc.M, matcher=bc.matcher(bc._Main.wl))
        assert 0 < len(want) <= n
        statuses |= {int(x) for x in want["status"]}
        full += sum(1 for x in want if len(bytes(x["umi"])) == 16)
        d_bases = torch.from_numpy(bases).to(dev)
        d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
        d_recs = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
        d_sup = torch.from_numpy(support.view(np.int32).copy()).to(dev)
        d_out = torch.full(((n + 8) * 40,), 0xAB, dtype=torch.uint8, device=dev)       # (room for n, and poison behind even then)
        m = ctx.rescue_batch_dev(d_bases, d_off, n, d_recs, U, d_sup, 1, bc.M, d_out)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert m == len(want) and ctx.rescue_counts() == (m, n)
        got = out[:m * 40].view(_native.RESCUE_DTYPE)
        _same(got[np.argsort(got["read"])], want, "rescue_batch_dev U %d" % U, names)
        assert (out[m * 40:] == 0xAB).all(), U
    assert statuses == {1, 2, 3} and full == 2


def test_pipelined_form_equals_the_one_call_form_and_the_rule(ctx_of):
    """every read of W1, W2, W4 and R1 through submit / collect / resolve, one store per UMI length (U 1 .. 14), on one context"""
    from test_rescue_gpu import _pipeline
    groups = bc.pipelined_set()
    assert sorted(groups) == list(range(1, 15))
    ctx = ctx_of(bc._Main.wl)
    d_sup = _native.DeviceArray.from_host(ctx, bc._Main.support)
    m = bc.matcher(bc._Main.wl)
    settings = ((1, bc.M), (2, 1))
    total = lost_total = stored = 0
    for U, (reads, names, r1) in groups.items():
        n = len(reads)
        bases, off = synth.list_to_reads(reads)
        runs = []
        for _ in range(2):                                                 # twice on one context: the same bytes
            ctx.extract_set_rescue(True)
            recs = _pipeline(ctx, bases, off, n, (1, 63, 64, 65, 257), U)
            got = {s: ctx.extract_rescue_resolve(d_sup, s[0], s[1]).copy() for s in settings}
            counts = ctx.rescue_counts()
            ctx.extract_set_rescue(False)
            runs.append((recs, got, counts))
        recs, got, counts = runs[0]
        assert (runs[1][0] == recs).all() and runs[1][2] == counts, U
        # the real extraction finds no adapter in these reads: they stay eligible (none of R1 may not)
        elig = np.array([rescue.eligible(r) for r in recs])
        assert elig[r1].all(), (U, [names[i] for i in np.nonzero(~elig & r1)[0]][:5])
        total, lost_total = total + n, lost_total + int((~elig).sum())
        for s in settings:
            want = rescue.rescue_batch(bases, off, recs, U, bc._Main.wl, bc._Main.support, s[0], s[1], matcher=m)
            _same(got[s], want, "pipelined U %d %r" % (U, s), names)
            assert _raw(runs[1][1][s]).tobytes() == _raw(got[s]).tobytes(), (U, s)
            one = ctx.rescue_batch(bases, off, recs, U, bc._Main.support, s[0], s[1])
            _same(one, want, "one call U %d %r" % (U, s), names)
            assert _raw(ctx.rescue_batch(bases, off, recs, U, bc._Main.support, s[0], s[1])).tobytes() == _raw(one).tobytes(), (U, s)
        assert counts == (len(got[settings[0]]), int(elig.sum())), U
        stored += counts[0]
    d_sup.free()
    print("pipelined: %d reads, %d not eligible, %d stored" % (total, lost_total, stored))
    assert total == 140 + 90 + 16 + 5 * 255 and lost_total <= 0.02 * total and stored > 0.9 * total
