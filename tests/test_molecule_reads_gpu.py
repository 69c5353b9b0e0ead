"""The molecule kernels (csrc/umi_kernels.hip) called directly: bdg_molecule_reps_dev on the inputs of tests/molecule_cases.py
against badger_amd/molecule_reads.py (every read's rep flag and read count), with and without the wave aggregation, around a wave,
with one molecule holding every read, with probes that wrap past the last slot, in shuffled order, with the workspace reused; its
argument checks; and k_cdna_len (bdg_extract_keep_cdna) through submit / collect in uneven chunks and with every chunk rerun,
against the lengths trim.py and chimera.py give.  Integers: every comparison is exact."""
import numpy as np
import pytest

import molecule_cases as mc
from badger_amd import _native, chimera, molecule_reads as mr, synth, trim

pytestmark = pytest.mark.gpu

POISON = 0xAB


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _device(ctx, case, aggregate=True):
    """bdg_molecule_reps_dev on the case, outputs poisoned first -> (rep, mol_reads)"""
    n = case.n
    d = [_native.DeviceArray.from_host(ctx, a) for a in (case.cells, case.rank, case.has, case.mol, case.length)]
    d_rep = _native.DeviceArray.from_host(ctx, np.full(max(n, 1), POISON, dtype=np.uint8))
    d_cnt = _native.DeviceArray.from_host(ctx, np.full(max(n, 1), POISON * 0x01010101, dtype=np.uint32))
    ctx.molecule_reps_set_aggregate(aggregate)
    try:
        ctx.molecule_reps_dev(d[1], d[2], d[3], d[4], n, d[0], len(case.cells), d_rep, d_cnt)
        return d_rep.to_host()[:n], d_cnt.to_host()[:n]
    finally:
        ctx.molecule_reps_set_aggregate(True)
        for a in d + [d_rep, d_cnt]:
            a.free()


def _same(case, got, want, what):
    for name, g, w in (("rep", got[0], want[0]), ("mol_reads", got[1], want[1])):
        bad = np.nonzero(g != w)[0]
        if len(bad):
            rows = ["read %d rank %d has %d molecule %08x length %d: got %d want %d"
                    % (i, case.rank[i], case.has[i], case.mol[i], case.length[i], g[i], w[i]) for i in bad[:6].tolist()]
            raise AssertionError("%s %s: %d of %d %s differ from the rule\n  %s" % (case.name, what, len(bad), case.n, name, "\n  ".join(rows)))


# ---- 1. every generator, both forms of the insert kernel ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.GENERATORS))
@pytest.mark.parametrize("aggregate", (True, False))
def test_device_equals_the_rule(ctx, aggregate, name):
    case = mc.case(name)
    _same(case, _device(ctx, case, aggregate), case.rule(), "aggregate %d" % aggregate)


def test_one_molecule_holds_every_read(ctx):
    case = mc.one_molecule(200000)
    want = case.rule()
    assert want[0].sum() == 1 and (want[1] == 200000).all()
    for aggregate in (True, False):
        got = _device(ctx, case, aggregate)
        _same(case, got, want, "aggregate %d" % aggregate)
    # the representative: the first of the thousands of reads with the longest cDNA
    assert int(np.flatnonzero(got[0])[0]) == int(np.flatnonzero(case.length == case.length.max())[0])


def test_nothing_to_do(ctx):
    empty = mc.Case("empty", [5], [], [], [], [])
    rep, cnt = _device(ctx, empty)
    assert len(rep) == 0 and len(cnt) == 0
    no_cells = mc.Case("no_cells", [], [7, 7], [1, 1], [12 << 28, 12 << 28], [4, 5])
    rep, cnt = _device(ctx, no_cells)
    assert rep.tolist() == [0, 0] and cnt.tolist() == [0, 0]


# ---- 2. table sizes and probes that wrap ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (511, 512, 513, 1023, 1024, 1025))
def test_table_size_boundaries(ctx, n):
    """all keys distinct: 512 and 1,024 reads fill half of their table, one read more doubles it"""
    case = mc.distinct_keys(n, seed=n)
    got = _device(ctx, case)
    _same(case, got, case.rule(), "n %d" % n)
    assert (got[1] == 1).all() and (got[0] == (case.length > 0)).all()


@pytest.mark.parametrize("n,P", ((512, 1024), (1024, 2048)))
def test_probe_wrap(ctx, n, P):
    """thirty sets of distinct keys that half fill the table: in some of them the occupied slots run from the last slot on to
    the first, so claims and lookups go round the end"""
    spanning = wrapping = 0
    for seed in range(30):
        case = mc.distinct_keys(n - seed % 3, seed=9000 + n + seed, n_cells=1 + seed % 4)
        used, wrapped = mc.occupied(case, P)
        assert used.sum() == case.n
        spanning += bool(used[P - 1] and used[0])
        wrapping += wrapped > 0
        _same(case, _device(ctx, case, bool(seed & 1)), case.rule(), "wrap seed %d" % seed)
    print("P %d: sets with the last and the first slot both taken: %d, with a key stored past the end: %d" % (P, spanning, wrapping))
    assert spanning >= 3 and wrapping >= 1


# ---- 3. order, reuse ------------------------------------------------------------------------------------------------------
def test_shuffled_order_gives_the_same_answers(ctx):
    """read counts follow the reads; so do the representatives where no two reads of a molecule share its longest length -
    and where they do, the earliest read of the new order wins (the rule on the shuffled case)"""
    case = mc.case("mixed_4097")
    base = _device(ctx, case)
    shuffled, perm = case.shuffled(31)
    got = _device(ctx, shuffled)
    _same(shuffled, got, shuffled.rule(), "shuffled")
    assert (got[1] == base[1][perm]).all()
    untied = mc.Case("untied", case.cells, case.rank, case.has, case.mol, np.where(case.length > 0, 1 + np.arange(case.n) * 2654435761 % 1000003, 0))     # (all different)
    base = _device(ctx, untied)
    _same(untied, base, untied.rule(), "untied")
    shuffled, perm = untied.shuffled(32)
    got = _device(ctx, shuffled)
    assert (got[0] == base[0][perm]).all() and (got[1] == base[1][perm]).all() and base[0].sum() > 500


def test_small_call_after_a_large_one(ctx):
    big, small = mc.one_molecule(150000, seed=8), mc.case("wave_ties")
    first = _device(ctx, big)
    _same(big, first, big.rule(), "large call")
    _same(small, _device(ctx, small), small.rule(), "small call in the large call's workspace")
    again = _device(ctx, big)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    # ... and behind a dedup call, which lays the same workspace out differently
    import umi_cases as uc
    u = uc.case("dense", 12)
    d = [_native.DeviceArray.from_host(ctx, a) for a in (u.cells, u.rank, u.has, u.umi)]
    d_mol, d_cnt = _native.DeviceArray(ctx, u.n, np.uint32), _native.DeviceArray(ctx, (len(u.cells), 4), np.uint32)
    ctx.umi_dedup_dev(d[1], d[2], d[3], u.n, d[0], len(u.cells), 12, 1, d_mol, d_cnt)
    mol = d_mol.to_host()
    for a in d + [d_mol, d_cnt]:
        a.free()
    length = (np.arange(u.n) % 7 * 30).astype(np.uint32)
    case = mc.Case("after_dedup", u.cells, u.rank, u.has, mol, length)
    _same(case, _device(ctx, case), case.rule(), "on the molecules of bdg_umi_dedup_dev")
    assert case.rule()[1].max() > 1


# ---- 4. rejections --------------------------------------------------------------------------------------------------------
def test_rejections_launch_nothing(ctx):
    case = mc.case("no_cdna")
    n = case.n
    d = [_native.DeviceArray.from_host(ctx, a) for a in (case.cells, case.rank, case.has, case.mol, case.length)]
    d_rep = _native.DeviceArray.from_host(ctx, np.full(n, POISON, dtype=np.uint8))
    d_cnt = _native.DeviceArray.from_host(ctx, np.full(n, POISON * 0x01010101, dtype=np.uint32))
    good = dict(d_rank=d[1], d_has=d[2], d_molecule=d[3], d_cdna_len=d[4], n=n, d_cells=d[0], n_cells=len(case.cells), d_rep=d_rep, d_mol_reads=d_cnt)
    for change in (dict(d_rank=0), dict(d_has=0), dict(d_molecule=0), dict(d_cdna_len=0), dict(d_rep=0), dict(d_mol_reads=0), dict(d_cells=0)):
        with pytest.raises(_native.BadgerHipError):
            ctx.molecule_reps_dev(**dict(good, **change))
        assert (d_rep.to_host() == POISON).all() and (d_cnt.to_host() == POISON * 0x01010101).all(), change
    ctx.molecule_reps_dev(**good)
    _same(case, (d_rep.to_host(), d_cnt.to_host()), case.rule(), "after the rejections")
    for a in d + [d_rep, d_cnt]:
        a.free()


# ---- 5. k_cdna_len --------------------------------------------------------------------------------------------------------
def _chunks(n):
    steps, a, k = (1, 377, 13, 900, 64, 599, 3, 250), 0, 0
    while a < n:
        b = min(n, a + steps[k % len(steps)])
        yield k, a, b
        a, k = b, k + 1


def _through_the_pipeline(ctx, bases, off, n, umi_len):
    """submit / collect in uneven chunks, three in flight -> the records"""
    recs, flying = [], []
    for k, a, b in _chunks(n):
        if len(flying) >= 3:
            slot, m, _ = flying.pop(0)
            recs.append(ctx.extract_collect(slot, m))
        o = np.ascontiguousarray(off[a:b + 1], dtype=np.uint64)       # (stays alive until the chunk is collected)
        ctx.extract_submit(k % _native.SLOTS, bases.ctypes.data, o.ctypes.data, b - a, umi_len)
        flying.append((k % _native.SLOTS, b - a, o))
    for slot, m, _ in flying:
        recs.append(ctx.extract_collect(slot, m))
    return np.concatenate(recs)


def _kept_cdna(ctx):
    ptr, n = ctx.kept_cdna()
    out = np.zeros(n, dtype=np.uint32)
    if n:
        ctx._check(ctx.lib.bdg_mem_to_host(ctx.h, out.ctypes.data, ptr, out.nbytes))
    return out


def test_kept_cdna_lengths_equal_the_rules():
    import chimera_cases as cc
    wl = synth.make_whitelist(2000)
    b, o = synth.make_reads(1500, wl, seed=91, tso=True)
    reads = synth.reads_to_list(b, o)
    for k in range(150):                                              # chimeras: pairs joined head to tail and head to head
        x, y = reads[2 * k], reads[2 * k + 1]
        reads.append(x + (y if k & 1 else trim.revcomp(y)) if k & 2 else (trim.revcomp(y) if k & 1 else y) + x)
    reads += cc.case_set()["reads"][::2][:300]
    n = len(reads)
    bases, off = synth.list_to_reads(reads)
    E = 4
    ctx = _native.Context(0)
    try:
        want_recs = ctx.extract_batch(bases, off, 12)
        tr = trim.trim_batch(bases, off, want_recs, 20)
        ch = chimera.chimera_batch(bases, off, want_recs, tr, E)
        want_cut, want_plain = mr.cdna_len(tr, ch), mr.cdna_len(tr)
        hit = (ch["flags"] & chimera.CHIMERA_HIT) != 0
        assert (want_plain > 0).sum() > 1200 and (want_plain == 0).sum() > 20 and hit.sum() > 60
        assert (want_cut < want_plain).sum() > 60
        with pytest.raises(_native.BadgerHipError):
            ctx.extract_keep_cdna(True)                              # the trim is off
        assert ctx.kept_cdna()[1] == 0

        def run(chimera_on, queue=0):
            ctx.extract_keep_records(True)                           # (empty arrays again)
            ctx.extract_set_trim(True, 20)
            if chimera_on:
                ctx.extract_set_chimera(True, E)
            ctx.extract_keep_cdna(True)
            ctx.extract_set_queue_capacity(queue)
            try:
                recs = _through_the_pipeline(ctx, bases, off, n, 12)
            finally:
                ctx.extract_set_queue_capacity(0)
            assert (recs == want_recs).all() and not (recs["flags"] & _native.FLAG_INCOMPLETE).any()
            got = _kept_cdna(ctx)
            ctx.extract_set_trim(False)                              # (the chimera search and the keeping go off with it)
            assert len(got) == n and ctx.kept_records()[1] == n
            return got

        for chimera_on, want in ((True, want_cut), (False, want_plain)):
            for queue in (0, 16):                                    # 16: every chunk overflows and is rerun by collect
                got = run(chimera_on, queue)
                bad = np.nonzero(got != want)[0]
                assert not len(bad), (chimera_on, queue, len(bad), [(i, int(got[i]), int(want[i])) for i in bad[:5].tolist()])
        # the trim went off: nothing more is kept, and a chunk submitted without it does not fail
        o = np.ascontiguousarray(off[:101], dtype=np.uint64)
        ctx.extract_submit(0, bases.ctypes.data, o.ctypes.data, 100, 12)
        ctx.extract_collect(0, 100)
        assert ctx.kept_cdna()[1] == n and ctx.kept_records()[1] == n + 100
        ctx.extract_keep_records(False)                              # frees
        assert ctx.kept_cdna() == (0, 0)
    finally:
        ctx.close()
