"""The UMI kernels (csrc/umi_kernels.hip) called directly: bdg_umi_dedup_dev on the inputs of tests/umi_cases.py against
badger_amd/umi_dedup.py (every read's molecule, every cell's four counts), around the table's size boundaries, with probes
that wrap past the last slot, with the workspace reused, in shuffled order and on a second context; its argument checks;
and k_umi_pack (bdg_extract_keep_umis) against the UMI column bdg_format_rows prints, through submit / collect in uneven chunks
and with every chunk rerun.  Integers and text: every comparison is exact."""
import numpy as np
import pytest

import umi_cases as uc
from badger_amd import _native, synth
from badger_amd import umi_dedup as ud

pytestmark = pytest.mark.gpu

POISON = 0xAB


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _poisoned(ctx, shape):
    return _native.DeviceArray.from_host(ctx, np.full(shape, POISON * 0x01010101, dtype=np.uint32))


def _device(ctx, case, umi_len, dist):
    """bdg_umi_dedup_dev on the case, outputs poisoned first -> (molecule code per read, counts per cell)"""
    n, nc = case.n, len(case.cells)
    d = [_native.DeviceArray.from_host(ctx, a) for a in (case.cells, case.rank, case.has, case.umi)]
    d_mol, d_cnt = _poisoned(ctx, max(n, 1)), _poisoned(ctx, (max(nc, 1), 4))
    try:
        ctx.umi_dedup_dev(d[1], d[2], d[3], n, d[0], nc, umi_len, dist, d_mol, d_cnt)
        return d_mol.to_host()[:n], d_cnt.to_host()[:nc]
    finally:
        for a in d + [d_mol, d_cnt]:
            a.free()


def _text(code):
    return "*" if code == ud.NONE else ud.umi_str(int(code))


def _same(case, got, want, what):
    (gm, gc), (wm, wc) = got, want
    bad = np.nonzero(gm != wm)[0]
    if len(bad):
        rows = ["read %d cell %s UMI %r: got %s want %s" % (i, case.cell_text[i], case.umi_text[i], _text(gm[i]), _text(wm[i]))
                for i in bad[:6].tolist()]
        raise AssertionError("%s %s: %d of %d molecules differ from the rule\n  %s" % (case.name, what, len(bad), case.n, "\n  ".join(rows)))
    bad = np.nonzero((gc != wc).any(axis=1))[0]
    if len(bad):
        rows = ["cell %d (rank %d): got %s want %s" % (j, case.cells[j], gc[j].tolist(), wc[j].tolist()) for j in bad[:6].tolist()]
        raise AssertionError("%s %s: %d of %d cells differ from the rule\n  %s" % (case.name, what, len(bad), len(wc), "\n  ".join(rows)))


_RULE = {}


def _rule(case, umi_len, dist):
    key = (case.name, umi_len, dist)
    if key not in _RULE:
        _RULE[key] = uc.rule(case, umi_len, dist)
    return _RULE[key]


# ---- 1. every generator -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(uc.GENERATORS))
@pytest.mark.parametrize("umi_dist", (0, 1))
@pytest.mark.parametrize("umi_len", (3, 10, 12))
def test_device_equals_the_rule(ctx, umi_len, umi_dist, name):
    case = uc.case(name, umi_len)
    want = _rule(case, umi_len, umi_dist)
    _same(case, _device(ctx, case, umi_len, umi_dist), want, "umi_len %d dist %d" % (umi_len, umi_dist))
    if name in ("dense", "ladders", "runs") and umi_dist:
        assert want[1][:, 3].sum() < _rule(case, umi_len, 0)[1][:, 3].sum()     # (distance 1 merges here)


# ---- 2. table sizes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 1, 2, 511, 512, 513, 1023, 1024, 1025, 1 << 17, (1 << 17) + 1))
def test_table_size_boundaries(ctx, n):
    """all reads usable and all keys distinct: 512, 1024 and 2^17 reads fill half of their table, one read more doubles it"""
    case = uc.distinct_keys(12, n, seed=n)
    assert case.n == n
    for dist in (0, 1):
        got = _device(ctx, case, 12, dist)
        _same(case, got, uc.rule(case, 12, dist), "n %d dist %d" % (n, dist))
        assert got[1][:, 2].sum() == n
    if n <= 1025:
        c10 = uc.distinct_keys(10, n, seed=n + 1)
        _same(c10, _device(ctx, c10, 10, 1), uc.rule(c10, 10, 1), "umi_len 10 n %d" % n)


def test_no_reads(ctx):
    # cells and no reads: the counts are zeroed
    case = uc.Case("no_reads", [5, 9, 11], [])
    mol, cnt = _device(ctx, case, 12, 1)
    assert len(mol) == 0 and cnt.shape == (3, 4) and not cnt.any()
    # neither: nothing to do, and no error
    mol, cnt = _device(ctx, uc.Case("nothing", [], []), 12, 1)
    assert len(mol) == 0 and len(cnt) == 0
    # reads and no cells: no read has a molecule
    case = uc.Case("no_cells", [], [(7, 1, "ACGTACGTACGT")] * 3)
    mol, cnt = _device(ctx, case, 12, 1)
    assert (mol == ud.NONE).all() and len(cnt) == 0


# ---- 3. probes that wrap ----------------------------------------------------------------------------------------------------
def _slot_of(keys, mask):
    """slot_of of csrc/umi_kernels.hip (the 64-bit mix), on a uint64 array"""
    k = keys.astype(np.uint64)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xff51afd7ed558ccd)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xc4ceb9fe1a85ec53)
    k = k ^ (k >> np.uint64(33))
    return (k & np.uint64(0xFFFFFFFF)).astype(np.uint32) & np.uint32(mask)


def _occupied(case, P):
    """the slots linear probing fills with the case's keys (the same set in any insertion order), and how many keys sit
    below their home slot: they went past the last slot"""
    ordinal = np.searchsorted(case.cells, case.rank).astype(np.uint64)
    keys = ordinal << np.uint64(32) | case.umi.astype(np.uint64)
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


def test_probe_wrap(ctx):
    """forty sets of 512 distinct keys: the 1,024-slot table is half full, and in some of them the occupied slots run from
    the last slot on to the first, so inserts and lookups go round the end"""
    spanning = wrapping = 0
    for seed in range(40):
        n = 512 - seed % 3
        case = uc.distinct_keys(12 if seed % 2 else 10, n, seed=7000 + seed, n_cells=1 + seed % 4)
        umi_len = 12 if seed % 2 else 10
        used, wrapped = _occupied(case, 1024)
        assert used.sum() == n
        spanning += bool(used[1023] and used[0])
        wrapping += wrapped > 0
        _same(case, _device(ctx, case, umi_len, 1), uc.rule(case, umi_len, 1), "wrap seed %d" % seed)
    print("sets with slots 1023 and 0 both taken: %d, with a key stored past the end: %d" % (spanning, wrapping))
    assert spanning >= 5 and wrapping >= 1


# ---- 4. reuse, order, contexts ----------------------------------------------------------------------------------------------
def test_workspace_reuse(ctx):
    big = uc.dense(12, n=1 << 17, seed=9)
    small = uc.distinct_keys(12, 300, seed=300)
    want_big, want_small = uc.rule(big, 12, 1), uc.rule(small, 12, 1)
    first = _device(ctx, big, 12, 1)
    _same(big, first, want_big, "first large call")
    _same(small, _device(ctx, small, 12, 1), want_small, "small call after a large one")
    third = _device(ctx, big, 12, 1)
    _same(big, third, want_big, "large call again")
    assert first[0].tobytes() == third[0].tobytes() and first[1].tobytes() == third[1].tobytes()


def test_same_answer_every_time_in_any_order_on_any_context(ctx):
    case = uc.case("dense", 12)
    want = _rule(case, 12, 1)
    runs = [_device(ctx, case, 12, 1) for _ in range(3)]
    for r in runs:
        _same(case, r, want, "repeat")
        assert r[0].tobytes() == runs[0][0].tobytes() and r[1].tobytes() == runs[0][1].tobytes()
    shuffled, perm = case.shuffled(21)
    got = _device(ctx, shuffled, 12, 1)
    assert (got[0] == runs[0][0][perm]).all() and (got[1] == runs[0][1]).all()
    other = _native.Context(0)
    try:
        again = _device(other, case, 12, 1)
    finally:
        other.close()
    assert again[0].tobytes() == runs[0][0].tobytes() and again[1].tobytes() == runs[0][1].tobytes()


# ---- 5. rejections ----------------------------------------------------------------------------------------------------------
def test_rejections_launch_nothing(ctx):
    case = uc.case("codes", 12)
    n, nc = case.n, len(case.cells)
    d = [_native.DeviceArray.from_host(ctx, a) for a in (case.cells, case.rank, case.has, case.umi)]
    d_mol, d_cnt = _poisoned(ctx, n), _poisoned(ctx, (nc, 4))
    good = dict(d_rank=d[1], d_has=d[2], d_umi=d[3], n=n, d_cells=d[0], n_cells=nc, umi_len=12, umi_dist=1, d_molecule=d_mol, d_cell_counts=d_cnt)
    bad = [dict(umi_dist=2), dict(umi_len=2), dict(umi_len=13), dict(d_rank=0), dict(d_has=0), dict(d_umi=0), dict(d_molecule=0)]
    for change in bad:
        with pytest.raises(_native.BadgerHipError):
            ctx.umi_dedup_dev(**dict(good, **change))
        # nothing ran: the outputs still hold the poison
        assert (d_mol.to_host() == POISON * 0x01010101).all() and (d_cnt.to_host() == POISON * 0x01010101).all(), change
    ctx.umi_dedup_dev(**good)                                        # the context still works
    _same(case, (d_mol.to_host(), d_cnt.to_host()), _rule(case, 12, 1), "after the rejections")
    for a in d + [d_mol, d_cnt]:
        a.free()


# ---- 6. k_umi_pack ----------------------------------------------------------------------------------------------------------
def _pack_reads(umi_len):
    """the suite's adversarial reads (tests/test_trim_gpu.py, the fragment fuzz of tests/test_hip_parity.py) and, on both
    strands, reads cut at every offset inside the UMI and UMIs holding N at the first, a middle and the last position"""
    from test_hip_parity import _fragment_reads
    from test_trim_gpu import _adversarial
    from badger_amd import trim
    wl = synth.make_whitelist(3000)
    b, o = synth.make_reads(1500, wl, seed=40 + umi_len, umi_len=umi_len)
    reads = synth.reads_to_list(b.cpu(), o.cpu())
    reads += _adversarial(reads, 50 + umi_len, umi_len)
    reads += _fragment_reads(np.random.default_rng(60 + umi_len), 3000)
    rng = np.random.default_rng(70 + umi_len)
    rs = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, size=n))       # noqa: E731
    planted = []
    for rep in range(6):
        head = rs(int(rng.integers(0, 41))) + synth.R1 + rs(16)
        umi = rs(umi_len)
        tail = "T" * 30 + rs(5) + rs(int(rng.integers(60, 200)))
        for cut in range(umi_len + 1):
            planted.append(head + umi[:cut])                         # the read ends inside the UMI
            planted.append(head + umi[:cut] + "T" * 4)               # ... or a few bases into the tail
        for p in (0, umi_len // 2, umi_len - 1):
            planted.append(head + umi[:p] + "N" + umi[p + 1:] + tail)
        planted.append(head + umi + tail)
    reads += planted + [trim.revcomp(s) for s in planted]
    return reads


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


def _kept_umis(ctx):
    ptr, n = ctx.kept_umis()
    out = np.zeros(n, dtype=np.uint32)
    if n:
        ctx._check(ctx.lib.bdg_mem_to_host(ctx.h, out.ctypes.data, ptr, out.nbytes))
    return out


def _column_codes(reads, recs):
    """umi_code of the UMI field of the row bdg_format_rows prints for every read ('*' and whatever else no code holds: NONE)"""
    from test_trim import _Chunk
    ck = _Chunk(["r%d" % i for i in range(len(reads))], reads)
    rows = _native.format_rows(ck.ch, recs)[0].decode().split("\n")[:-1]
    assert len(rows) == len(reads)
    fields = [r.split("\t")[2] for r in rows]
    return np.array([ud.umi_code(f) for f in fields], dtype=np.uint32), fields


@pytest.mark.parametrize("umi_len", (10, 12))
def test_packed_umis_equal_the_stage1_column(umi_len):
    reads = _pack_reads(umi_len)
    n = len(reads)
    bases, off = synth.list_to_reads(reads)
    ctx = _native.Context(0)
    try:
        want_recs = ctx.extract_batch(bases, off, umi_len)
        want, fields = _column_codes(reads, want_recs)
        rev = (want_recs["flags"] & _native.FLAG_REV) != 0
        ok = want != ud.NONE
        # the inputs hold what they are for: codes on both strands, every length up to 14, fields no code holds
        assert (ok & rev).sum() > 300 and (ok & ~rev).sum() > 300
        assert set(range(1, 15)) <= {len(f) for f, k in zip(fields, ok) if k}
        valid = want_recs["valid"] != 0
        assert sum(1 for f, v in zip(fields, valid) if v and "N" in f) >= 20 and sum(1 for f, v in zip(fields, valid) if v and len(f) > 14) >= 5
        assert (~valid).sum() > 300

        def check(got, recs, what):
            assert len(got) == n, (what, len(got), n)
            assert (recs == want_recs).all(), what
            bad = np.nonzero(got != want)[0]
            assert not len(bad), (what, len(bad), [(i, reads[i][:80], fields[i], hex(got[i]), hex(want[i])) for i in bad[:5].tolist()])

        ctx.extract_keep_records(True)
        ctx.extract_keep_umis(True)
        recs = _through_the_pipeline(ctx, bases, off, n, umi_len)
        check(_kept_umis(ctx), recs, "pipelined")
        # a queue far too small: every chunk overflows and is rerun by collect; its UMIs are kept once
        ctx.extract_keep_records(True)                               # (an empty array again)
        ctx.extract_set_queue_capacity(16)
        try:
            recs = _through_the_pipeline(ctx, bases, off, n, umi_len)
        finally:
            ctx.extract_set_queue_capacity(0)
        assert not (recs["flags"] & _native.FLAG_INCOMPLETE).any()
        check(_kept_umis(ctx), recs, "after the reruns")
        # off and on again: from zero
        ctx.extract_keep_umis(False)
        ctx.extract_keep_umis(True)
        assert ctx.kept_umis()[1] == 0
        o = np.ascontiguousarray(off[:101], dtype=np.uint64)
        ctx.extract_submit(0, bases.ctypes.data, o.ctypes.data, 100, umi_len)
        ctx.extract_collect(0, 100)
        got = _kept_umis(ctx)
        assert len(got) == 100 and (got == want[:100]).all()
        ctx.extract_keep_umis(False)
        ctx.extract_keep_records(False)
    finally:
        ctx.close()
