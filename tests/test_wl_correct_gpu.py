"""Abundance-weighted whitelist correction on the GPU: bdg_nearest16_correct against the host restatement
(badger_amd/wl_correct.py) fed by a numpy top-8 restatement, on both match paths, overflowing queries included; the call's
refusals; stage 1's --bc_correct against the restatement run on the oracle's records, over file shapes, contexts and
--bc_candidates; and the correction's accuracy on synthetic reads with known cells."""
import os

import numpy as np
import pytest

from badger_amd import _native, common, extract_raw_barcodes as erb, synth, wl_correct as wc

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
EVEN = np.uint32(0x55555555)


def _ctx():
    return _native.default_context(0)


# ---- the top-8 restatement (as tests/test_nearest_topk_gpu.py states it: the oracle has no top-k form) ------------------------
def lev_matrix(q, wl):
    """unit-cost Levenshtein distance of every (query, entry) pair of rank-packed 16-mers: Myers' bit-vector algorithm with
    the entry as the pattern (row i at bit 2i), the query read column by column, vectorised over the pairs"""
    q = np.asarray(q, np.uint32)
    wl = np.asarray(wl, np.uint32)
    out = np.empty((len(q), len(wl)), np.uint8)
    P0 = (wl & EVEN)[None, :]
    P1 = ((wl >> np.uint32(1)) & EVEN)[None, :]
    one = np.uint32(1)
    for r0 in range(0, len(q), 256):
        t = q[r0:r0 + 256, None]
        pv = np.full((len(t), len(wl)), 0xFFFFFFFF, np.uint32)
        mv = np.zeros_like(pv)
        score = np.full(pv.shape, 16, np.int32)
        for j in range(16):
            c0 = ((t >> np.uint32(2 * j)) & one) * np.uint32(0xFFFFFFFF)
            c1 = ((t >> np.uint32(2 * j + 1)) & one) * np.uint32(0xFFFFFFFF)
            eq = ~(P0 ^ c0) & ~(P1 ^ c1) & EVEN
            xv = eq | mv
            xh = (((eq & pv) + pv) ^ pv) | eq
            ph = mv | ~(xh | pv)
            mh = pv & xh
            score += ((ph >> np.uint32(30)) & one).astype(np.int32)
            score -= ((mh >> np.uint32(30)) & one).astype(np.int32)
            ph = (ph << one) << one | one
            mh = (mh << one) << one
            pv = mh | ~(xv | ph)
            mv = ph & xv
        out[r0:r0 + 256] = score
    return out


class Restated:
    """the top-8 lists of every max_ed from one distance matrix"""

    def __init__(self, q, wl):
        self.d = lev_matrix(q, wl)
        nq, nw = self.d.shape
        kk = min(8, nw)
        self.top = np.full((nq, 8), np.iinfo(np.uint64).max, np.uint64)
        cols = np.arange(nw, dtype=np.uint64)[None, :]
        for r0 in range(0, nq, 256):
            key = (self.d[r0:r0 + 256].astype(np.uint64) << np.uint64(32)) | cols
            top = np.partition(key, kk - 1, axis=1)[:, :kk] if nw > kk else key
            self.top[r0:r0 + 256, :kk] = np.sort(top, axis=1)

    def answer(self, max_ed, k=8):
        ed = (self.top[:, :k] >> np.uint64(32)).astype(np.int64)
        idx = (self.top[:, :k] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        hit = (self.top[:, :k] != np.iinfo(np.uint64).max) & (ed <= max_ed)
        n_within = np.minimum((self.d <= max_ed).sum(axis=1), 65535).astype(np.uint16)
        return np.where(hit, idx, NONE).astype(np.uint32), np.where(hit, ed, 255).astype(np.uint8), n_within


def _queries(wl, n, seed):
    """half of them near whitelist entries (a few edits), half uniform"""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    near = rng.random(n) < 0.5
    base = wl[rng.integers(0, len(wl), size=n)]
    for _ in range(3):
        pos = rng.integers(0, 16, size=n).astype(np.uint32)
        sub = rng.integers(0, 4, size=n).astype(np.uint32)
        mask = ~(np.uint32(3) << (2 * pos))
        hit = rng.random(n) < 0.7
        base = np.where(hit, (base & mask) | (sub << (2 * pos)), base).astype(np.uint32)
    return np.where(near, base, q).astype(np.uint32)


def _with_exact_hits(wl, q, seed, n_hot=40, reps=12):
    """the queries plus repeated exact copies of a few entries (support) and one-substitution variants of them (calls)"""
    rng = np.random.default_rng(seed)
    hot = wl[rng.choice(len(wl), size=min(n_hot, len(wl)), replace=False)]
    copies = np.repeat(hot, rng.integers(1, reps, size=len(hot)))
    pos = rng.integers(0, 16, size=len(copies)).astype(np.uint32)
    var = (copies & ~(np.uint32(3) << (2 * pos))) | (rng.integers(0, 4, size=len(copies)).astype(np.uint32) << (2 * pos))
    out = np.concatenate([q, copies, var.astype(np.uint32)]).astype(np.uint32)
    return out[rng.permutation(len(out))]


def _tie_dense(centres, rng, cap=6000):
    """one- and two-substitution neighbours of the centres and their single-base shifts (a sample of the two-edit ones)"""
    out = set()
    for c in centres.tolist():
        out.add(c)
        for i in range(16):
            for a in range(4):
                x = (c & ~(3 << (2 * i))) | (a << (2 * i))
                out.add(x)
                for j in rng.choice(16, size=3, replace=False).tolist():
                    out.add((x & ~(3 << (2 * j))) | (int(rng.integers(0, 4)) << (2 * j)))
        for a in range(4):
            out.add(((c << 2) | a) & 0xFFFFFFFF)
            out.add((c >> 2) | (a << 30))
    out = np.array(sorted(out), dtype=np.uint32)
    return out[rng.permutation(len(out))[:cap]]


def _overflow_list(rng, n_heavy):
    """queries with more than four entries one deletion + one insertion away (none within Hamming distance 2) behind the
    deletion variants one lane of the probe path's second pass owns: that lane's hit list overflows"""
    heavy = rng.integers(0, 1 << 32, size=n_heavy, dtype=np.uint64).astype(np.uint32)
    ents = set()
    for qv in heavy.tolist():
        s = "".join("ACGT"[(qv >> (2 * i)) & 3] for i in range(16))
        for i in range(4):
            d = s[:i] + s[i + 1:]
            for p in range(11, 16):
                for b in "ACGT":
                    e = d[:p] + b + d[p:]
                    if sum(x != y for x, y in zip(e, s)) > 2:
                        ents.add(sum("ACGT".index(ch) << (2 * k) for k, ch in enumerate(e)))
    return heavy, np.array(sorted(ents), dtype=np.uint32)


def _check(ctx, q, wl, max_eds=(0, 1, 2, 3), algos=(0, 2, 3), params=((5, 975), (1, 501), (8, 1000), (3, 900))):
    want = Restated(q, wl)
    statuses = set()
    for max_ed in max_eds:
        wi, we, wn = want.answer(max_ed)
        for bits, pm in params:
            w = wc.resolve(wi, we, wn, len(wl), max_ed, bits, pm)
            statuses |= set(w[4].tolist())
            for algo in algos:
                if algo == 2 and max_ed > 2:
                    continue
                ctx.nearest16_set_algo(algo)
                got = ctx.nearest16_correct(q, wl, max_ed, bits, pm)
                for g, x, name in zip(got, w, ("idx", "ed", "support", "permille", "status")):
                    assert g.dtype == x.dtype and (g == x).all(), (algo, max_ed, bits, pm, name, np.argwhere(g != x)[:4])
    ctx.nearest16_set_algo(0)
    return statuses


# ---- bdg_nearest16_correct --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw", [257, 4097])
def test_correct_equals_restatement(nw):
    ctx = _ctx()
    wl = synth.make_whitelist(nw, seed=nw)
    wl = wl[np.random.default_rng(nw).permutation(nw)]                # a shuffled caller order
    q = _with_exact_hits(wl, _queries(wl, 3000, nw + 1), nw + 2)
    statuses = _check(ctx, q, wl)
    assert {wc.NONE, wc.EXACT, wc.CORRECTED, wc.AMBIGUOUS} <= statuses, statuses


def test_correct_tie_dense_list():
    ctx = _ctx()
    rng = np.random.default_rng(11)
    centres = rng.integers(0, 1 << 32, size=4, dtype=np.uint64).astype(np.uint32)
    wl = _tie_dense(centres, rng)
    q = np.concatenate([centres, _queries(wl, 300, 12), _queries(centres, 60, 13)]).astype(np.uint32)
    q = _with_exact_hits(wl, q, 14, n_hot=60, reps=5)
    statuses = _check(ctx, q, wl, params=((5, 975), (2, 700)))
    assert wc.TRUNCATED in statuses and wc.AMBIGUOUS in statuses, statuses


def test_correct_with_overflowing_queries():
    ctx = _ctx()
    rng = np.random.default_rng(31)
    heavy, ents = _overflow_list(rng, 40)
    wl = np.unique(np.concatenate([synth.make_whitelist(30000, seed=5), ents])).astype(np.uint32)
    wl = wl[rng.permutation(len(wl))]
    q = _with_exact_hits(wl, np.concatenate([heavy, _queries(wl, 1000, 32)]).astype(np.uint32), 33)
    _check(ctx, q, wl, max_eds=(2,), algos=(2, 3))
    ctx.nearest16_set_algo(2)
    ctx.nearest16_correct(q, wl, 2)
    assert ctx.nearest16_overflow_count() >= len(heavy)              # the planted queries did take the overflow step
    ctx.nearest16_set_algo(0)


def test_correct_rejections():
    ctx = _ctx()
    wl = synth.make_whitelist(100, seed=1)
    q = wl[:10].copy()
    for args in ((4, 5, 975), (2, 0, 975), (2, 9, 975), (2, 5, 500), (2, 5, 1001)):
        with pytest.raises(_native.BadgerHipError) as e:
            ctx.nearest16_correct(q, wl, *args)
        assert e.value.code == _native.E_ARG, args
    ctx.nearest16_set_algo(1)
    with pytest.raises(_native.BadgerHipError) as e:
        ctx.nearest16_correct(q, wl, 2)
    assert e.value.code == _native.E_ARG
    ctx.nearest16_set_algo(2)
    with pytest.raises(_native.BadgerHipError):
        ctx.nearest16_correct(q, wl, 3)
    ctx.nearest16_set_algo(0)
    idx, ed, sup, pm, st = ctx.nearest16_correct(q, wl, 2)           # the context is usable afterwards
    assert (st == wc.EXACT).all() and (idx == np.arange(10)).all() and (sup == 1).all()


# ---- stage 1 --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_input(tmp_path_factory):
    d = tmp_path_factory.mktemp("corr")
    wl = synth.make_whitelist(3000)
    wl = wl[np.random.default_rng(1).permutation(len(wl))]
    wl_path = str(d / "wl.txt")
    with open(wl_path, "w") as f:
        f.write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    bases, off = synth.make_reads(20000, wl, seed=35, n_cells=300)
    seqs = synth.reads_to_list(bases, off)
    path = str(d / "reads.fastq")
    with open(path, "w") as f:
        f.write("".join("@read_%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(seqs)))
    return d, wl, wl_path, path, bases.numpy(), off.numpy().astype(np.uint64)


_ORACLE_LISTS = {}


def _want_corrected(run_input, max_ed, bits=5, pm=975):
    """the correction file from the oracle's records: their barcodes' top-8 lists (numpy), the rule (wl_correct)"""
    from oracle import pyoracle as orc
    _, wl, _, _, b, o = run_input
    if "top" not in _ORACLE_LISTS:
        recs = orc.extract_batch(b, o, 12, threads=16)
        usable = (recs["flags"] & _native.FLAG_RANK_OK) != 0
        q = np.where(usable, recs["bc_rank"], 0).astype(np.uint32)
        _ORACLE_LISTS["top"] = (Restated(q, wl), usable)
    top, usable = _ORACLE_LISTS["top"]
    li, le, ln = top.answer(max_ed)
    li[~usable], le[~usable], ln[~usable] = NONE, 255, 0
    res = wc.resolve(li, le, ln, len(wl), max_ed, bits, pm)
    return wc.rows(["read_%d" % i for i in range(len(usable))], res, wl)


def _stage1(run_input, name, *extra):
    d, _, wl_path, path, _, _ = run_input
    out = str(d / name)
    erb.main(["--mode", "tenX_v3", "-i", path, "-o", out, "-b", wl_path] + list(extra))
    return out


@pytest.mark.parametrize("max_ed", ["2", "3"])
def test_stage1_bc_correct(run_input, monkeypatch, max_ed):
    """main TSV and .stats as with -b alone (plus one line), the correction file as the restatement says; -t 1 / -t 5 and
    --gpus 1 / 3 (contexts of one device, 1 MB segments: many chunks each) give the same files"""
    monkeypatch.setenv("BADGER_AMD_CONTEXTS_ON_ONE_DEVICE", "1")
    monkeypatch.setenv("BADGER_AMD_SEGMENT_MB", "1")
    want = _want_corrected(run_input, int(max_ed))
    corrected = {}
    for t in ("1", "5"):
        plain = _stage1(run_input, "plain_%s_%s.tsv" % (max_ed, t), "-t", t, "--max_bc_dist", max_ed)
        for gpus in ("1", "3"):
            out = _stage1(run_input, "corr_%s_%s_%s.tsv" % (max_ed, t, gpus), "-t", t, "--max_bc_dist", max_ed, "--gpus", gpus,
                          "--bc_correct")
            assert open(out).read() == open(plain).read()
            stats = open(out + ".stats").read()
            assert stats.startswith(open(plain + ".stats").read())
            corrected[(t, gpus)] = open(out + erb.CORRECTED_SUFFIX).read()
            lines = corrected[(t, gpus)].split("\n")
            assert lines[-1] == "" and lines[:-1] == want, (t, gpus)
            n_called = sum(l.endswith(("\texact", "\tcorrected")) for l in want[1:])
            sep = ":\t" if t == "1" else ": "
            assert stats[len(open(plain + ".stats").read()):] == "Whitelist corrected%s%d\n" % (sep, n_called)
    assert len(set(corrected.values())) == 1
    st = [l.rsplit("\t", 1)[1] for l in want[1:]]
    assert st.count("corrected") > 0 and st.count("ambiguous") > 0 and st.count("exact") > 0 and st.count("none") > 0


def test_stage1_bc_correct_keeps_the_candidates_column(run_input):
    alone = _stage1(run_input, "cand.tsv", "-t", "1", "--bc_candidates", "3")
    both = _stage1(run_input, "cand_corr.tsv", "-t", "1", "--bc_candidates", "3", "--bc_correct")
    assert open(both).read() == open(alone).read()
    assert open(both + erb.CORRECTED_SUFFIX).read().split("\n")[:-1] == _want_corrected(run_input, 2)


def test_stage1_bc_correct_posterior_flag(run_input):
    out = _stage1(run_input, "p.tsv", "-t", "1", "--bc_correct", "--bc_min_posterior", "0.6", "--bc_edit_bits", "3")
    assert open(out + erb.CORRECTED_SUFFIX).read().split("\n")[:-1] == _want_corrected(run_input, 2, 3, 600)


# ---- accuracy on reads with known cells ------------------------------------------------------------------------------------------
def _accuracy(calls, truth):
    """recall: reads of a whitelist cell called right; precision: calls that are right"""
    called = calls != NONE
    right = called & (calls == truth)
    return right.sum() / len(truth), right.sum() / max(called.sum(), 1)


def accuracy_run(tmp_path, n_reads=200000, n_wl=3000000, bits_list=(3, 5, 7), seed=41):
    """stage 1 with -b --bc_correct on synthetic reads against an n_wl-entry list: per B, recall and precision of
    corrected_barcode and of whitelist_barcode (the unique nearest entry), over the reads whose true barcode is a list entry
    and that have a usable barcode"""
    wl = synth.make_whitelist(n_wl, seed=seed)
    wl_path = str(tmp_path / "big_wl.txt")
    with open(wl_path, "w") as f:
        f.write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    bases, off, truth = synth.make_reads(n_reads, wl, seed=seed + 1, with_truth=True)
    seqs = synth.reads_to_list(bases, off)
    path = str(tmp_path / "acc.fastq")
    with open(path, "w") as f:
        f.write("".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(seqs)))
    pos = {int(r): i for i, r in enumerate(wl.tolist())}
    tb = truth["barcode"].numpy().astype(np.int64) & 0xFFFFFFFF
    tidx = np.array([pos.get(int(x), -1) for x in tb], np.int64)

    def col(text, c):
        rows = [l.split("\t") for l in text.split("\n")[1:-1]]
        return np.array([pos[int(common.rank(r[c], 16))] if r[c] != "*" else NONE for r in rows], np.int64)

    out = {}
    for bits in bits_list:
        o = str(tmp_path / ("acc_%d.tsv" % bits))
        erb.main(["--mode", "tenX_v3", "-i", path, "-o", o, "-b", wl_path, "-t", "1", "--bc_correct", "--bc_edit_bits", str(bits)])
        main = open(o).read()
        hdr = main.split("\n", 1)[0].split("\t")
        wlc = col(main, hdr.index("whitelist_barcode"))
        usable = np.array([len(l.split("\t")[1]) == 16 and not l.split("\t")[1].strip("ACGT") for l in main.split("\n")[1:-1]])
        corr_text = open(o + erb.CORRECTED_SUFFIX).read()
        cor = col(corr_text, 1)
        keep = (tidx >= 0) & usable
        # how often the nearest distance is shared (whitelist_barcode '*' with a distance): the ties the correction settles
        rows = [l.split("\t") for l in main.split("\n")[1:-1]]
        ti, di = hdr.index("whitelist_ties"), hdr.index("whitelist_dist")
        tied = sum(1 for r in rows if int(r[di]) >= 0 and int(r[ti]) > 1)
        within = sum(1 for r in rows if int(r[di]) >= 0)
        status = [l.rsplit("\t", 1)[1] for l in corr_text.split("\n")[1:-1]]
        r_wl, p_wl = _accuracy(wlc[keep], tidx[keep])
        r_c, p_c = _accuracy(cor[keep], tidx[keep])
        out[bits] = dict(recall_whitelist=float(r_wl), precision_whitelist=float(p_wl), recall_corrected=float(r_c),
                         precision_corrected=float(p_c), reads=int(keep.sum()), rows_within_max_ed=within,
                         rows_tied=tied, status={k: status.count(k) for k in wc.STATUS})
    return out


# precision may fall by at most this much (absolute) against whitelist_barcode's (from the measured run)
PRECISION_MARGIN = 0.01


def test_correction_accuracy(tmp_path):
    acc = accuracy_run(tmp_path)
    print("wl_correct accuracy:", acc)
    for bits, a in acc.items():
        assert a["recall_corrected"] > a["recall_whitelist"], (bits, a)
        assert a["precision_corrected"] >= a["precision_whitelist"] - PRECISION_MARGIN, (bits, a)


# ---- callers built against the struct sizes before the correction ------------------------------------------------------------
def _guarded_result(old_size=136, guard=16):
    """a result buffer of the old bdg_stage1_result size followed by sentinel bytes"""
    import ctypes as C
    assert C.sizeof(_native.Stage1Result) == old_size
    buf = (C.c_uint8 * (old_size + guard))(*([0xA5] * (old_size + guard)))
    return buf, C.cast(buf, C.POINTER(_native.Stage1Result))


def test_old_size_result_is_not_overrun(run_input):
    """bdg_stage1_collect and bdg_stage1_run without BDG_STAGE1_WL_CORRECT write nothing past the 136-byte result a caller
    built against the old header passes"""
    import ctypes as C
    d, wl, _, path, _, _ = run_input
    ctx = _ctx()
    L = _native.load()
    o = _native.Stage1Opts(12, 1, 0, 0, 0, 0, 0)
    buf, res = _guarded_result()
    ids = _native.IdStore()
    assert L.bdg_stage1_collect(ctx.h, os.fsencode(path), C.byref(o), ids.h, res) == 0
    assert res.contents.reads == 20000 and len(ids) == 20000
    assert bytes(buf[136:]) == b"\xa5" * 16
    buf, res = _guarded_result()
    bad = _native.Stage1Opts(0, 1, 0, 0, 0, 0, 0)                   # rejected after the result is cleared
    assert L.bdg_stage1_collect(ctx.h, os.fsencode(path), C.byref(bad), ids.h, res) == _native.E_ARG
    assert bytes(buf[136:]) == b"\xa5" * 16
    ctx.whitelist_load(wl)
    for wl_mode in (0, 1):
        buf, res = _guarded_result()
        o = _native.Stage1Opts(12, 1, 0, 0, 0, 0, 0, wl_mode, 2, 0)
        arr = (C.c_void_p * 1)(ctx.h)
        assert L.bdg_stage1_run(arr, 1, os.fsencode(path), os.fsencode(str(d / "old.tsv")), b"#read_id", C.byref(o), res) == 0
        assert res.contents.reads == 20000
        assert bytes(buf[136:]) == b"\xa5" * 16, wl_mode
