"""k nearest whitelist candidates on the GPU (bdg_nearest16_topk*): exactly the CPU restatement (full distance matrix in
numpy, sorted by (distance, caller index)) over query / list sizes, distances, k and paths; slot 0 and the slots at its
distance agree with nearest16; the probe and cooperative paths agree, overflowing queries included; record input;
rejections; and stage 1's whitelist_candidates column."""
import os

import numpy as np
import pytest

from badger_amd import _native, common, extract_raw_barcodes as erb, synth

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
EVEN = np.uint32(0x55555555)


def _ctx():
    return _native.default_context(0)


# ---- the restatement ----------------------------------------------------------------------------------------------------
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
    """the answer of §1 for every max_ed and k from one distance matrix: the order (ed, index) is the same for every max_ed,
    so the slots for max_ed m are the first entries of the order that lie within m"""

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

    def answer(self, max_ed, k):
        ed = (self.top[:, :k] >> np.uint64(32)).astype(np.int64)
        idx = (self.top[:, :k] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        hit = (self.top[:, :k] != np.iinfo(np.uint64).max) & (ed <= max_ed)
        n_within = np.minimum((self.d <= max_ed).sum(axis=1), 65535).astype(np.uint16)
        return np.where(hit, idx, NONE).astype(np.uint32), np.where(hit, ed, 255).astype(np.uint8), n_within


def test_restatement_matches_the_oracle_distance():
    from oracle import pyoracle as orc
    rng = np.random.default_rng(2)
    wl = synth.make_whitelist(300, seed=3)
    q = _queries(wl, 40, 4)
    d = lev_matrix(q, wl)
    for _ in range(400):
        i, j = int(rng.integers(0, len(q))), int(rng.integers(0, len(wl)))
        assert d[i, j] == orc.lev16_packed(int(q[i]), 16, int(wl[j]), 16), (i, j)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
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


def _check_all(ctx, q, wl, max_eds=(0, 1, 2, 3, 16), ks=(1, 2, 8), algos=(0, 2, 3)):
    want = Restated(q, wl)
    for max_ed in max_eds:
        for k in ks:
            wi, we, wn = want.answer(max_ed, k)
            for algo in algos:
                if algo == 2 and max_ed > 2:
                    continue
                ctx.nearest16_set_algo(algo)
                gi, ge, gn = ctx.nearest16_topk(q, wl, max_ed, k)
                for g, w, name in ((gi, wi, "idx"), (ge, we, "ed"), (gn, wn, "n_within")):
                    assert (g == w).all(), (algo, max_ed, k, len(q), len(wl), name, np.argwhere(g != w)[:4])
    ctx.nearest16_set_algo(0)


# ---- exact equality ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw", [1, 255, 256, 257, 4097, 12289])
def test_topk_equals_restatement(nw):
    ctx = _ctx()
    wl = synth.make_whitelist(nw, seed=nw)
    wl = wl[np.random.default_rng(nw).permutation(nw)]                # a shuffled caller order
    for nq in (1, 63, 64, 65, 4096):
        _check_all(ctx, _queries(wl, nq, nq * 7 + nw), wl)


def test_topk_tie_dense_list():
    ctx = _ctx()
    rng = np.random.default_rng(11)
    centres = rng.integers(0, 1 << 32, size=4, dtype=np.uint64).astype(np.uint32)
    wl = _tie_dense(centres, rng)
    q = np.concatenate([centres, _queries(wl, 300, 12), _queries(centres, 60, 13)]).astype(np.uint32)
    _check_all(ctx, q, wl)


# ---- consistency with nearest16 ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_list():
    wl = synth.make_whitelist(737280, seed=7)
    return wl[np.random.default_rng(8).permutation(len(wl))]


@pytest.mark.parametrize("algo", [2, 3])
def test_slot0_and_ties_agree_with_nearest16(big_list, algo):
    ctx = _ctx()
    q = _queries(big_list, 100000, 17)
    k = 8
    ctx.nearest16_set_algo(algo)
    bi, be, bt = ctx.nearest16(q, big_list, 2)
    ti, te, tn = ctx.nearest16_topk(q, big_list, 2, k)
    ctx.nearest16_set_algo(0)
    assert (ti[:, 0] == bi).all() and (te[:, 0] == be).all()
    at0 = ((te == te[:, :1]) & (te != 255)).sum(axis=1)
    assert (at0 == np.minimum(k, bt)).all()
    assert (tn >= bt).all() and ((tn == 0) == (be == 255)).all()
    # slots ascend by (ed, idx) and a slot is filled exactly when n_within reaches it
    key = (te.astype(np.uint64) << np.uint64(32)) | ti.astype(np.uint64)
    assert (key[:, 1:] > key[:, :-1])[te[:, 1:] != 255].all()
    assert ((te != 255).sum(axis=1) == np.minimum(tn, k)).all()


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


def test_probe_and_coop_agree(big_list):
    ctx = _ctx()
    q = _queries(big_list, 20000, 19)
    got = {}
    for algo in (2, 3):
        ctx.nearest16_set_algo(algo)
        got[algo] = ctx.nearest16_topk(q, big_list, 2, 8)
    ctx.nearest16_set_algo(0)
    for a, b in zip(got[2], got[3]):
        assert (a == b).all()


def test_probe_overflow_goes_to_coop_topk():
    ctx = _ctx()
    rng = np.random.default_rng(31)
    heavy, ents = _overflow_list(rng, 40)
    wl = np.unique(np.concatenate([synth.make_whitelist(30000, seed=5), ents])).astype(np.uint32)
    wl = wl[rng.permutation(len(wl))]
    q = np.concatenate([heavy, _queries(wl, 1000, 32)]).astype(np.uint32)
    q = q[rng.permutation(len(q))]
    want = Restated(q, wl)
    for k in (2, 8):
        wi, we, wn = want.answer(2, k)
        res = {}
        for algo in (2, 3):
            ctx.nearest16_set_algo(algo)
            ctx.profile(True)
            ctx.profile_reset()
            res[algo] = ctx.nearest16_topk(q, wl, 2, k)
            names = {n for n, (launches, _) in ctx.profile_read().items() if launches}
            ctx.profile(False)
            if algo == 2:
                assert "k_nearest_delins_topk" in names and "k_nearest_coop_topk_overflow" in names, names
                # the planted queries did overflow pass 2 (the overflow step runs on every call, an empty list included)
                assert len(heavy) <= ctx.nearest16_overflow_count() < len(q), ctx.nearest16_overflow_count()
            for g, w in zip(res[algo], (wi, we, wn)):
                assert (g == w).all(), (algo, k)
    ctx.nearest16_set_algo(0)
    # the best-hit probe path's overflow list, counted the same way
    ctx.nearest16_set_algo(2)
    ctx.nearest16(q, wl, 2)
    assert 0 < ctx.nearest16_overflow_count() < len(q)
    ctx.nearest16(q[~np.isin(q, heavy)], wl, 1)               # max_ed 1: no pass 2, nothing overflows
    assert ctx.nearest16_overflow_count() == 0
    ctx.nearest16_set_algo(0)


# ---- device forms, records, rejections ------------------------------------------------------------------------------------------
def test_dev_forms_and_unusable_records():
    import torch
    ctx = _ctx()
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    wl = synth.make_whitelist(5000, seed=4)
    rng = np.random.default_rng(21)
    n, k = 1000, 4
    recs = np.zeros(n, dtype=_native.REC_DTYPE)
    recs["bc_rank"] = _queries(wl, n, 22)
    kind = rng.integers(0, 4, size=n)
    recs["valid"] = kind != 0
    recs["flags"] = np.where(kind >= 2, _native.FLAG_RANK_OK | _native.FLAG_BC16, np.where(kind == 1, _native.FLAG_BC16, 0))
    usable = (recs["flags"] & _native.FLAG_RANK_OK) != 0
    ctx.whitelist_load(wl)
    want = Restated(recs["bc_rank"], wl)
    d_recs = torch.from_numpy(recs.view(np.int32).reshape(-1, 8).copy()).to(dev)
    d_q = torch.from_numpy(recs["bc_rank"].view(np.int32).copy()).to(dev)
    for max_ed in (1, 2, 3):
        wi, we, wn = want.answer(max_ed, k)
        for algo in (0, 3):
            ctx.nearest16_set_algo(algo)
            for recs_in in (False, True):
                bi = torch.full((n * k,), 7, dtype=torch.int32, device=dev)
                be = torch.full((n * k,), 7, dtype=torch.uint8, device=dev)
                bn = torch.full((n,), 7, dtype=torch.int16, device=dev)
                if recs_in:
                    ctx.nearest16_topk_recs_dev(d_recs, n, max_ed, k, bi, be, bn)
                else:
                    ctx.nearest16_topk_dev(d_q, n, max_ed, k, bi, be, bn)
                ctx.synchronize()
                gi = bi.cpu().numpy().view(np.uint32).reshape(n, k)
                ge = be.cpu().numpy().reshape(n, k)
                gn = bn.cpu().numpy().view(np.uint16)
                ei, ee, en = wi.copy(), we.copy(), wn.copy()
                if recs_in:
                    ei[~usable], ee[~usable], en[~usable] = NONE, 255, 0
                assert (gi == ei).all() and (ge == ee).all() and (gn == en).all(), (algo, max_ed, recs_in)
    ctx.nearest16_set_algo(0)
    ctx.set_stream(None)


def test_rejections():
    import torch
    ctx = _native.Context(0)
    wl = synth.make_whitelist(500, seed=1)
    q = _queries(wl, 10, 2)
    for k in (0, 9):
        with pytest.raises(_native.BadgerHipError):
            ctx.nearest16_topk(q, wl, 2, k)
    ctx.nearest16_set_algo(1)
    with pytest.raises(_native.BadgerHipError):
        ctx.nearest16_topk(q, wl, 2, 3)
    ctx.nearest16_set_algo(2)
    with pytest.raises(_native.BadgerHipError):
        ctx.nearest16_topk(q, wl, 3, 3)
    ctx.nearest16_topk(q, wl, 2, 3)
    # record input in overlap mode is refused at the call as well
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    ctx.whitelist_load(wl)
    ctx.set_overlap(True)
    d_recs = torch.zeros((10, 8), dtype=torch.int32, device=dev)
    bi = torch.zeros(30, dtype=torch.int32, device=dev)
    be = torch.zeros(30, dtype=torch.uint8, device=dev)
    bn = torch.zeros(10, dtype=torch.int16, device=dev)
    for algo, max_ed, k in ((1, 2, 3), (2, 3, 3), (0, 2, 0), (0, 2, 9)):
        ctx.nearest16_set_algo(algo)
        with pytest.raises(_native.BadgerHipError):
            ctx.nearest16_topk_recs_dev(d_recs, 10, max_ed, k, bi, be, bn)
    ctx.nearest16_set_algo(0)
    ctx.nearest16_topk_recs_dev(d_recs, 10, 2, 3, bi, be, bn)
    ctx.synchronize()
    assert (bn.cpu().numpy() == 0).all()                     # zero records: no usable barcode
    ctx.close()


# ---- stage 1 ----------------------------------------------------------------------------------------------------------------
def _run(tmp_path, golden_dir, name, *extra):
    out = str(tmp_path / name)
    erb.main(["--mode", "tenX_v3", "-i", os.path.join(golden_dir, "c1_reads.fa.gz"), "-o", out,
              "-b", os.path.join(golden_dir, "c1_whitelist.txt")] + list(extra))
    return out


def _want_candidates(rows, wl, max_ed, k):
    bcs = [r.split("\t")[1] for r in rows]
    ok = np.array([len(b) == 16 and not b.strip("ACGT") for b in bcs])
    ranks = np.array([common.rank(b, 16) if o else 0 for b, o in zip(bcs, ok)], dtype=np.uint32)
    wi, we, _ = Restated(ranks, wl).answer(max_ed, k)
    out = []
    for o, ii, ee in zip(ok, wi, we):
        c = ["%s:%d" % (common.unrank(int(wl[i]), 16), e) for i, e in zip(ii, ee) if e != 255] if o else []
        out.append(",".join(c) if c else "*")
    return out


@pytest.mark.parametrize("max_ed", [None, 3])
def test_stage1_candidates_column(tmp_path, golden_dir, max_ed):
    dist = [] if max_ed is None else ["--max_bc_dist", str(max_ed)]
    wl = erb.load_barcodes(os.path.join(golden_dir, "c1_whitelist.txt"))
    for t in ("1", "4"):
        plain = _run(tmp_path, golden_dir, "plain%s.tsv" % t, "-t", t, *dist)
        cand = _run(tmp_path, golden_dir, "cand%s.tsv" % t, "-t", t, "--bc_candidates", "3", *dist)
        p = open(plain).read().split("\n")
        c = open(cand).read().split("\n")
        assert len(p) == len(c)
        for a, b in zip(p, c):
            if a.startswith("#"):
                assert b == a + "\t" + erb.CANDIDATES_COLUMN
            elif a:
                assert b.rsplit("\t", 1)[0] == a
        assert open(cand + ".stats").read() == open(plain + ".stats").read()
        rows = [l for l in c[:-1] if not l.startswith("#")]
        assert [r.rsplit("\t", 1)[1] for r in rows] == _want_candidates(rows, wl, 2 if max_ed is None else max_ed, 3)
        assert any(r.rsplit("\t", 1)[1] != "*" for r in rows)


def test_stage1_candidates_over_contexts(tmp_path, monkeypatch):
    """--gpus 3 rehearsed with three contexts of one device, many chunks: the bytes of the one-context run"""
    wl = synth.make_whitelist(3000)
    wl = wl[np.random.default_rng(1).permutation(len(wl))]
    wl_path = str(tmp_path / "wl.txt")
    with open(wl_path, "w") as f:
        f.write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    bases, off = synth.make_reads(20000, wl, seed=35)
    seqs = synth.reads_to_list(bases, off)
    path = str(tmp_path / "reads.fastq")
    with open(path, "w") as f:
        f.write("".join("@read_%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(seqs)))
    monkeypatch.setenv("BADGER_AMD_CONTEXTS_ON_ONE_DEVICE", "1")
    monkeypatch.setenv("BADGER_AMD_SEGMENT_MB", "1")
    outs = {}
    for gpus in ("1", "3"):
        for t in ("1", "5"):
            out = str(tmp_path / ("g%s_t%s.tsv" % (gpus, t)))
            erb.main(["--mode", "tenX_v3", "-i", path, "-o", out, "-b", wl_path, "--max_bc_dist", "3", "--bc_candidates", "8",
                      "-t", t, "--gpus", gpus])
            outs[(gpus, t)] = (open(out).read(), open(out + ".stats").read())
    for t in ("1", "5"):
        assert outs[("1", t)] == outs[("3", t)]
    rows = [l for l in outs[("1", "1")][0].split("\n")[1:-1]]
    assert [r.rsplit("\t", 1)[1] for r in rows] == _want_candidates(rows, wl, 3, 8)


def test_topk_after_deferred_match_in_overlap_mode():
    """overlap mode: a best-hit record match is deferred (queued on the auxiliary stream later), then a top-k record match
    goes on the main stream; the two share the match workspaces, so the top-k must run after it - both answers exact.  Also
    with the deferred match flushed by the next extraction before the top-k call."""
    import torch
    from oracle import pyoracle as orc
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    wl = synth.make_whitelist(5000, seed=61)
    ctx.whitelist_load(wl)
    ctx.set_overlap(True)

    def batch(n, seed):
        bases, off = synth.make_reads(n, wl, seed=seed)
        b, o = bases.numpy(), off.numpy().astype(np.int64)
        d_b = torch.from_numpy(np.concatenate([b, np.zeros(64, np.uint8)])).to(dev)
        d_o = torch.from_numpy(o).to(dev)
        d_r = torch.zeros((n, 8), dtype=torch.int32, device=dev)
        ctx.extract_batch_dev(d_b, d_o, n, int(o[-1]), 12, d_r)
        return orc.extract_batch(b, o.astype(np.uint64), 12, threads=16), d_r

    def best_want(recs):
        ok = (recs["flags"] & _native.FLAG_RANK_OK) != 0
        wi, we, wt = orc.nearest16(recs["bc_rank"], wl, 2, threads=16)
        wi[~ok], we[~ok], wt[~ok] = NONE, 255, 0
        return wi, we

    def topk_want(recs, k):
        ok = (recs["flags"] & _native.FLAG_RANK_OK) != 0
        wi, we, wn = Restated(recs["bc_rank"], wl).answer(2, k)
        wi[~ok], we[~ok], wn[~ok] = NONE, 255, 0
        return wi, we, wn

    k = 8
    for algo in (2, 0):
        ctx.nearest16_set_algo(algo)
        for flush_first in (False, True):
            ra, da = batch(3000, 70 + algo)
            n = len(ra)
            bi = torch.zeros(n, dtype=torch.int32, device=dev)
            be = torch.zeros(n, dtype=torch.uint8, device=dev)
            bt = torch.zeros(n, dtype=torch.int16, device=dev)
            ctx.nearest16_recs_dev(da, n, 2, bi, be, bt)              # deferred
            rb, db = (batch(2500, 80 + algo) if flush_first else (ra, da))
            m = len(rb)
            ti = torch.full((m * k,), 7, dtype=torch.int32, device=dev)
            te = torch.full((m * k,), 7, dtype=torch.uint8, device=dev)
            tn = torch.full((m,), 7, dtype=torch.int16, device=dev)
            ctx.nearest16_topk_recs_dev(db, m, 2, k, ti, te, tn)
            ctx.synchronize()
            wi, we = best_want(ra)
            assert (bi.cpu().numpy().view(np.uint32) == wi).all() and (be.cpu().numpy() == we).all(), (algo, flush_first)
            ki, ke, kn = topk_want(rb, k)
            assert (ti.cpu().numpy().view(np.uint32).reshape(m, k) == ki).all(), (algo, flush_first)
            assert (te.cpu().numpy().reshape(m, k) == ke).all() and (tn.cpu().numpy().view(np.uint16) == kn).all()
    ctx.nearest16_set_algo(0)
    ctx.close()


def test_stage1_bc_candidates_needs_the_flag(tmp_path):
    """bdg_stage1_opts.bc_candidates is the upper half of what was a 32-bit max_bc_dist: a caller that does not set
    BDG_STAGE1_WL_CANDIDATES and leaves it nonzero gets the old 'out of range' answer, not a fifth column"""
    import ctypes as C
    ctx = _native.Context(0)
    wl = synth.make_whitelist(100, seed=2)
    ctx.whitelist_load(wl)
    fa = tmp_path / "r.fa"
    fa.write_text(">r0\n" + "ACGT" * 40 + "\n")
    L = _native.load()
    arr = (C.c_void_p * 1)(ctx.h)
    header = b"#read_id\tbarcode\tUMI\tBC_score\tvalid_UMI\tstrand\tpolyT_start\tR1_end\twhitelist_barcode\twhitelist_dist\twhitelist_ties"
    for wl_mode, bc, ok in ((1, 1, False), (1, 0, True), (1 | _native.STAGE1_WL_CANDIDATES, 1, True),
                            (1 | _native.STAGE1_WL_CANDIDATES, 9, False)):
        o = _native.Stage1Opts(12, 1, 0, 0, 0, 0, 0, wl_mode, 2, bc)
        res = _native.Stage1Result()
        rc = L.bdg_stage1_run(arr, 1, str(fa).encode(), str(tmp_path / "o.tsv").encode(), header, C.byref(o), C.byref(res))
        assert (rc == 0) == ok, (wl_mode, bc, rc)
        if ok:
            cols = open(tmp_path / "o.tsv").read().split("\n")[1].split("\t")
            assert len(cols) == 11 + (1 if bc else 0)
    ctx.close()
