"""Every per-chunk result of the pipelined path at once - records, trim, chimera, whitelist match with candidates, correction
store - on slots that regrow: bdg_stage1_run over two contexts in uneven chunks, with every chunk rerun and without, against each
other and against the one-shot wrappers; and submit / collect on one slot with a small, a large and a small chunk again.
Integers and text: every comparison is exact.  (The wrappers themselves are checked against the oracle and the Python rules
in test_hip_parity.py, test_trim_gpu.py, test_chimera_gpu.py and test_nearest_topk_gpu.py.)"""
import numpy as np
import pytest

from badger_amd import _native, synth
from ingest_chunk import Chunk as _Chunk

pytestmark = pytest.mark.gpu

N, W, K, MAX_BC_DIST, TSO_MIN, CHIM_ED = 2000, 2000, 3, 2, 20, 3
HEADER = ("#read_id\tbarcode\tUMI\tBC_score\tvalid_UMI\tstrand\tpolyT_start\tR1_end\twhitelist_barcode\twhitelist_dist\twhitelist_ties"
          "\twhitelist_candidates")


@pytest.fixture(scope="module")
def one_shot():
    """the reads and what the one-shot wrappers say about them (computed once, read only)"""
    wl = synth.make_whitelist(W)
    b, o = synth.make_reads(N, wl, seed=131, tso=True)
    bases, off = b.numpy(), o.numpy().astype(np.uint64)
    ctx = _native.Context(0)
    recs = ctx.extract_batch(bases, off, 12)
    trim = ctx.trim_batch(bases, off, recs, TSO_MIN)
    chim = ctx.chimera_batch(bases, off, recs, trim, CHIM_ED)
    ok = (recs["flags"] & _native.FLAG_RANK_OK) != 0           # (the match of records reports no hit for the others)
    bi, be, bt = ctx.nearest16(recs["bc_rank"], wl, MAX_BC_DIST)
    ci, ce, _ = ctx.nearest16_topk(recs["bc_rank"], wl, MAX_BC_DIST, K)
    ctx.close()
    bi[~ok], be[~ok], bt[~ok], ci[~ok], ce[~ok] = 0xFFFFFFFF, 255, 0, 0xFFFFFFFF, 255
    return dict(wl=wl, bases=bases, off=off, recs=recs, trim=trim, chim=chim, best=(bi, be, bt), cand=(ci, ce),
                ids=["r%d" % i for i in range(N)], reads=synth.reads_to_list(b, o))


def _counts(res):
    return {f: getattr(res, f) for f, _ in (_native.Stage1Result._fields_ + _native.Stage1ResultCorrect._fields_
                                            + _native.Stage1ResultTrim._fields_ + _native.Stage1ResultChimera._fields_)
            if not f.startswith("seconds_")}


def test_stage1_every_result_with_and_without_reruns(one_shot, tmp_path):
    S = one_shot
    fa = str(tmp_path / "reads.fa")
    with open(fa, "w") as f:
        f.write("".join(">%s\n%s\n" % (i, s) for i, s in zip(S["ids"], S["reads"])))
    ctxs = [_native.default_context(0, 0), _native.default_context(0, 1)]
    for c in ctxs:
        c.whitelist_load(S["wl"])
    runs = {}
    try:
        for cap in (16, 0):                                    # 16: every chunk overflows, is run again and matched again
            for c in ctxs:
                c.extract_set_queue_capacity(cap)
            out = str(tmp_path / ("cap%d" % cap))
            res = _native.stage1_run(ctxs, fa, out + ".tsv", HEADER, 12, threads=2, chunk_reads=300, whitelist=True,
                                     max_bc_dist=MAX_BC_DIST, bc_candidates=K, corrected_path=out + ".corr", trimmed_path=out + ".fa",
                                     tso_min_score=TSO_MIN, chimera_max_ed=CHIM_ED)
            assert isinstance(res, _native.Stage1ResultChimera)
            runs[cap] = (_counts(res), [open(out + e, "rb").read() for e in (".tsv", ".corr", ".fa")])
    finally:
        for c in ctxs:
            c.extract_set_queue_capacity(0)
    (counts_a, files_a), (counts_b, files_b) = runs[16], runs[0]
    assert files_a[0] == files_b[0] and files_a[1] == files_b[1] and files_a[2] == files_b[2]
    assert counts_a == counts_b
    assert counts_b["reads"] == N and counts_b["chunks"] >= 7 and counts_b["whitelist_barcodes"] > 0 and len(files_b[1]) > 0
    # the one-shot wrappers on the same reads
    ck = _Chunk(S["ids"], S["bases"], S["off"])
    bi, be, bt = S["best"]
    rows, _ = _native.format_rows_wlk(ck.ch, S["recs"], bi, be, bt, S["cand"][0], S["cand"][1], S["wl"])
    assert files_b[0] == HEADER.encode() + b"\n" + rows
    text, six = _native.format_trimmed_chimera(ck.ch, S["recs"], S["trim"], S["chim"], bi, bt, S["wl"])
    assert files_b[2] == text
    assert six == tuple(counts_b[f] for f in ("trimmed_reads", "trimmed_tso", "trimmed_bases", "chimera_cut", "chimera_dropped", "chimera_bases"))
    assert six[1] > 0                                          # (the reads end in the TSO: the trim has work)


def test_slot_regrows_and_is_reused(one_shot):
    """slot 0 takes 50 reads, then 1,500, then 50 again: every mirror of the slot regrows once while it is idle and is reused"""
    S = one_shot
    bases, off = S["bases"], S["off"]
    ctx = _native.Context(0)
    ctx.extract_set_trim(True, TSO_MIN)
    ctx.extract_set_chimera(True, CHIM_ED)
    for a, m in ((0, 50), (100, 1500), (1900, 50)):
        o = np.ascontiguousarray(off[a:a + m + 1], dtype=np.uint64)
        ctx.extract_submit(0, bases.ctypes.data, o.ctypes.data, m, 12)
        got = ctx.extract_collect(0, m), ctx.extract_collect_trim(0, m), ctx.extract_collect_chimera(0, m)
        for g, w in zip(got, (S["recs"], S["trim"], S["chim"])):
            assert g.tobytes() == w[a:a + m].tobytes(), (a, m, g.dtype.names)
    ctx.close()
