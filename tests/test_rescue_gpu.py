"""Barcode rescue on the GPU: bdg_rescue_batch and the device form against badger_amd/rescue.py on every field of every record,
the store's independence of order, the pipelined path in uneven chunks (with a forced queue overflow) against the one-call form,
the wave's edge lanes, and the command line end to end."""
import logging

import numpy as np
import pytest

import rescue_cases as rc
from badger_amd import _native, common, extract_raw_barcodes as erb, rescue, synth

pytestmark = pytest.mark.gpu

SETTINGS = [(d, m) for d in (0, 1, 2) for m in (1, 3)]
_CACHE = {}


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in rescue.FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert not len(bad), (what, f, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def _set():
    """the case reads and 3,000 generated ones under hand-made records, the whitelist of 2,000 entries with its cluster, a support
    array given directly, and the rule's records at every setting (one matcher, shared by the tests)"""
    if not _CACHE:
        S = rc.build()
        reads, recs = rc.random_set(3000, 3, S["wl"], S["support"])
        reads = [c[1] for c in S["cases"]] + reads
        recs = np.concatenate([np.array([c[2] for c in S["cases"]], dtype=_native.REC_DTYPE), recs])
        bases, off = synth.list_to_reads(reads)
        m = rescue.Matcher(S["wl"])
        want = {s: rescue.rescue_batch(bases, off, recs, rc.U, S["wl"], S["support"], s[0], s[1], matcher=m) for s in SETTINGS}
        _CACHE.update(S, reads=reads, recs=recs, bases=bases, off=off, matcher=m, want=want)
    return _CACHE


def _ctx(S):
    ctx = _native.Context(0)
    ctx.whitelist_load(S["wl"])
    return ctx


# ---- 1. parity ----------------------------------------------------------------------------------------------------------
def test_rescue_batch_equals_the_rule():
    S = _set()
    ctx = _ctx(S)
    for d, m in SETTINGS:
        got = ctx.rescue_batch(S["bases"], S["off"], S["recs"], rc.U, S["support"], d, m)
        _same(got, S["want"][(d, m)], "rescue_batch max_ed %d min_support %d" % (d, m))
        assert ctx.rescue_counts() == (len(got), sum(1 for r in S["recs"] if rescue.eligible(r)))
    st = S["want"][(1, 1)]["status"]
    assert {int(x) for x in st} == {0, 1, 2, 3} and (st == rescue.RESCUED).sum() > 900
    # the hand-built cases, by name, at the defaults
    got = ctx.rescue_batch(S["bases"], S["off"], S["recs"], rc.U, S["support"])
    by_read = {int(r["read"]): r for r in got}
    for i, (name, _, _, want) in enumerate(S["cases"]):
        if want is None:
            assert i not in by_read, name
        else:
            assert {k: (bytes(by_read[i][k]) if k == "umi" else by_read[i][k].item()) for k in rescue.FIELDS[1:]} == \
                {k: want[k] for k in rescue.FIELDS[1:]}, name
    # another UMI length moves every window
    want10 = rescue.rescue_batch(S["bases"], S["off"], S["recs"], 10, S["wl"], S["support"], matcher=S["matcher"])
    _same(ctx.rescue_batch(S["bases"], S["off"], S["recs"], 10, S["support"]), want10, "umi_len 10")
    for umi_len, max_ed in ((0, 1), (15, 1), (12, 3)):
        with pytest.raises(_native.BadgerHipError):
            ctx.rescue_batch(S["bases"], S["off"], S["recs"], umi_len, S["support"], max_ed, 2)
    assert len(ctx.rescue_batch(S["bases"][:0], S["off"][:1], S["recs"][:0], rc.U, S["support"])) == 0
    ctx.extract_set_layout(_native.LAYOUT_5P)                             # no read of the 5' layout is eligible
    assert len(ctx.rescue_batch(S["bases"], S["off"], S["recs"], rc.U, S["support"])) == 0
    ctx.extract_set_layout(_native.LAYOUT_3P)
    nowl = _native.Context(0)
    with pytest.raises(_native.BadgerHipError):
        nowl.rescue_batch(S["bases"], S["off"], S["recs"], rc.U, S["support"])
    nowl.close()
    ctx.close()


def _real_set():
    """reads that go through the extraction: 2,000 of the error model, 1,000 more with the adapter cut off, 300 of random bases
    with a planted tail, the suite's adversarial reads and the case reads; the whitelist the reads were made from, with the
    support their own records give"""
    if "real" not in _CACHE:
        from test_trim_gpu import _adversarial
        S = _set()
        wl = synth.make_whitelist(2000)
        reads, kind, _ = rescue.cut_read_set(2000, 1000, 300, wl, 41, 100, errors=(0.01, 0.005, 0.005))
        reads += _adversarial(reads, 42, rc.U) + [c[1] for c in S["cases"]]
        bases, off = synth.list_to_reads(reads)
        ctx = _native.Context(0)
        recs = ctx.extract_batch(bases, off, rc.U)
        ctx.close()
        sup = rescue.exact_support(recs, reads, wl)
        m = rescue.Matcher(wl)
        want = {s: rescue.rescue_batch(bases, off, recs, rc.U, wl, sup, s[0], s[1], matcher=m) for s in ((1, 2), (2, 1))}
        _CACHE["real"] = dict(wl=wl, reads=reads, bases=bases, off=off, recs=recs, support=sup, want=want)
    return _CACHE["real"]


def test_rescue_batch_dev_behind_the_extraction():
    import torch
    R = _real_set()
    n = len(R["reads"])
    dev = torch.device("cuda", 0)
    total = int(R["off"][-1])
    d_bases = torch.zeros((total + 15) // 16 * 16 + 64, dtype=torch.uint8, device=dev)
    d_bases[:total] = torch.from_numpy(R["bases"][:total]).to(dev)
    d_off = torch.from_numpy(R["off"].astype(np.int64)).to(dev)
    d_recs = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_sup = torch.from_numpy(R["support"].view(np.int32)).to(dev)
    d_out = torch.full((n * 40,), 0xAB, dtype=torch.uint8, device=dev)
    ctx = _native.Context(0)
    ctx.whitelist_load(R["wl"])
    ctx.set_stream(0)
    for _ in range(8):
        ctx.extract_batch_dev(d_bases, d_off, n, total, rc.U, d_recs)
        rc_, _, _ = ctx.extract_status()
        if rc_ != _native.E_CAPACITY:
            break
    assert rc_ == 0
    m = ctx.rescue_batch_dev(d_bases, d_off, n, d_recs, rc.U, d_sup, 1, 2, d_out)
    torch.cuda.synchronize()
    assert (d_recs.cpu().numpy().view(_native.REC_DTYPE) == R["recs"]).all()
    got = d_out.cpu().numpy()[:m * 40].view(_native.RESCUE_DTYPE)
    _same(got[np.argsort(got["read"])], R["want"][(1, 2)], "rescue_batch_dev")
    assert (R["want"][(1, 2)]["status"] == rescue.RESCUED).sum() > 100
    with pytest.raises(_native.BadgerHipError):
        ctx.rescue_batch_dev(d_bases, d_off, n, d_recs, rc.U, d_sup, 3, 2, d_out)
    ctx.close()


# ---- 2. the order of the store --------------------------------------------------------------------------------------------
def test_shuffled_reads_and_a_second_context_give_the_same_records():
    S = _set()
    n = len(S["reads"])
    perm = np.random.default_rng(9).permutation(n)
    reads = [S["reads"][i] for i in perm]
    bases, off = synth.list_to_reads(reads)
    want = S["want"][(1, 1)]
    a, b = _ctx(S), _ctx(S)
    for ctx in (a, b, a):
        got = ctx.rescue_batch(bases, off, S["recs"][perm], rc.U, S["support"], 1, 1)
        back = got.copy()
        back["read"] = perm[got["read"]]
        _same(back[np.argsort(back["read"])], want, "shuffled")
        _same(ctx.rescue_batch(S["bases"], S["off"], S["recs"], rc.U, S["support"], 1, 1), want, "in order again")
    a.close()
    b.close()


# ---- 3. the pipelined path ------------------------------------------------------------------------------------------------
def _pipeline(ctx, bases, off, n, sizes, umi_len):
    recs, flying = [], []

    def collect():
        slot, a, b, _ = flying.pop(0)
        recs.append(ctx.extract_collect(slot, b - a))

    a, k = 0, 0
    while a < n:
        b = min(a + sizes[k % len(sizes)], n)
        if len(flying) >= 3:
            collect()
        o = np.ascontiguousarray(off[a:b + 1], dtype=np.uint64)       # (stays alive until the chunk is collected)
        ctx.extract_submit(k % _native.SLOTS, bases.ctypes.data, o.ctypes.data, b - a, umi_len)
        flying.append((k % _native.SLOTS, a, b, o))
        a, k = b, k + 1
    while flying:
        collect()
    return np.concatenate(recs)


def test_submit_collect_in_uneven_chunks_and_overflow_rerun():
    R = _real_set()
    bases, off, n = R["bases"], R["off"], len(R["reads"])
    ctx = _native.Context(0)
    ctx.whitelist_load(R["wl"])
    d_sup = _native.DeviceArray.from_host(ctx, R["support"])
    one_call = {s: ctx.rescue_batch(bases, off, R["recs"], rc.U, R["support"], s[0], s[1]) for s in R["want"]}
    for s in R["want"]:
        _same(one_call[s], R["want"][s], "one call %r" % (s,))
    elig = sum(1 for r in R["recs"] if rescue.eligible(r))
    with pytest.raises(_native.BadgerHipError):
        ctx.extract_rescue_resolve(d_sup)                                 # the rescue is off
    for cap in (0, 16):                                                   # 16: every chunk that can overflow does, and is run again
        ctx.extract_set_rescue(True)
        with pytest.raises(_native.BadgerHipError):
            ctx.rescue_batch(bases, off, R["recs"], rc.U, R["support"])   # the store is in use
        ctx.extract_set_queue_capacity(cap)
        got_recs = _pipeline(ctx, bases, off, n, (1, 63, 64, 65, 1000), rc.U)
        ctx.extract_set_queue_capacity(0)
        assert (got_recs == R["recs"]).all()
        for s in R["want"]:                                               # (the store stays: resolved twice, under two settings)
            _same(ctx.extract_rescue_resolve(d_sup, s[0], s[1]), one_call[s], "pipelined, queue capacity %d, %r" % (cap, s))
        assert ctx.rescue_counts() == (len(one_call[(1, 2)]), elig)
        ctx.extract_set_rescue(False)
    # off again: nothing is stored, the one-call form serves
    _pipeline(ctx, bases, off, 500, (100,), rc.U)
    assert ctx.rescue_counts() == (0, 0)
    _same(ctx.rescue_batch(bases, off, R["recs"], rc.U, R["support"], 1, 2), one_call[(1, 2)], "after the pipeline")
    d_sup.free()
    ctx.close()


# ---- 4. a wave's edge lanes -----------------------------------------------------------------------------------------------
def test_eligible_reads_at_lane_0_and_lane_63_and_none_at_all():
    S = _set()
    read = S["cases"][0][1]                                               # "tail on the forward strand": rescued, entry E_A
    n = 192
    bases, off = synth.list_to_reads([read] * n)
    recs = np.zeros(n, dtype=_native.REC_DTYPE)
    recs["valid"] = 1
    ctx = _ctx(S)
    got = ctx.rescue_batch(bases, off, recs, rc.U, S["support"])
    assert len(got) == 0 and ctx.rescue_counts() == (0, 0)
    recs["valid"][[64, 127]] = 0                                          # lanes 0 and 63 of the second wave
    got = ctx.rescue_batch(bases, off, recs, rc.U, S["support"])
    assert ctx.rescue_counts() == (2, 2) and got["read"].tolist() == [64, 127]
    assert (got["status"] == rescue.RESCUED).all() and (got["entry"] == S["index"][rc.E_A]).all() and (got["umi"] == rc.UMI.encode()).all()
    recs["flags"][:] = _native.FLAG_INCOMPLETE                            # placeholders: nothing is eligible
    assert len(ctx.rescue_batch(bases, off, recs, rc.U, S["support"])) == 0 and ctx.rescue_counts() == (0, 0)
    ctx.close()


# ---- 5. the command line --------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path, monkeypatch, caplog):
    """3,300 reads: 2,000 of the error model, 1,000 more of the same cells with the first 40 bases cut off, 300 of random bases with a
    planted tail.  Under rescue.py alone 167 of the 1,000 cut reads are rescued on this seed and no random-base read is; half cannot be
    with a 40-base cut of synth.make_reads reads (DESIGN 4.16 says why).  The assertion is equality with the rule."""
    R = _real_set()
    n = 3300
    reads, ids = R["reads"][:n], ["read_%d" % i for i in range(n)]
    bases, off = synth.list_to_reads(reads)
    recs = R["recs"][:n]
    fq = str(tmp_path / "reads.fastq")
    with open(fq, "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in zip(ids, reads)))
    wl = R["wl"][np.random.default_rng(2).permutation(len(R["wl"]))]
    wl_path = str(tmp_path / "wl.txt")
    open(wl_path, "w").write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    sup = rescue.exact_support(recs, reads, wl)
    want = rescue.rescue_batch(bases, off, recs, rc.U, wl, sup)
    st = want["status"]
    cut = (want["read"] >= 2000) & (want["read"] < 3000)
    assert (st[cut] == rescue.RESCUED).sum() >= 150 and (st[want["read"] >= 3000] != rescue.RESCUED).all()
    monkeypatch.setenv("BADGER_AMD_CONTEXTS_ON_ONE_DEVICE", "1")
    monkeypatch.setenv("BADGER_AMD_SEGMENT_MB", "1")
    base = ["--mode", "tenX_v3", "-i", fq, "-t", "4", "-b", wl_path, "--bc_correct"]
    plain = str(tmp_path / "plain.tsv")
    erb.main(base + ["-o", plain])
    # the run's support, from its own correction file: the reads called exact, per barcode
    where = {common.unrank(int(r), 16): i for i, r in enumerate(wl)}
    run_sup = np.zeros(len(wl), dtype=np.uint32)
    for line in open(plain + ".corrected.tsv").read().split("\n")[1:-1]:
        f = line.split("\t")
        if f[5] == "exact":
            run_sup[where[f[1]]] += 1
    assert (run_sup == sup).all() and (sup >= 2).sum() > 50
    for gpus, extra in (("1", []), ("2", []), ("1", ["--rescue_max_ed", "2", "--rescue_min_support", "1"])):
        out = str(tmp_path / ("r%s%d.tsv" % (gpus, len(extra))))
        w = want if not extra else rescue.rescue_batch(bases, off, recs, rc.U, wl, sup, 2, 1)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="BarcodeGraph"):
            erb.main(base + ["-o", out, "--gpus", gpus, "--bc_rescue"] + extra)
        assert open(out + ".rescued.tsv").read() == "\n".join(rescue.rows(ids, w, wl)) + "\n", (gpus, extra)
        for suffix in ("", ".stats", ".corrected.tsv"):
            assert open(out + suffix, "rb").read() == open(plain + suffix, "rb").read(), suffix
        line = "Rescued reads: %d eligible, %d rescued, %d ambiguous, %d truncated" % rescue.counts(recs, w)
        assert any(line in r.getMessage() for r in caplog.records), [r.getMessage() for r in caplog.records][-4:]


def test_stage1_run_checks_the_bit(tmp_path):
    """BDG_STAGE1_WL_RESCUE without the correction's bit is E_ARG; small chunks over three contexts write the file one context writes"""
    R = _real_set()
    n = 3300
    ids = ["read_%d" % i for i in range(n)]
    fq = str(tmp_path / "reads.fastq")
    with open(fq, "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in zip(ids, R["reads"][:n])))
    ctxs = [_native.Context(0) for _ in range(3)]
    for c in ctxs:
        c.whitelist_load(R["wl"])
    header = "#read_id\tbarcode\tUMI\tBC_score\tvalid_UMI\tstrand\tpolyT_start\tR1_end\twhitelist_barcode\twhitelist_dist\twhitelist_ties"
    kw = dict(threads=3, header_every=1000, chunk_reads=257, format_threads=3, whitelist=True, max_bc_dist=2)
    a, b = str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv")
    ra = _native.stage1_run(ctxs[:1], fq, a, header, rc.U, corrected_path=a + ".corr", rescued_path=a + ".resc", **kw)
    rb = _native.stage1_run(ctxs, fq, b, header, rc.U, corrected_path=b + ".corr", rescued_path=b + ".resc", **kw)
    assert open(a + ".resc", "rb").read() == open(b + ".resc", "rb").read() and open(a, "rb").read() == open(b, "rb").read()
    sup = rescue.exact_support(R["recs"][:n], R["reads"][:n], R["wl"])
    bases, off = synth.list_to_reads(R["reads"][:n])
    want = rescue.rescue_batch(bases, off, R["recs"][:n], rc.U, R["wl"], sup)
    assert open(a + ".resc").read() == "\n".join(rescue.rows(ids, want, R["wl"])) + "\n"
    cnt = rescue.counts(R["recs"][:n], want)
    for r in (ra, rb):
        assert (r.rescue_eligible, r.rescue_rescued, r.rescue_ambiguous, r.rescue_truncated) == cnt
    with pytest.raises(_native.BadgerHipError):
        _native.stage1_run(ctxs[:1], fq, a, header, rc.U, rescued_path=a + ".resc", **kw)          # no correction
    with pytest.raises(_native.BadgerHipError):
        _native.stage1_run(ctxs[:1], fq, a, header, rc.U, corrected_path=a + ".corr", rescued_path=a + ".resc", rescue_max_ed=3, **kw)
    for c in ctxs:
        c.close()
