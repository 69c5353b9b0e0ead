#!/usr/bin/env python3
"""Measurements of the barcode rescue, one JSON line each to --out (and stdout).

    python tools/rescue_probe.py --model --out profiles/r17_rescue.jsonl
        no GPU: badger_amd/rescue.py over rescue.cut_read_set - reads of synth.make_reads with the first 40 bases cut off, as
        many reads of random bases with a planted tail, beside the whole reads whose exact hits are the support (records from
        the CPU oracle).  Per max_ed 0 .. 2 and min_support 1, 2, 5: the share of cut reads rescued to the right cell, to a
        wrong one, and the share of random reads rescued.
    python tools/rescue_probe.py --device [--reads 1000000] [--distinct 100000] --out ...
        synth.make_reads reads, a third of them cut, device-resident: the extraction step (bdg_extract_batch_dev) and the rescue
        behind it (bdg_rescue_batch_dev: windows, match, resolve, and its wait), 3 warm-ups and --reps timed calls, median; then
        k_rescue_windows and k_rescue_resolve alone from the library's per-kernel timers, one kernel timed per pass.
    python tools/rescue_probe.py --cli [--parent DIR] [--cli_reads 2000000] [--pairs 5] --out ...
        the stage-1 command line on a FASTQ with -b --bc_correct --bc_rescue against -b --bc_correct on this tree, alternating
        pairs of fresh processes; with --parent DIR (a built checkout of the parent commit) also the flag-off run against the
        parent's, beside the parent's own pair-to-pair spread.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def model_probe(args):
    from badger_amd import rescue, synth
    from oracle import pyoracle as orc
    wl = synth.make_whitelist(args.model_whitelist)
    n_cut = args.model_cut
    reads, kind, bc = rescue.cut_read_set(args.model_whole, n_cut, n_cut, wl, args.seed, args.model_cells)
    b, o = synth.list_to_reads(reads)
    recs = orc.extract_batch(b, o, 12, threads=8)
    sup = rescue.exact_support(recs, reads, wl)
    m = rescue.Matcher(wl)
    elig = np.array([rescue.eligible(r) for r in recs])
    table = []
    for D in range(rescue.MAX_ED_MAX + 1):
        for M in (1, 2, 5):
            r = rescue.rescue_batch(b, o, recs, 12, wl, sup, D, M, matcher=m)
            res = r[r["status"] == rescue.RESCUED]
            k = kind[res["read"]]
            right = wl[res["entry"]].astype(np.int64) == bc[res["read"]]
            table.append({"max_ed": D, "min_support": M, "cut_right": int((right & (k == 1)).sum()), "cut_wrong": int((~right & (k == 1)).sum()),
                          "random_rescued": int((k == 2).sum()), "whole_without_barcode_right": int((right & (k == 0)).sum()),
                          "whole_without_barcode_wrong": int((~right & (k == 0)).sum()),
                          "ambiguous": int((r["status"] == rescue.AMBIGUOUS).sum()), "truncated": int((r["status"] == rescue.TRUNCATED).sum())})
    emit(args.out, {"what": "rescue.py over cut reads, random reads with a planted tail and the whole reads that give the support",
                    "whitelist": len(wl), "cells": args.model_cells, "whole_reads": args.model_whole, "cut_reads": n_cut, "random_reads": n_cut,
                    "error_rate": "sub 3 % ins 2 % del 3 % (synth.make_reads)", "seed": args.seed, "exact_hits": int(sup.sum()),
                    "entries_with_support_2": int((sup >= 2).sum()), "cut_eligible": int(elig[kind == 1].sum()),
                    "random_eligible": int(elig[kind == 2].sum()), "whole_eligible": int(elig[kind == 0].sum()), "table": table, "gpu": "not used"})


def device_probe(args):
    import torch
    from badger_amd import _native, rescue, synth
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    ctx.set_stream(0)
    wl = synth.make_whitelist(100000)
    ctx.whitelist_load(wl)
    reads, _, _ = rescue.cut_read_set(args.distinct - args.distinct // 3, args.distinct // 3, 0, wl, args.seed, 5000)
    hb, ho = synth.list_to_reads(reads)
    rep = (args.reads + args.distinct - 1) // args.distinct
    lens = np.tile(np.diff(ho.astype(np.int64)), rep)[:args.reads]
    n = len(lens)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    d_bases = torch.zeros((total + 15) // 16 * 16 + 64, dtype=torch.uint8, device=dev)
    d_bases[:total] = torch.from_numpy(np.tile(hb, rep)[:total]).to(dev)
    o = torch.from_numpy(off).to(dev)
    d_recs = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
    ctx.extract_batch_dev(d_bases, o, n, total, 12, d_recs)
    assert ctx.extract_status()[0] == 0
    recs = d_recs.cpu().numpy().view(_native.REC_DTYPE)
    sup = rescue.exact_support(recs[:args.distinct], reads, wl) * rep
    d_sup = torch.from_numpy(sup.astype(np.int32)).to(dev)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    ext = timed(lambda: ctx.extract_batch_dev(d_bases, o, n, total, 12, d_recs))
    stored = [0]

    def run_rescue():
        stored[0] = ctx.rescue_batch_dev(d_bases, o, n, d_recs, 12, d_sup, rescue.MAX_ED_DEFAULT, rescue.MIN_SUPPORT_DEFAULT, d_out)

    rs = timed(run_rescue)
    per = {}
    ctx.profile(True)
    for kernel in ("k_rescue_windows", "k_rescue_resolve", "k_nearest_pairs_topk"):
        ctx.profile_only(kernel)
        ctx.profile_reset()
        for _ in range(args.reps):
            run_rescue()
        launches, ms = ctx.profile_read()[kernel]
        per[kernel] = round(ms / args.reps, 4)                            # per call: the sum over the pieces of the store
    ctx.profile_only(None)
    ctx.profile(False)
    res = d_out.cpu().numpy()[:stored[0] * 40].view(_native.RESCUE_DTYPE)
    counts = ctx.rescue_counts()
    # the pipelined form: chunks of 100,000 reads through submit / collect, k_rescue_windows with p from the scan's array
    h_bases = np.tile(hb, rep)[:total]
    h_off = off.astype(np.uint64)
    ctx.extract_set_rescue(True)
    ctx.profile(True)
    ctx.profile_only("k_rescue_windows")
    ctx.profile_reset()
    flying = []
    for k, a in enumerate(range(0, n, 100000)):
        b = min(a + 100000, n)
        if len(flying) >= 2:
            slot, m, _ = flying.pop(0)
            ctx.extract_collect(slot, m)
        oo = np.ascontiguousarray(h_off[a:b + 1])
        ctx.extract_submit(k % 4, h_bases.ctypes.data, oo.ctypes.data, b - a, 12)
        flying.append((k % 4, b - a, oo))
    for slot, m, _ in flying:
        ctx.extract_collect(slot, m)
    launches, pipe_ms = ctx.profile_read()["k_rescue_windows"]
    ctx.profile_only(None)
    ctx.profile(False)
    t0 = time.perf_counter()
    piped = ctx.extract_rescue_resolve(d_sup, rescue.MAX_ED_DEFAULT, rescue.MIN_SUPPORT_DEFAULT)
    resolve_wall = time.perf_counter() - t0
    pipe_counts = ctx.rescue_counts()
    ctx.extract_set_rescue(False)
    emit(args.out, {"what": "rescue, device-resident: the extraction step, and bdg_rescue_batch_dev behind it (device events around the whole call, its "
                            "host waits included; p recomputed from the bases), the kernels alone per call (library timers)",
                    "reads": n, "distinct_reads": args.distinct, "bases": total, "eligible": counts[1], "stored": stored[0],
                    "pipelined": {"chunks": launches, "k_rescue_windows_ms_total": round(pipe_ms, 4), "stored": pipe_counts[0], "eligible": pipe_counts[1],
                                  "same_records_as_one_call": bool(len(piped) == len(res) and (piped == res[np.argsort(res["read"])]).all()),
                                  "match_and_resolve_wall_ms": round(1000 * resolve_wall, 3)},
                    "rescued": int((res["status"] == 1).sum()), "ambiguous": int((res["status"] == 2).sum()), "truncated": int((res["status"] == 3).sum()),
                    "extract_ms_median": round(float(np.median(ext)), 4), "extract_ms_min": round(min(ext), 4), "extract_ms_max": round(max(ext), 4),
                    "rescue_ms_median": round(float(np.median(rs)), 4), "rescue_ms_min": round(min(rs), 4), "rescue_ms_max": round(max(rs), 4),
                    "kernel_ms_per_call": per, "warmups": 3, "timed": args.reps, "version": ctx.lib.bdg_version().decode()})


def cli_probe(args):
    from badger_amd import common, rescue, synth
    tmp = tempfile.mkdtemp(prefix="rescue_probe_", dir=os.environ.get("TMPDIR", "/tmp"))
    n = args.cli_reads
    wl = synth.make_whitelist(737280)
    wl_path = os.path.join(tmp, "wl.txt")
    with open(wl_path, "w") as f:
        f.write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    fq = os.path.join(tmp, "reads.fastq")
    with open(fq, "wb") as f:
        done = 0
        while done < n:
            k = min(250000, n - done)
            reads, _, _ = rescue.cut_read_set(k - k // 3, k // 3, 0, wl, 1 + done // 250000, 5000)
            f.write(b"".join(b"@read_%d\n%s\n+\n%s\n" % (done + i, s.encode(), b"I" * len(s)) for i, s in enumerate(reads)))
            done += k
    base = [sys.executable, "-m", "badger_amd.extract_raw_barcodes", "--mode", "tenX_v3", "-i", fq, "-t", "16", "-b", wl_path, "--bc_correct"]
    runs = {"correct": (ROOT, []), "rescue": (ROOT, ["--bc_rescue"])}
    if args.parent:
        if not os.path.exists(os.path.join(args.parent, "badger_amd", "libbadger_hip.so")):
            raise SystemExit("--parent DIR: a checkout of the parent commit with its library built")
        runs["parent"] = (args.parent, [])
    cmd = lambda name: base + ["-o", os.path.join(tmp, name + ".tsv")] + runs[name][1]                  # noqa: E731
    walls = {name: [] for name in runs}
    for name in runs:                                                                                  # (page cache, clocks)
        subprocess.run(cmd(name), cwd=runs[name][0], capture_output=True, text=True, timeout=900)
    for _ in range(args.pairs):
        for name in runs:
            t0 = time.perf_counter()
            r = subprocess.run(cmd(name), cwd=runs[name][0], capture_output=True, text=True, timeout=900)
            walls[name].append(time.perf_counter() - t0)
            if r.returncode != 0:
                raise SystemExit(r.stderr[-2000:] + r.stdout[-2000:])
    same = all(open(os.path.join(tmp, "correct.tsv" + s), "rb").read() == open(os.path.join(tmp, "rescue.tsv" + s), "rb").read()
               for s in ("", ".stats", ".corrected.tsv"))
    rows = open(os.path.join(tmp, "rescue.tsv.rescued.tsv")).read().split("\n")[1:-1]
    diff = [b - a for a, b in zip(walls["correct"], walls["rescue"])]
    rec = {"what": "stage-1 CLI -b --bc_correct --bc_rescue against -b --bc_correct on this tree, alternating pairs of fresh processes",
           "reads": n, "cut_reads": n // 3, "pairs": args.pairs, "fastq_bytes": os.path.getsize(fq), "same_other_outputs": same,
           "rescued_rows": len(rows), "rescued": sum(1 for r in rows if r.endswith("\trescued")),
           "correct_s": [round(x, 3) for x in walls["correct"]], "rescue_s": [round(x, 3) for x in walls["rescue"]],
           "median_correct_s": round(float(np.median(walls["correct"])), 3), "median_rescue_s": round(float(np.median(walls["rescue"])), 3),
           "median_paired_difference_s": round(float(np.median(diff)), 3),
           "correct_pair_to_pair_spread_s": round(max(walls["correct"]) - min(walls["correct"]), 3)}
    if args.parent:
        d2 = [b - a for a, b in zip(walls["parent"], walls["correct"])]
        spread = max(walls["parent"]) - min(walls["parent"])
        rec.update({"parent_s": [round(x, 3) for x in walls["parent"]], "median_parent_s": round(float(np.median(walls["parent"])), 3),
                    "flag_off_median_paired_difference_to_parent_s": round(float(np.median(d2)), 3), "parent_pair_to_pair_spread_s": round(spread, 3),
                    "flag_off_inside_parent_spread": bool(abs(float(np.median(d2))) <= spread),
                    "flag_off_same_bytes_as_parent": open(os.path.join(tmp, "parent.tsv"), "rb").read() == open(os.path.join(tmp, "correct.tsv"), "rb").read()})
    emit(args.out, rec)
    for p in os.listdir(tmp):
        os.remove(os.path.join(tmp, p))
    os.rmdir(tmp)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", action="store_true")
    p.add_argument("--device", action="store_true")
    p.add_argument("--cli", action="store_true")
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--model_whitelist", type=int, default=6000)
    p.add_argument("--model_cells", type=int, default=3000)
    p.add_argument("--model_whole", type=int, default=30000)
    p.add_argument("--model_cut", type=int, default=2000)
    p.add_argument("--reads", type=int, default=1000000)
    p.add_argument("--distinct", type=int, default=100000)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--cli_reads", type=int, default=2000000)
    p.add_argument("--pairs", type=int, default=5)
    p.add_argument("--parent", default=None)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.model:
        model_probe(args)
    if args.device:
        device_probe(args)
    if args.cli:
        cli_probe(args)


if __name__ == "__main__":
    main()
