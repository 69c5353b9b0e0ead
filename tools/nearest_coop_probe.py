#!/usr/bin/env python3
"""Measurements of the wave-cooperative nearest-whitelist kernel (bdg_nearest16_set_algo 3), one JSON object per line:

  kernel     nq queries x the 737,280-entry list, exhaustive (max_ed 3): forced scan (algo 1) vs forced cooperative kernel
             (algo 3), device time from the library's per-kernel event timers, answers compared between the two
  overflow   the probe path (max_ed 2) on 100,000 queries + H queries planted to overflow pass 2's hit lists, lists of 737 K and
             4.9 M entries: the time of the overflow step (k_nearest_coop_overflow), of the same step with nothing planted (the
             list empty: a launch and nothing more), and what the old kernel (k_nearest_scan, one query per lane) takes for the
             planted queries; answers compared with the cooperative kernel's
  cli        the stage-1 command line on N synthetic FASTQ reads, without and with -b (737 K list), process start to TSV on disk

Builder tool (the numbers go to DESIGN.md / README.md / profiles/), not the bench contract.

    python tools/nearest_coop_probe.py [--cli-reads N] [--skip-cli]
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from badger_amd import _native, common, synth  # noqa: E402


def queries(wl, n, seed):
    """half near a whitelist entry (up to three substitutions), half uniform: what read barcodes look like to the match"""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    base = wl[rng.integers(0, len(wl), size=n)]
    for _ in range(3):
        pos = rng.integers(0, 16, size=n).astype(np.uint32)
        sub = rng.integers(0, 4, size=n).astype(np.uint32)
        base = np.where(rng.random(n) < 0.5, (base & ~(np.uint32(3) << (2 * pos))) | (sub << (2 * pos)), base).astype(np.uint32)
    return np.where(rng.random(n) < 0.5, base, q).astype(np.uint32)


def planted(rng, n):
    """n queries, each with > 4 entries one deletion + one insertion away behind one lane's deletion variants (and none within
    Hamming distance 2): every one of them overflows pass 2 of the probe path"""
    heavy = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    ents = set()
    for qv in heavy.tolist():
        s = common.unrank(qv, 16)
        for i in range(4):
            d = s[:i] + s[i + 1:]
            for p in range(11, 16):
                for b in "ACGT":
                    e = d[:p] + b + d[p:]
                    if sum(x != y for x, y in zip(e, s)) > 2:
                        ents.add(common.rank(e, 16))
    return heavy, np.array(sorted(ents), dtype=np.uint32)


def timed(ctx, d_q, nq, max_ed, outs, kernel, reps):
    ctx.profile(True)
    ctx.profile_only(None)
    ctx.nearest16_dev(d_q, nq, max_ed, *outs)                    # warm: plan, workspace
    ctx.profile_reset()
    for _ in range(reps):
        ctx.nearest16_dev(d_q, nq, max_ed, *outs)
    prof = ctx.profile_read()
    ctx.profile(False)
    launches, ms = prof.get(kernel, (0, 0.0))
    return ms / max(launches, 1), prof


def dev_arrays(ctx, q):
    d_q = _native.DeviceArray.from_host(ctx, q)
    n = len(q)
    outs = (_native.DeviceArray(ctx, (n,), np.uint32), _native.DeviceArray(ctx, (n,), np.uint8), _native.DeviceArray(ctx, (n,), np.uint16))
    return d_q, outs


def kernel_part(ctx):
    wl = synth.make_whitelist(737280)
    ctx.whitelist_load(wl)
    for nq in (1, 64, 512, 2048, 4096, 5000, 8192, 16384, 32768, 65536):
        q = queries(wl, nq, nq)
        d_q, outs = dev_arrays(ctx, q)
        row = {"part": "kernel", "nq": nq, "nw": len(wl), "max_ed": 3}
        answers = {}
        for algo, kname in ((1, "k_nearest_scan"), (3, "k_nearest_coop")):
            ctx.nearest16_set_algo(algo)
            reps = 3 if nq * len(wl) > 5e9 else 10
            ms, _ = timed(ctx, d_q, nq, 3, outs, kname, reps)
            answers[algo] = [o.to_host() for o in outs]
            row[kname + "_ms"] = round(ms, 4)
            row[kname + "_Gpairs_per_s"] = round(nq * len(wl) / (ms * 1e-3) / 1e9, 1) if ms else None
        row["equal"] = all((a == b).all() for a, b in zip(answers[1], answers[3]))
        ctx.nearest16_set_algo(0)
        print(json.dumps(row), flush=True)
        for a in (d_q,) + outs:
            a.free()


def overflow_part(ctx):
    rng = np.random.default_rng(7)
    for nw in (737280, 4900000):
        heavy, ents = planted(rng, 64)
        base = synth.make_whitelist(nw)
        wl = np.unique(np.concatenate([base, ents])).astype(np.uint32)
        wl = wl[rng.permutation(len(wl))]
        ctx.whitelist_load(wl)
        q0 = queries(wl, 100000, 5)
        for label, q in (("none planted", q0), ("64 planted", np.concatenate([q0, heavy]).astype(np.uint32))):
            d_q, outs = dev_arrays(ctx, q)
            ctx.nearest16_set_algo(2)
            ms, prof = timed(ctx, d_q, len(q), 2, outs, "k_nearest_coop_overflow", 5)
            probe = [o.to_host() for o in outs]
            row = {"part": "overflow", "nw": len(wl), "nq": len(q), "queries": label,
                   "k_nearest_coop_overflow_ms": round(ms, 4),
                   "probe_step_ms": round(sum(v[1] / max(v[0], 1) for k, v in prof.items() if k.startswith("k_nearest") and v[0]), 4)}
            # the cooperative kernel's answers for the planted queries and a sample: the probe path's must equal them
            sel = np.concatenate([np.arange(2000), np.arange(len(q0), len(q))])
            ctx.nearest16_set_algo(3)
            got = ctx.nearest16(q[sel], wl, 2)
            row["equal_on_sample"] = all((g == p[sel]).all() for g, p in zip(got, probe))
            if label != "none planted":
                # the old overflow step: k_nearest_scan over just those queries (one query per lane, one block)
                ctx.nearest16_set_algo(1)
                d_h, outs_h = dev_arrays(ctx, heavy)
                ms_old, _ = timed(ctx, d_h, len(heavy), 2, outs_h, "k_nearest_scan", 2)
                row["old_k_nearest_scan_on_planted_ms"] = round(ms_old, 3)
                row["coop_per_planted_query_us_upper_bound"] = round(1e3 * ms / len(heavy), 2)
                for a in (d_h,) + outs_h:
                    a.free()
            ctx.nearest16_set_algo(0)
            print(json.dumps(row), flush=True)
            for a in (d_q,) + outs:
                a.free()


def cli_part(n):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import cli_throughput as ct
    tmp = os.environ.get("TMPDIR", "/tmp")
    L = ct.helper(tmp)
    wl = synth.make_whitelist(737280)
    wl_path = os.path.join(tmp, "wl737k.txt")
    with open(wl_path, "w") as f:
        f.write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    fq = os.path.join(tmp, "coop_cli_reads.fastq")
    if os.path.exists(fq):
        os.remove(fq)
    done = 0
    while done < n:
        k = min(ct.SLAB, n - done)
        tb, to = synth.make_reads(k, wl, seed=1 + done // ct.SLAB, device="cuda")
        bases, off = tb.cpu().numpy(), to.cpu().numpy().astype(np.uint64)
        assert L.fq_append(fq.encode(), bases.ctypes.data, off.ctypes.data, k, done, b"read_") > 0
        done += k
    timing = os.path.join(tmp, "coop_cli_timing.jsonl")
    out = os.path.join(tmp, "coop_cli_out.tsv")
    for rep in range(2):                                      # alternating, twice: the spread shows in the pairs
        for extra in ((), ("-b", wl_path)):
            wall, br = ct.run_cli(fq, out, 16, timing, extra)
            rows = sum(1 for _ in open(out, "rb"))
            wlcount = open(out + ".stats").read().strip().split("\n")[-1]
            print(json.dumps({"part": "cli", "reads": n, "rep": rep, "barcodes_flag": bool(extra), "wall_s": round(wall, 3),
                              "lines": rows, "last_stats_line": wlcount, "pipeline": br}), flush=True)
    for p in (fq, out, out + ".stats"):
        if os.path.exists(p):
            os.remove(p)


def main():
    args = sys.argv[1:]
    n_cli = int(args[args.index("--cli-reads") + 1]) if "--cli-reads" in args else 4000000
    print(json.dumps({"version": _native.load().bdg_version().decode()}), flush=True)
    ctx = _native.Context(0)
    t0 = time.perf_counter()
    kernel_part(ctx)
    overflow_part(ctx)
    ctx.close()
    if "--skip-cli" not in args:
        cli_part(n_cli)
    print(json.dumps({"done_s": round(time.perf_counter() - t0, 1)}), flush=True)


if __name__ == "__main__":
    main()
