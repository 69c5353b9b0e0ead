#!/usr/bin/env python3
"""Measurements of stage 2's --tagged_reads, one JSON line each to --out (and stdout).

    python tools/tagged_reads_probe.py --device [--reads 1000000,12500000] --out profiles/r13_tagged_reads.jsonl
        bdg_molecule_reps_dev alone on the workload of tools/umi_dedup_probe.py (its synthetic cells and UMIs, the molecules
        bdg_umi_dedup_dev makes of them, synthetic cDNA lengths), already on the device: wall time per call (after a warm-up,
        synchronised) and the per-kernel split from the library's event timers; then one molecule holding every read, with
        and without the wave aggregation.
    python tools/tagged_reads_probe.py --cli [--cli_reads 1000000] [--pairs 3] [--parent DIR] --out ...
        the stage-2 command line on a FASTQ file, as alternating pairs of fresh processes: with --tagged_reads (and with
        --chimera_cut --umi_dedup --molecule_reads) against this build without them; and, with --parent DIR (a built checkout
        of the parent commit), this build with the new flags off against the parent, beside parent against parent
        (--parent_flags: the same two pairs also without any flag and with all four).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from umi_dedup_probe import emit, synthetic  # noqa: E402


def _timed(ctx, call, reps):
    call()
    ctx.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        times.append(time.perf_counter() - t0)
    ctx.profile(True)
    ctx.profile_reset()
    call()
    ctx.synchronize()
    kt = {k: round(v[1], 4) for k, v in ctx.profile_read().items() if k.startswith("k_mol")}
    ctx.profile(False)
    return times, kt


def device_probe(args):
    from badger_amd import _native
    _native.PRELOAD_TORCH = False
    ctx = _native.default_context(0)
    for n in [int(x) for x in args.reads.split(",")]:
        cells, rank, has, umi = synthetic(n)
        rng = np.random.default_rng(2)
        length = rng.integers(50, 1500, n).astype(np.uint32)
        length[rng.random(n) < 0.1] = 0
        d = [_native.DeviceArray.from_host(ctx, a) for a in (cells, rank, has, umi, length)]
        d_mol = _native.DeviceArray(ctx, n, np.uint32)
        d_cnt = _native.DeviceArray(ctx, (len(cells), 4), np.uint32)
        ctx.umi_dedup_dev(d[1], d[2], d[3], n, d[0], len(cells), 12, 1, d_mol, d_cnt)
        molecules = int(d_cnt.to_host()[:, 3].sum())
        d_rep, d_reads = _native.DeviceArray(ctx, n, np.uint8), _native.DeviceArray(ctx, n, np.uint32)
        for aggregate in (True, False):
            ctx.molecule_reps_set_aggregate(aggregate)
            times, kt = _timed(ctx, lambda: ctx.molecule_reps_dev(d[1], d[2], d_mol, d[4], n, d[0], len(cells), d_rep, d_reads), args.reps)
            emit(args.out, {"what": "bdg_molecule_reps_dev", "reads": n, "cells": int(len(cells)), "molecules": molecules,
                            "representatives": int(d_rep.to_host().sum()), "wave_aggregation": aggregate,
                            "ms_median": round(1e3 * float(np.median(times)), 4), "ms_min": round(1e3 * min(times), 4),
                            "ms_per_1M_reads": round(1e3 * float(np.median(times)) * 1e6 / n, 4), "kernel_ms": kt})
        ctx.molecule_reps_set_aggregate(True)
        for a in d + [d_mol, d_cnt, d_rep, d_reads]:
            a.free()
    # one molecule holding every read: one address
    n = args.one_hot_reads
    rng = np.random.default_rng(3)
    cells = np.array([77], dtype=np.uint32)
    arrays = (cells, np.full(n, 77, np.uint32), np.ones(n, np.uint8), np.full(n, 12 << 28 | 0x1B1B1B, np.uint32),
              rng.integers(0, 1500, n).astype(np.uint32))
    d = [_native.DeviceArray.from_host(ctx, a) for a in arrays]
    d_rep, d_reads = _native.DeviceArray(ctx, n, np.uint8), _native.DeviceArray(ctx, n, np.uint32)
    for aggregate in (True, False):
        ctx.molecule_reps_set_aggregate(aggregate)
        times, kt = _timed(ctx, lambda: ctx.molecule_reps_dev(d[1], d[2], d[3], d[4], n, d[0], 1, d_rep, d_reads), args.reps)
        assert int(d_rep.to_host().sum()) == 1 and int(d_reads.to_host()[0]) == n
        emit(args.out, {"what": "bdg_molecule_reps_dev, one molecule holds every read", "reads": n, "wave_aggregation": aggregate,
                        "ms_median": round(1e3 * float(np.median(times)), 4), "ms_min": round(1e3 * min(times), 4), "kernel_ms": kt})
    ctx.molecule_reps_set_aggregate(True)
    for a in d + [d_rep, d_reads]:
        a.free()


def _fastq(n, tmp):
    """n reads of the error model with a TSO, 5,000 cells -> FASTQ path, whitelist path"""
    import torch  # noqa: F401  (synth.make_reads on the device)
    from cli_throughput import helper
    from badger_amd import synth
    L = helper(tmp)
    wl = synth.make_whitelist(6000)
    with open(os.path.join(tmp, "wl.txt"), "w") as f:
        f.write("\n".join(synth.rank_to_str(int(r)) for r in wl) + "\n")
    fq = os.path.join(tmp, "reads.fastq")
    done = 0
    while done < n:
        k = min(500000, n - done)
        tb, to = synth.make_reads(k, wl, seed=1 + done // 500000, device="cuda", tso=True)
        bases, off = tb.cpu().numpy(), to.cpu().numpy().astype(np.uint64)
        assert L.fq_append(fq.encode(), bases.ctypes.data, off.ctypes.data, k, done, b"read_") > 0
        done += k
    return fq, os.path.join(tmp, "wl.txt")


def cli_probe(args):
    tmp = tempfile.mkdtemp(prefix="tagged_probe_")
    fq, wl = _fastq(args.cli_reads, tmp)
    args_of = lambda out: ["-m", "badger_amd.badger", "-r", fq, "-d", "tenX_v3", "-l", wl, "-c", "5000", "-tr", "4", "-o", os.path.join(tmp, out)]  # noqa: E731

    def run(cwd, out, extra):
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable] + args_of(out) + extra, cwd=cwd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(r.stdout[-2000:] + r.stderr[-2000:])
        return time.perf_counter() - t0

    def pairs(name_a, a, name_b, b, what):
        walls = {name_a: [], name_b: []}
        for _ in range(args.pairs):
            for name, (cwd, extra) in ((name_a, a), (name_b, b)):
                walls[name].append(run(cwd, name.replace(" ", "_"), extra))
        ma, mb = float(np.median(walls[name_a])), float(np.median(walls[name_b]))
        emit(args.out, {"what": what, "reads": args.cli_reads, "pairs": args.pairs, "fastq_bytes": os.path.getsize(fq),
                        name_a + "_s": [round(x, 3) for x in walls[name_a]], name_b + "_s": [round(x, 3) for x in walls[name_b]],
                        "median_" + name_a + "_s": round(ma, 3), "median_" + name_b + "_s": round(mb, 3),
                        "ratio_%s_over_%s" % (name_b, name_a): round(mb / ma, 3)})

    run(ROOT, "warm", [])                                            # (the file into the page cache, the runtime's caches)
    fa = os.path.join(tmp, "tagged.fa")
    pairs("plain", (ROOT, []), "tagged", (ROOT, ["--tagged_reads", fa]), "stage2 CLI from FASTQ: --tagged_reads against none")
    pairs("umi_dedup", (ROOT, ["--umi_dedup"]), "tagged_molecules", (ROOT, ["--umi_dedup", "--tagged_reads", fa, "--chimera_cut", "--molecule_reads"]),
          "stage2 CLI from FASTQ: --umi_dedup --tagged_reads --chimera_cut --molecule_reads against --umi_dedup")
    if args.parent:
        parent = os.path.abspath(args.parent)
        pairs("parent", (parent, ["--umi_dedup"]), "flags_off", (ROOT, ["--umi_dedup"]), "stage2 CLI from FASTQ, --umi_dedup: this build with the new flags off against the parent commit's")
        pairs("parent_a", (parent, ["--umi_dedup"]), "parent_b", (parent, ["--umi_dedup"]), "stage2 CLI from FASTQ, --umi_dedup: the parent commit's build against itself")
        if args.parent_flags:                                        # (a change that should move nothing: the same flags on both sides)
            for label, extra in (("no flags", []), ("--umi_dedup --tagged_reads --chimera_cut --molecule_reads",
                                                    ["--umi_dedup", "--tagged_reads", fa, "--chimera_cut", "--molecule_reads"])):
                pairs("parent", (parent, extra), "this", (ROOT, extra), "stage2 CLI from FASTQ, %s: this build against the parent commit's" % label)
                pairs("parent_a", (parent, extra), "parent_b", (parent, extra), "stage2 CLI from FASTQ, %s: the parent commit's build against itself" % label)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--device", action="store_true")
    p.add_argument("--cli", action="store_true")
    p.add_argument("--reads", default="1000000,12500000")
    p.add_argument("--one_hot_reads", type=int, default=1000000)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--cli_reads", type=int, default=1000000)
    p.add_argument("--pairs", type=int, default=3)
    p.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    p.add_argument("--parent_flags", action="store_true", help="with --parent: the pairs also without flags and with all of them")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.device:
        device_probe(args)
    if args.cli:
        cli_probe(args)


if __name__ == "__main__":
    main()
