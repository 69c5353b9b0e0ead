#!/usr/bin/env python3
"""Measurements of stage 2's --umi_dedup, one JSON line each to --out (and stdout).

    python tools/umi_dedup_probe.py --device [--reads 1000000,12500000] --out profiles/r09_umi_dedup.jsonl
        bdg_umi_dedup_dev alone on synthetic per-read cells and UMIs already on the device: wall time per call (after a
        warm-up, synchronised) and the per-kernel split from the library's event timers.
    python tools/umi_dedup_probe.py --cli [--cli_reads 1000000] [--pairs 5] --out ...
        the stage-2 command line on a stage-1 TSV with and without --umi_dedup, as alternating pairs of fresh processes:
        median wall clock of each and the ratio.
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


def synthetic(n, n_cells=5000, seed=1):
    """per read: cell rank, has, UMI code; molecules of about five reads, one read in ten with one substitution"""
    rng = np.random.default_rng(seed)
    cells = np.unique(rng.integers(0, 1 << 32, n_cells, dtype=np.uint64).astype(np.uint32))
    w = np.exp(rng.standard_normal(len(cells)))
    n_mol = max(1, n // 5)
    mol = rng.integers(0, n_mol, n)
    cell = rng.choice(len(cells), n_mol, p=w / w.sum())[mol]          # (a molecule lives in one cell)
    letters = (mol.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)
    letters = letters.astype(np.uint32) & np.uint32(0xFFFFFF)
    err = rng.random(n) < 0.1
    pos = rng.integers(0, 12, n).astype(np.uint32)
    letters = np.where(err, letters ^ (np.uint32(1) << (2 * pos)), letters).astype(np.uint32)
    umi = (np.uint32(12) << np.uint32(28)) | letters
    has = (rng.random(n) < 0.95).astype(np.uint8)
    return cells, cells[cell].astype(np.uint32), has, umi.astype(np.uint32)


def device_probe(args):
    from badger_amd import _native
    _native.PRELOAD_TORCH = False
    ctx = _native.default_context(0)
    for n in [int(x) for x in args.reads.split(",")]:
        cells, rank, has, umi = synthetic(n)
        d = [_native.DeviceArray.from_host(ctx, a) for a in (cells, rank, has, umi)]
        d_mol = _native.DeviceArray(ctx, n, np.uint32)
        d_cnt = _native.DeviceArray(ctx, (len(cells), 4), np.uint32)
        for dist in (1, 0):
            call = lambda: ctx.umi_dedup_dev(d[1], d[2], d[3], n, d[0], len(cells), 12, dist, d_mol, d_cnt)
            call()
            ctx.synchronize()
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                call()
                ctx.synchronize()
                times.append(time.perf_counter() - t0)
            ctx.profile(True)
            ctx.profile_reset()
            call()
            ctx.synchronize()
            kt = {k: round(v[1], 4) for k, v in ctx.profile_read().items() if k.startswith("k_umi")}
            ctx.profile(False)
            cnt = d_cnt.to_host()
            emit(args.out, {"what": "bdg_umi_dedup_dev", "reads": n, "umi_dist": dist, "cells": int(len(cells)),
                            "umis": int(cnt[:, 2].sum()), "molecules": int(cnt[:, 3].sum()),
                            "ms_median": round(1e3 * float(np.median(times)), 4), "ms_min": round(1e3 * min(times), 4),
                            "ms_per_1M_reads": round(1e3 * float(np.median(times)) * 1e6 / n, 4), "kernel_ms": kt})
        for a in d + [d_mol, d_cnt]:
            a.free()


def cli_probe(args):
    from badger_amd import synth
    tmp = tempfile.mkdtemp(prefix="umi_probe_")
    n = args.cli_reads
    rng = np.random.default_rng(3)
    wl = synth.make_whitelist(6000)
    wl_s = [synth.rank_to_str(int(r)) for r in wl]
    with open(os.path.join(tmp, "wl.txt"), "w") as f:
        f.write("\n".join(wl_s) + "\n")
    mol = rng.integers(0, n // 5, n)
    cell = rng.choice(5000, n // 5, p=(lambda w: w / w.sum())(np.exp(rng.standard_normal(5000))))[mol]
    acgt = np.frombuffer(b"ACGT", np.uint8)
    umi_l = acgt[(((mol[:, None].astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> (np.uint64(2) * np.arange(12, dtype=np.uint64) + np.uint64(20)))
                  & np.uint64(3)).astype(np.intp)]
    sub = rng.random(n) < 0.1
    umi_l[sub, rng.integers(0, 12, int(sub.sum()))] = acgt[rng.integers(0, 4, int(sub.sum()))]
    tsv = os.path.join(tmp, "s1.tsv")
    with open(tsv, "w") as f:
        f.write("#read_id\tbarcode\tUMI\tBC_score\tvalid_UMI\tstrand\tpolyT_start\tR1_end\n")
        umis = umi_l.view("S12").ravel()
        f.write("".join("read_%d\t%s\t%s\t0\tFalse\t+\t60\t22\n" % (i, wl_s[c], u.decode()) for i, (c, u) in enumerate(zip(cell, umis))))
    base = [sys.executable, "-m", "badger_amd.badger", "-r", tsv, "-d", "tenX_v3", "-l", os.path.join(tmp, "wl.txt"), "-c", "5000",
            "-o", os.path.join(tmp, "o")]
    walls = {"plain": [], "umi_dedup": []}
    for _ in range(args.pairs):
        for name, extra in (("plain", []), ("umi_dedup", ["--umi_dedup"])):
            t0 = time.perf_counter()
            r = subprocess.run(base + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
            walls[name].append(time.perf_counter() - t0)
            if r.returncode != 0:
                raise SystemExit(r.stderr[-2000:])
    mp, mu = float(np.median(walls["plain"])), float(np.median(walls["umi_dedup"]))
    emit(args.out, {"what": "stage2 CLI from TSV, alternating pairs", "reads": n, "pairs": args.pairs,
                    "plain_s": [round(x, 3) for x in walls["plain"]], "umi_dedup_s": [round(x, 3) for x in walls["umi_dedup"]],
                    "median_plain_s": round(mp, 3), "median_umi_dedup_s": round(mu, 3), "ratio": round(mu / mp, 3)})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--device", action="store_true")
    p.add_argument("--cli", action="store_true")
    p.add_argument("--reads", default="1000000,12500000")
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--cli_reads", type=int, default=1000000)
    p.add_argument("--pairs", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.device:
        device_probe(args)
    if args.cli:
        cli_probe(args)


if __name__ == "__main__":
    main()
