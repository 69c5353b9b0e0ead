#!/usr/bin/env python3
"""Measurements of --umi_per_gene, one JSON line each to --out (and stdout).

    python tools/umi_gene_probe.py --device [--reads 1000000,12500000] --out profiles/r25_umi_per_gene.jsonl
        bdg_umi_dedup_genes_dev beside bdg_umi_dedup_dev on the workload of tools/umi_dedup_probe.py (its synthetic cells and
        UMIs already on the device; every molecule is given a gene drawn from 2,000, one read in twenty no gene): wall time per
        call (after a warm-up, synchronised, median of --reps) and the per-kernel split from the library's event timers, both
        calls in the same run; then one hot group holding every read, with and without the aggregation inside the wave.
    python tools/umi_gene_probe.py --dist 2 [--reads 1000000,12500000] [--reps 3] --out profiles/r26_umi_dist2.jsonl
        k_umi_parent2 beside k_umi_parent on the same workload in one run: bdg_umi_dedup_genes_dev and
        bdg_umi_dedup_dev at umi_dist 1 and, behind bdg_umi_set_max_dist(2), at umi_dist 2 - wall time per call, the two parent
        kernels' times from the library's event timers, and the molecules each distance finds.
    python tools/umi_gene_probe.py --cli --dist 2 [--pairs 3] [--parent DIR] --out profiles/r26_umi_dist2.jsonl
        the --cli pairs below with --umi_per_gene on every side: --gene_umi_dist2 against without, and with --parent this
        build without the flag against the parent's, and the parent's against itself.
    python tools/umi_gene_probe.py --cli [--cli_reads 1000000] [--pairs 3] [--parent DIR] --out ...
        the stage-2 command line from FASTQ with --umi_dedup --tagged_reads --count_matrix, as alternating pairs of fresh
        processes: with --umi_per_gene against without; and, with --parent DIR (a built checkout of the parent commit), this
        build with the flag off against the parent's, and the parent's against itself in the same rounds.
"""
import argparse
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

N_GENES = 2000


def gene_records(n, umi, seed=2):
    """a gene record per read: the feature a function of the read's molecule (its UMI's letters before the substitution, near
    enough: of the UMI's upper letters), one read in twenty LOW"""
    from badger_amd import _native
    rng = np.random.default_rng(seed)
    recs = np.zeros(n, dtype=_native.GENE_DTYPE)
    recs["feature"] = ((umi.astype(np.uint64) >> np.uint64(8)) * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(40)) % np.uint64(N_GENES)
    recs["flags"] = np.where(rng.random(n) < 0.05, 2, 1)
    recs["hits"] = 40
    return recs


def _time(ctx, call, reps):
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
    kt = {k: round(v[1], 4) for k, v in ctx.profile_read().items() if k.startswith(("k_umi", "k_group")) and v[0]}
    ctx.profile(False)
    return times, kt


def device_probe(args):
    from badger_amd import _native
    _native.PRELOAD_TORCH = False
    ctx = _native.default_context(0)
    for n in [int(x) for x in args.reads.split(",")]:
        cells, rank, has, umi = synthetic(n)
        cell = np.where(has != 0, np.searchsorted(cells, rank), 0xFFFFFFFF).astype(np.uint32)
        recs = gene_records(n, umi)
        d = [_native.DeviceArray.from_host(ctx, a) for a in (cells, rank, has, umi, cell, recs)]
        d_mol = _native.DeviceArray(ctx, n, np.uint32)
        d_cnt = _native.DeviceArray(ctx, (len(cells), 4), np.uint32)
        d_groups = _native.DeviceArray(ctx, n, _native.GENE_GROUP_DTYPE)
        d_n = _native.DeviceArray(ctx, 1, np.uint32)
        for dist in (1, 0):
            per_cell = lambda: ctx.umi_dedup_dev(d[1], d[2], d[3], n, d[0], len(cells), 12, dist, d_mol, d_cnt)      # noqa: E731
            per_gene = lambda: ctx.umi_dedup_genes_dev(d[4], d[5], d[3], n, 12, dist, d_mol, d_groups, n, d_n)      # noqa: E731
            tc, kc = _time(ctx, per_cell, args.reps)
            cnt = d_cnt.to_host()
            tg, kg = _time(ctx, per_gene, args.reps)
            groups = d_groups.to_host(int(d_n.to_host()[0]))
            mc, mg = float(np.median(tc)), float(np.median(tg))
            emit(args.out, {"what": "bdg_umi_dedup_genes_dev beside bdg_umi_dedup_dev, device-resident", "reads": n, "umi_dist": dist,
                            "cells": int(len(cells)), "genes": N_GENES, "per_cell_molecules": int(cnt[:, 3].sum()),
                            "groups": int(len(groups)), "per_gene_molecules": int(groups["molecules"].sum(dtype=np.int64)),
                            "own": int(groups["own"].sum(dtype=np.int64)),
                            "per_cell_ms_median": round(1e3 * mc, 4), "per_gene_ms_median": round(1e3 * mg, 4),
                            "per_cell_ms_per_1M_reads": round(1e3 * mc * 1e6 / n, 4), "per_gene_ms_per_1M_reads": round(1e3 * mg * 1e6 / n, 4),
                            "ratio": round(mg / mc, 3), "per_cell_kernel_ms": kc, "per_gene_kernel_ms": kg, "reps": args.reps})
        # one hot group: every read of one cell and one gene
        hot_cell = np.zeros(n, dtype=np.uint32)
        hot_recs = recs.copy()
        hot_recs["feature"], hot_recs["flags"] = 7, 1
        h = [_native.DeviceArray.from_host(ctx, a) for a in (hot_cell, hot_recs)]
        for on in (True, False):
            ctx.umi_dedup_genes_set_aggregate(on)
            try:
                t, k = _time(ctx, lambda: ctx.umi_dedup_genes_dev(h[0], h[1], d[3], n, 12, 1, d_mol, d_groups, n, d_n), args.reps)
            finally:
                ctx.umi_dedup_genes_set_aggregate(True)
            emit(args.out, {"what": "bdg_umi_dedup_genes_dev, one hot group holding every read", "reads": n, "umi_dist": 1,
                            "wave_aggregation": on, "ms_median": round(1e3 * float(np.median(t)), 4),
                            "ms_per_1M_reads": round(1e3 * float(np.median(t)) * 1e6 / n, 4), "kernel_ms": k, "reps": args.reps})
        for a in d + h + [d_mol, d_cnt, d_groups, d_n]:
            a.free()


def dist2_probe(args):
    from badger_amd import _native
    _native.PRELOAD_TORCH = False
    ctx = _native.default_context(0)
    for n in [int(x) for x in args.reads.split(",")]:
        cells, rank, has, umi = synthetic(n)
        cell = np.where(has != 0, np.searchsorted(cells, rank), 0xFFFFFFFF).astype(np.uint32)
        recs = gene_records(n, umi)
        d = [_native.DeviceArray.from_host(ctx, a) for a in (cells, rank, has, umi, cell, recs)]
        d_mol = _native.DeviceArray(ctx, n, np.uint32)
        d_cnt = _native.DeviceArray(ctx, (len(cells), 4), np.uint32)
        d_groups = _native.DeviceArray(ctx, n, _native.GENE_GROUP_DTYPE)
        d_n = _native.DeviceArray(ctx, 1, np.uint32)
        row = {"what": "k_umi_parent2 (umi_dist 2) beside k_umi_parent (umi_dist 1), device-resident", "reads": n,
               "cells": int(len(cells)), "genes": N_GENES, "reps": args.reps}
        with ctx.umi_max_dist_of(2):
            for dist in (1, 2):
                per_gene = lambda: ctx.umi_dedup_genes_dev(d[4], d[5], d[3], n, 12, dist, d_mol, d_groups, n, d_n)      # noqa: E731
                per_cell = lambda: ctx.umi_dedup_dev(d[1], d[2], d[3], n, d[0], len(cells), 12, dist, d_mol, d_cnt)      # noqa: E731
                tg, kg = _time(ctx, per_gene, args.reps)
                groups = d_groups.to_host(int(d_n.to_host()[0]))
                tc, kc = _time(ctx, per_cell, args.reps)
                cnt = d_cnt.to_host()
                kernel = "k_umi_parent2" if dist == 2 else "k_umi_parent"
                row["dist%d" % dist] = {
                    "per_gene_ms_median": round(1e3 * float(np.median(tg)), 4), "per_cell_ms_median": round(1e3 * float(np.median(tc)), 4),
                    "per_gene_" + kernel + "_ms": kg.get(kernel), "per_cell_" + kernel + "_ms": kc.get(kernel),
                    "per_gene_" + kernel + "_ms_per_1M_reads": round(kg.get(kernel, 0.0) * 1e6 / n, 4),
                    "per_gene_kernel_ms": kg, "per_cell_kernel_ms": kc, "groups": int(len(groups)),
                    "umis": int(groups["umis"].sum(dtype=np.int64)), "per_gene_molecules": int(groups["molecules"].sum(dtype=np.int64)),
                    "per_cell_molecules": int(cnt[:, 3].sum())}
        emit(args.out, row)
        for a in d + [d_mol, d_cnt, d_groups, d_n]:
            a.free()


def cli_probe(args):
    from consensus_probe import _fastq
    from genes_probe import _transcripts_of
    tmp = tempfile.mkdtemp(prefix="umi_gene_probe_")
    fq, wl = _fastq(args.cli_reads, tmp)
    tx = os.path.join(tmp, "tx.fa")
    _transcripts_of(fq, tx)
    args_of = lambda out: ["-m", "badger_amd.badger", "-r", fq, "-d", "tenX_v3", "-l", wl, "-c", "5000", "-tr", "4", "-o", os.path.join(tmp, out)]  # noqa: E731

    def run(cwd, out, extra):
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable] + args_of(out) + extra, cwd=cwd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(r.stdout[-2000:] + r.stderr[-2000:])
        return time.perf_counter() - t0, [l.split(" - ")[-1] for l in r.stdout.split("\n") if "Genes: " in l or "Molecules per gene: " in l]

    def pairs(name_a, a, name_b, b, what):
        walls, said = {name_a: [], name_b: []}, []
        for _ in range(args.pairs):
            for name, (cwd, extra) in ((name_a, a), (name_b, b)):
                t, lines = run(cwd, name, extra)
                walls[name].append(t)
                said = lines or said
        ma, mb = float(np.median(walls[name_a])), float(np.median(walls[name_b]))
        emit(args.out, {"what": what, "reads": args.cli_reads, "pairs": args.pairs, "fastq_bytes": os.path.getsize(fq),
                        name_a + "_s": [round(x, 3) for x in walls[name_a]], name_b + "_s": [round(x, 3) for x in walls[name_b]],
                        "median_" + name_a + "_s": round(ma, 3), "median_" + name_b + "_s": round(mb, 3),
                        "spread_" + name_a + "_s": round(max(walls[name_a]) - min(walls[name_a]), 3),
                        "spread_" + name_b + "_s": round(max(walls[name_b]) - min(walls[name_b]), 3),
                        "ratio_%s_over_%s" % (name_b, name_a): round(mb / ma, 3), "log": said})

    matrix = ["--umi_dedup", "--tagged_reads", os.path.join(tmp, "tagged.fa"), "--transcripts", tx, "--count_matrix", os.path.join(tmp, "matrix")]
    run(ROOT, "warm", matrix)                                          # (the file into the page cache, the runtime's caches)
    if args.dist == 2:                                                 # --gene_umi_dist2 against --umi_per_gene alone, and that against the parent's
        per_gene, what = matrix + ["--umi_per_gene"], "stage2 CLI from FASTQ, --umi_dedup --tagged_reads --count_matrix --umi_per_gene: "
        pairs("umi_per_gene", (ROOT, per_gene), "gene_umi_dist2", (ROOT, per_gene + ["--gene_umi_dist2"]), what + "with --gene_umi_dist2 against without")
        if args.parent:
            parent = os.path.abspath(args.parent)
            pairs("parent", (parent, per_gene), "flag_off", (ROOT, per_gene), what + "this build without --gene_umi_dist2 against the parent commit's")
            pairs("parent_a", (parent, per_gene), "parent_b", (parent, per_gene), what + "the parent commit's build against itself")
        return
    pairs("flag_off", (ROOT, matrix), "umi_per_gene", (ROOT, matrix + ["--umi_per_gene"]),
          "stage2 CLI from FASTQ, --umi_dedup --tagged_reads --count_matrix: with --umi_per_gene against without")
    if args.parent:
        parent = os.path.abspath(args.parent)
        pairs("parent", (parent, matrix), "flag_off", (ROOT, matrix),
              "stage2 CLI from FASTQ, --umi_dedup --tagged_reads --count_matrix: this build with the flag off against the parent commit's")
        pairs("parent_a", (parent, matrix), "parent_b", (parent, matrix),
              "stage2 CLI from FASTQ, --umi_dedup --tagged_reads --count_matrix: the parent commit's build against itself")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--device", action="store_true")
    p.add_argument("--cli", action="store_true")
    p.add_argument("--dist", type=int, default=None, choices=(2,), help="time k_umi_parent2 beside k_umi_parent")
    p.add_argument("--reads", default="1000000,12500000")
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--cli_reads", type=int, default=1000000)
    p.add_argument("--pairs", type=int, default=3)
    p.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.device:
        device_probe(args)
    if args.dist and not args.cli:
        dist2_probe(args)
    if args.cli:
        cli_probe(args)


if __name__ == "__main__":
    main()
