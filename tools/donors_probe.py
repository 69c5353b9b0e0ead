#!/usr/bin/env python3
"""Measurements of the donor step (--donor_genotypes; --donors K).  Every record is one JSON line on
stdout and, with --out, in that file.

    python tools/donors_probe.py --device [--cells 10000] [--entries 300] [--donors 8 32] [--rounds 5] --out profiles/r29_donors.jsonl
        a synthetic pool on the device: per number of donors, bdg_donor_scores_dev over device-resident arrays in alternating
        rounds, k_donor_scores from the context's event timers and the whole call (launch to synchronise) from the host clock;
        beside it the numpy checker on the same input, once, and whether both give the same records.
    python tools/donors_probe.py --cli [--cli_reads 1000000] [--pairs 3] [--parent DIR] --out ...
        the stage-2 command from FASTQ with --variants, with --donor_genotypes (8 donors) against without, in alternating fresh
        processes; with --parent (a built checkout of the parent commit) this build with the flags off against the parent's, and
        the parent's against itself.
    python tools/donors_probe.py --bench --parent DIR [--pairs 3] --out ...
        bench.py --gpus 1 --steps 10 --warmup 3 in alternating fresh processes, this build and the parent's.
    python tools/donors_probe.py --cluster [--cells 10000] [--entries 300] [--donors 8 32] [--rounds 5] --out profiles/r30_donor_clusters.jsonl
        the clustering of --donors K on the same synthetic pool: per K one iteration over device-resident arrays (k_cluster_counts,
        k_cluster_assign) and the final step (k_cluster_words, k_cluster_geno) from the event timers, k_donor_scores on the same
        input in the same rounds, the numpy checker's iteration once, and a whole fit of 8 restarts (bdg_donor_cluster) from the
        host clock.
    python tools/donors_probe.py --cli --cluster_cli [--parent DIR] --out ...
        --cli with its first comparison replaced: the stage-2 command with --donors 8 against --donor_genotypes (8 donors).
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

from umi_dedup_probe import emit  # noqa: E402


def synthetic_pool(n_cells, per_cell, n_donors, n_variants=20000, seed=3):
    """cells of exactly per_cell entries at random variants, the molecules of a random donor with 2 % errors
    -> (entries, cell_off, genotype words)"""
    from badger_amd import donors as dn
    rng = np.random.default_rng(seed)
    dosage = rng.binomial(2, rng.uniform(0.05, 0.5, size=n_variants)[:, None], size=(n_variants, n_donors))
    words = np.zeros(n_variants, dtype=np.uint64)
    for d in range(n_donors):
        words |= dosage[:, d].astype(np.uint64) << np.uint64(2 * d)
    entries = np.zeros(n_cells * per_cell, dtype=dn.ENTRY_DTYPE)
    variant = np.sort(rng.integers(0, n_variants, size=(n_cells, per_cell)), axis=1)
    who = np.repeat(rng.integers(0, n_donors, size=n_cells), per_cell)
    depth = 1 + rng.poisson(0.5, size=n_cells * per_cell)
    p_alt = np.abs(dosage[variant.ravel(), who] / 2 - 0.02)
    alt = rng.binomial(depth, p_alt)
    entries["variant"], entries["ref"], entries["alt"] = variant.ravel(), depth - alt, alt
    return entries, (np.arange(n_cells + 1, dtype=np.uint64) * np.uint64(per_cell)), words


def device_probe(args):
    from badger_amd import _native
    from badger_amd import donors as dn
    ctx = _native.Context(0)
    tables = dn.level_tables()
    pools = {d: synthetic_pool(args.cells, args.entries, d) for d in args.donors}
    dev, per_run, calls = {}, {d: [] for d in args.donors}, {d: [] for d in args.donors}
    for d, (entries, off, words) in pools.items():
        dev[d] = [_native.DeviceArray.from_host(ctx, a) for a in (entries.view(np.uint32), off, words)] + \
                 [_native.DeviceArray(ctx, args.cells * _native.DONOR_DTYPE.itemsize, np.uint8)]
    ctx.profile(True)
    for r in range(args.rounds + 1):                                      # (the first round warms up and is left out)
        for d in args.donors:
            ctx.profile_reset()
            t0 = time.perf_counter()
            ctx.donor_scores_dev(dev[d][0], dev[d][1], args.cells, dev[d][2], len(pools[d][2]), d, tables, dev[d][3])
            ctx.synchronize()
            wall = time.perf_counter() - t0
            if r:
                per_run[d].append(ctx.profile_read()["k_donor_scores"][1])
                calls[d].append(wall * 1e3)
    ctx.profile(False)
    for d, (entries, off, words) in pools.items():
        got = dev[d][3].to_host().view(_native.DONOR_DTYPE)
        t0 = time.perf_counter()
        want = dn.records(dn.scores(entries, off, words, d, tables), d)
        checker_s = time.perf_counter() - t0
        h = d + d * (d - 1) // 2
        ms = float(np.median(per_run[d]))
        emit(args.out, {"what": "bdg_donor_scores_dev, device-resident, no score matrix; the numpy checker on the same input",
                        "cells": args.cells, "entries_per_cell": args.entries, "donors": d, "hypotheses": h,
                        "kernel_ms": [round(x, 4) for x in per_run[d]], "median_kernel_ms": round(ms, 4),
                        "call_ms": [round(x, 4) for x in calls[d]], "median_call_ms": round(float(np.median(calls[d])), 4),
                        "terms_per_s": round(args.cells * args.entries * h / (ms * 1e-3), 0), "entry_bytes": int(entries.nbytes),
                        "checker_s": round(checker_s, 3), "same_records": bool(got.tolist() == want.tolist()), "version": ctx_version()})
        for a in dev[d]:
            a.free()
    ctx.close()


def cluster_probe(args):
    from badger_amd import _native
    from badger_amd import donors as dn
    ctx = _native.Context(0)
    tables = dn.level_tables()
    kernels = ("k_cluster_counts", "k_cluster_assign", "k_cluster_words", "k_cluster_geno", "k_donor_scores")
    for k in args.donors:
        entries, off, words = synthetic_pool(args.cells, args.entries, k)
        n_variants, n = len(words), args.cells
        z = dn.start_assignments(n, k, 1, 1)[0]
        gp = dn.pooled_genotypes(entries, n_variants, tables)
        d = [_native.DeviceArray.from_host(ctx, a) for a in (entries.view(np.uint32), off, z, gp, words)]
        counts, z_out, sums = (_native.DeviceArray(ctx, b, np.uint8) for b in (8 * n_variants * k, 4 * n, 16))
        d_words, geno = _native.DeviceArray(ctx, len(entries), np.uint64), _native.DeviceArray(ctx, n_variants * k, np.uint8)
        recs = _native.DeviceArray(ctx, n * _native.DONOR_DTYPE.itemsize, np.uint8)
        per_run = {name: [] for name in kernels}
        ctx.profile(True)
        for r in range(args.rounds + 1):                                  # (the first round warms up and is left out)
            ctx.profile_reset()
            ctx.donor_cluster_counts_dev(d[0], d[1], n, d[2], n_variants, k, counts)
            ctx.donor_cluster_assign_dev(d[0], d[1], n, d[2], d[3], n_variants, k, tables, counts, z_out, sums)
            ctx.donor_cluster_words_dev(d[0], d[1], n, d[2], d[3], n_variants, k, tables, counts, d_words, geno)
            ctx.donor_scores_dev(d[0], d[1], n, d[4], n_variants, k, tables, recs)
            ctx.synchronize()
            times = ctx.profile_read()
            if r:
                for name in kernels:
                    per_run[name].append(times[name][1])
        ctx.profile(False)
        got = (z_out.to_host().view(np.uint32), sums.to_host().view(np.int64).tolist(), d_words.to_host())
        t0 = time.perf_counter()
        z1, total, changed, _ = dn.cluster_step(entries, off, z, gp, k, tables)
        checker_s = time.perf_counter() - t0
        same = bool(got[0].tolist() == z1.tolist() and got[1] == [total, changed]
                    and got[2].tolist() == dn.entry_words(entries, off, z, gp, k, tables).tolist())
        for a in d + [counts, z_out, sums, d_words, geno, recs]:
            a.free()
        z0 = dn.start_assignments(n, k, 8, 1)
        ctx.donor_cluster(entries, off, n_variants, k, tables, z0[:1], 2)        # (the staging buffers grow here)
        t0 = time.perf_counter()
        fit = ctx.donor_cluster(entries, off, n_variants, k, tables, z0, 50)
        fit_s = time.perf_counter() - t0
        med = {name: round(float(np.median(v)), 4) for name, v in per_run.items()}
        emit(args.out, {"what": "one iteration of the clustering (counts with its clear, assign), the final step (words, genotypes) and "
                                "k_donor_scores on the same input, device-resident; the numpy checker's iteration; a fit of 8 restarts",
                        "cells": n, "entries_per_cell": args.entries, "clusters": k, "variants": n_variants,
                        "kernel_ms": {name: [round(x, 4) for x in v] for name, v in per_run.items()}, "median_kernel_ms": med,
                        "iteration_ms": round(med["k_cluster_counts"] + med["k_cluster_assign"], 4), "entry_bytes": int(entries.nbytes),
                        "count_table_bytes": 8 * n_variants * k, "checker_iteration_s": round(checker_s, 3), "same_as_checker": same,
                        "fit_restarts": 8, "fit_max_iter": 50, "fit_s": round(fit_s, 3), "fit_iterations": int(fit["restarts"]["iterations"].sum()),
                        "fit_table": [list(x) for x in fit["restarts"].tolist()], "fit_chosen": fit["chosen"], "version": ctx_version()})
    ctx.close()


def ctx_version():
    from badger_amd import _native
    return _native.load().bdg_version().decode()


def _genotypes_of(var, path, n_donors=8, seed=5):
    """random genotypes of n_donors donors for every id of a variants file"""
    rng = np.random.default_rng(seed)
    ids = []
    with open(var) as f:
        for line in f:
            name = line.split("\t")[0]
            if name and not line.startswith("#") and (not ids or ids[-1] != name):
                ids.append(name)
    ids = list(dict.fromkeys(ids))
    dosage = rng.binomial(2, rng.uniform(0.05, 0.5, size=len(ids))[:, None], size=(len(ids), n_donors))
    with open(path, "w") as out:
        out.write("variant\t%s\n" % "\t".join("donor%d" % d for d in range(n_donors)))
        for name, row in zip(ids, dosage.tolist()):
            out.write("%s\t%s\n" % (name, "\t".join(str(g) for g in row)))


def cli_probe(args):
    from consensus_probe import _fastq
    from genes_probe import _transcripts_of, _variants_of
    tmp = tempfile.mkdtemp(prefix="donors_probe_")
    fq, wl = _fastq(args.cli_reads, tmp)
    tx, var, geno = (os.path.join(tmp, n) for n in ("tx.fa", "variants.tsv", "donors.tsv"))
    _transcripts_of(fq, tx)
    _variants_of(tx, var)
    _genotypes_of(var, geno)
    args_of = lambda out: ["-m", "badger_amd.badger", "-r", fq, "-d", "tenX_v3", "-l", wl, "-c", "5000", "-tr", "4", "-o", os.path.join(tmp, out)]  # noqa: E731

    def run(cwd, out, extra):
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable] + args_of(out) + extra, cwd=cwd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(r.stdout[-2000:] + r.stderr[-2000:])
        return time.perf_counter() - t0, [l.split(" - ")[-1].replace(tmp, "TMP") for l in r.stdout.split("\n") if "Alleles: " in l or "Donors: " in l]

    def pairs(name_a, a, name_b, b, what):
        walls, said = {name_a: [], name_b: []}, []
        for _ in range(args.pairs):
            for name, (cwd, extra) in ((name_a, a), (name_b, b)):
                t, lines = run(cwd, name, extra)
                walls[name].append(t)
                said = lines if len(lines) > len(said) else said
        ma, mb = float(np.median(walls[name_a])), float(np.median(walls[name_b]))
        emit(args.out, {"what": what, "reads": args.cli_reads, "pairs": args.pairs, "fastq_bytes": os.path.getsize(fq),
                        name_a + "_s": [round(x, 3) for x in walls[name_a]], name_b + "_s": [round(x, 3) for x in walls[name_b]],
                        "median_" + name_a + "_s": round(ma, 3), "median_" + name_b + "_s": round(mb, 3),
                        "spread_" + name_a + "_s": round(max(walls[name_a]) - min(walls[name_a]), 3),
                        "spread_" + name_b + "_s": round(max(walls[name_b]) - min(walls[name_b]), 3),
                        "ratio_%s_over_%s" % (name_b, name_a): round(mb / ma, 3), "log": said})

    fa = os.path.join(tmp, "tagged.fa")
    tagged = ["--umi_dedup", "--tagged_reads", fa]
    run(ROOT, "warm", tagged)                                          # (the file into the page cache, the runtime's caches)
    matrix = tagged + ["--transcripts", tx, "--count_matrix", os.path.join(tmp, "matrix"), "--variants", var]
    if args.cluster_cli:
        pairs("genotypes", (ROOT, matrix + ["--donor_genotypes", geno]), "clusters", (ROOT, matrix + ["--donors", "8"]),
              "stage2 CLI from FASTQ, --umi_dedup --tagged_reads --count_matrix --variants: with --donors 8 against --donor_genotypes (8 donors)")
    else:
        pairs("variants", (ROOT, matrix), "donors", (ROOT, matrix + ["--donor_genotypes", geno]),
              "stage2 CLI from FASTQ, --umi_dedup --tagged_reads --count_matrix --variants: with --donor_genotypes (8 donors) against without")
    if args.parent:
        parent = os.path.abspath(args.parent)
        pairs("parent", (parent, matrix), "flags_off", (ROOT, matrix),
              "stage2 CLI from FASTQ, --umi_dedup --tagged_reads --count_matrix --variants: this build without the new flag against the parent commit's")
        pairs("parent_a", (parent, matrix), "parent_b", (parent, matrix),
              "stage2 CLI from FASTQ, --umi_dedup --tagged_reads --count_matrix --variants: the parent commit's build against itself")


def bench_probe(args):
    rounds = []
    for r in range(args.pairs):
        for who, cwd in (("this", ROOT), ("parent", os.path.abspath(args.parent))):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3"], cwd=cwd, capture_output=True,
                                 text=True, timeout=900)
            if out.returncode != 0:
                raise SystemExit(out.stdout[-2000:] + out.stderr[-2000:])
            line = json.loads([l for l in out.stdout.split("\n") if l.startswith("{")][-1])
            rounds.append({"who": who, "round": r + 1, "ms_per_step": round(line["ms_per_step"], 4)})
    med = {who: float(np.median([x["ms_per_step"] for x in rounds if x["who"] == who])) for who in ("this", "parent")}
    spread = {who: max(x["ms_per_step"] for x in rounds if x["who"] == who) - min(x["ms_per_step"] for x in rounds if x["who"] == who)
              for who in ("this", "parent")}
    emit(args.out, {"what": "bench.py --gpus 1 --steps 10 --warmup 3, alternating rounds of fresh processes, this build and the parent commit's",
                    "rounds": rounds, "median_this_ms": round(med["this"], 4), "median_parent_ms": round(med["parent"], 4),
                    "spread_this_ms": round(spread["this"], 4), "spread_parent_ms": round(spread["parent"], 4),
                    "ratio_this_over_parent": round(med["this"] / med["parent"], 4)})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--device", action="store_true")
    p.add_argument("--cli", action="store_true")
    p.add_argument("--bench", action="store_true")
    p.add_argument("--cluster", action="store_true")
    p.add_argument("--cluster_cli", action="store_true", help="--cli: --donors 8 against --donor_genotypes instead of --donor_genotypes against without")
    p.add_argument("--cells", type=int, default=10000)
    p.add_argument("--entries", type=int, default=300)
    p.add_argument("--donors", type=int, nargs="+", default=[8, 32])
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--cli_reads", type=int, default=1000000)
    p.add_argument("--pairs", type=int, default=3)
    p.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.bench and not args.parent:
        p.error("--bench needs --parent")
    if args.device:
        device_probe(args)
    if args.cluster:
        cluster_probe(args)
    if args.cli:
        cli_probe(args)
    if args.bench:
        bench_probe(args)


if __name__ == "__main__":
    main()
