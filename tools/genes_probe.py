#!/usr/bin/env python3
"""Measurements of the gene calls by k-mer lookup, of the isoform pass on top of them and of the EM
over its class counts, one JSON line each to --out (and stdout).

    python tools/genes_probe.py --device [--reads 1000000] [--tx_bases 4000000 100000000] --out profiles/r22_genes.jsonl
        bdg_genes_index_build and bdg_genes_assign_dev alone.  Per --tx_bases value a random transcriptome of that many bases in
        transcripts of 2,000, a feature each: 4 M bases give a table of 134 MB, which the Infinity Cache holds, 100 M bases one
        of 4.3 GB, which it does not.  The reads are 3' fragments of 300 .. 1,500 bases of random transcripts at synth's error
        rates, every fifth read random, device-resident: wall time of the build (upload, the host's window count, the kernels)
        and of an assign call, and the kernels from the library's event timers.
    python tools/genes_probe.py --cli [--cli_reads 1000000] [--pairs 3] [--parent DIR] --out ...
        the stage-2 command line on consensus_probe's FASTQ file (every read with four siblings), as alternating pairs of fresh
        processes: --tagged_reads --umi_dedup with --count_matrix against without, the transcripts being the middles of the
        first 20,000 reads in both senses; and, with --parent DIR (a built checkout of the parent commit), this build with the
        flags off against the parent, beside parent against parent.
    python tools/genes_probe.py --device --isoforms [--reads 1000000] [--tx_bases 4000000] --out profiles/r23_isoforms.jsonl
        the same workload over genes of 2 .. 4 isoforms: every gene a random text of 2,000 bases, its first
        isoform that text, every other one the text without 150 bases at a place of its own within the last 1,200, behind 150
        bases of its own, so that every transcript has 2,000 bases; features are the genes.  bdg_genes_index_build_iso against
        bdg_genes_index_build, and bdg_genes_assign_dev followed by bdg_iso_assign_dev: k_iso_insert and k_iso_assign beside
        k_genes_insert and k_genes_assign from the event timers of the same run.
    python tools/genes_probe.py --cli --isoforms ...
        the command line with --count_matrix --isoforms against --count_matrix alone (the transcripts paired into genes of two
        by a --tx2gene map: a read's middle and, as its second isoform, the same without its bases 100 .. 199), then the pairs
        with --parent as above.
    python tools/genes_probe.py --em [--em_problems 1000000] [--em_wide 100000] --out profiles/r24_isoform_em.jsonl
        k_em_tcc alone, device-resident, at eps 1e-3 and 1,000 iterations at most: (cell, gene) problems as the
        isoform workload above makes them - genes of 2 .. 4 isoforms, 1 .. 4 molecules a problem, one in four of them compatible
        with more than their own transcript - and problems of 16 .. 64 transcripts with 20 .. 200 molecules in sets of 1 .. 4.
        The share of closed-form problems, the iteration counts and the kernel from the library's event timer.
    python tools/genes_probe.py --cli --isoforms --em ...
        the command line with --isoforms --isoform_em against --isoforms alone, then, in this process, the EM step once more
        over the tagged file of the run: how much of it is the device calls and how much host numpy.
    python tools/genes_probe.py --device --spans [--reads 1000000] [--tx_bases 4000000 100000000] --out profiles/r27_matrix_from_reads.jsonl
        the isoform workload once more: every fragment also lies inside a raw read, behind 100 random bases and in
        front of 60, every second one reverse-complemented, with its span.  bdg_genes_assign_spans_dev and
        bdg_iso_assign_spans_dev on the raw reads beside bdg_genes_assign_dev and bdg_iso_assign_dev on the fragments: the four
        kernels from the event timers of the same run, and whether the records are the same.
    python tools/genes_probe.py --cli --spans ...
        the command line with --umi_dedup --count_matrix --matrix_from_reads against --umi_dedup --tagged_reads --count_matrix,
        the pair once more with --isoforms --isoform_em --umi_per_gene, then the pairs with --parent as above.
    python tools/genes_probe.py --device --alleles [--reads 1000000] [--tx_bases 4000000] --out profiles/r28_alleles.jsonl
        the first workload once more with 4 sites planted per transcript, then with sites on one transcript in ten:
        bdg_alleles_index_build (k_alleles_insert, k_alleles_stats, the whole call) and bdg_alleles_assign_dev behind
        bdg_genes_assign_dev on the same reads: k_alleles_assign beside k_genes_assign from the event timers of the same run,
        the median of --reps runs each.
    python tools/genes_probe.py --cli --alleles ...
        the command line with --count_matrix --variants against --count_matrix alone (4 sites per transcript), then the pairs
        with --parent as above.
    python tools/genes_probe.py --device --discover [--reads 1000000] [--tx_bases 4000000] [--reps 10] --out profiles/r31_discover.jsonl
        the first workload once more: bdg_sites_index_build (k_sites_insert, k_sites_stats, the whole call), then
        bdg_genes_assign_dev, bdg_alleles_assign_dev (4 sites per transcript), bdg_sites_pileup_dev and bdg_sites_select on the same
        reads: k_sites_pileup beside k_genes_assign and k_alleles_assign and k_sites_select from the event timers of the same run,
        the median of --reps runs each; then the pileup alone with every read a fragment of ONE transcript, where every add of
        the call meets the same few thousand addresses.
    python tools/genes_probe.py --cli --discover ...
        the command line with --count_matrix --discover_variants against --count_matrix alone, then the pairs with --parent as
        above.
    python tools/genes_probe.py --device --fusions [--reads 1000000] [--tx_bases 4000000] [--reps 10] --out profiles/r32_fusions.jsonl
        the first workload once more with one read in a hundred a fragment of a planted fusion transcript:
        bdg_fusion_scan_dev behind bdg_genes_assign_dev on the same reads, k_fusion_scan beside k_genes_assign from the event timers
        of the same run, the median of --reps runs each; then the worst case, every read a fragment of a planted fusion, so that
        every read but the random ones passes the gate and the scan walks the windows the gene kernel walks.
    python tools/genes_probe.py --cli --fusions ...
        the command line with --count_matrix --fusions against --count_matrix alone, then the pairs with --parent as above.
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

from umi_dedup_probe import emit  # noqa: E402

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
TX_LEN = 2000


def fragments(tx, n_reads, seed=1, lo=300, hi=1500, chunk=50000):
    """tx: codes of the transcripts [n_tx, TX_LEN] -> (bases uint8 ASCII, off uint64 [n + 1])"""
    rng = np.random.default_rng(seed)
    parts, lens = [], []
    for r0 in range(0, n_reads, chunk):
        m = min(chunk, n_reads - r0)
        L = rng.integers(lo, hi + 1, m)
        t = rng.integers(0, len(tx), m)
        r_off = np.concatenate([[0], np.cumsum(L)])
        rid = np.repeat(np.arange(m), L)
        pos = np.arange(int(r_off[-1])) - r_off[rid]
        codes = tx[t[rid], TX_LEN - L[rid] + pos]
        random_read = (np.arange(r0, r0 + m) % 5 == 4)[rid]
        codes = np.where(random_read, rng.integers(0, 4, len(codes), dtype=np.uint8), codes).astype(np.uint8)
        u = rng.random(len(codes))
        is_del, is_sub, is_ins = u < 0.03, (u >= 0.03) & (u < 0.06), (u >= 0.06) & (u < 0.08)
        codes = np.where(is_sub, (codes + rng.integers(1, 4, len(codes), dtype=np.uint8)) & 3, codes).astype(np.uint8)
        cnt = (~is_del).astype(np.int64) + is_ins
        at = np.cumsum(cnt) - cnt
        out = np.empty(int(cnt.sum()), dtype=np.uint8)
        out[at[~is_del]] = codes[~is_del]
        out[(at + ~is_del)[is_ins]] = rng.integers(0, 4, int(is_ins.sum()), dtype=np.uint8)
        parts.append(ACGT[out])
        lens.append(np.diff(np.concatenate([at, [int(cnt.sum())]])[r_off]))
    return np.concatenate(parts), np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.uint64)


def device_probe(args):
    from badger_amd import _native
    _native.PRELOAD_TORCH = False
    ctx = _native.default_context(0)
    for tx_bases in args.tx_bases:
        n_tx = max(tx_bases // TX_LEN, 1)
        tx = np.random.default_rng(7).integers(0, 4, (n_tx, TX_LEN), dtype=np.uint8)
        bases, off = fragments(tx, args.reads)
        n = len(off) - 1
        tx_ascii, tx_off = ACGT[tx].ravel(), (np.arange(n_tx + 1) * TX_LEN).astype(np.uint64)
        feat = np.arange(n_tx, dtype=np.uint32)
        ctx.genes_index_build(tx_ascii, tx_off, feat, args.k)             # (warm: the first allocation of this size)
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        ctx.genes_index_build(tx_ascii, tx_off, feat, args.k)
        build_s = time.perf_counter() - t0
        build_kt = {k: round(v[1], 4) for k, v in ctx.profile_read().items() if k.startswith("k_genes") and v[0]}
        ctx.profile(False)
        stats = [int(x) for x in ctx.genes_index_stats()]
        d = [_native.DeviceArray.from_host(ctx, a) for a in (bases, off)]
        d_out = _native.DeviceArray(ctx, n * 6, np.uint32)
        call = lambda: ctx.genes_assign_dev(d[0], d[1], n, args.min_hits, d_out)  # noqa: E731
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
        for _ in range(args.reps):
            call()
        ctx.synchronize()
        kt = {k: round(v[1] / args.reps, 4) for k, v in ctx.profile_read().items() if k.startswith("k_genes") and v[0]}
        ctx.profile(False)
        recs = d_out.to_host().view(_native.GENE_DTYPE)
        emit(args.out, {"what": "bdg_genes_index_build, bdg_genes_assign_dev, device-resident", "k": args.k, "min_hits": args.min_hits,
                        "transcripts": n_tx, "transcript_bases": int(n_tx * TX_LEN), "table_bytes": 16 * stats[3],
                        "stats": dict(zip(("windows", "keys", "ambiguous", "slots", "longest_run", "wrapped"), stats)),
                        "build_wall_s": round(build_s, 3), "build_kernel_ms": build_kt,
                        "reads": n, "read_bases": int(off[-1]), "windows_looked_up": int(recs["n_keys"].astype(np.int64).sum()),
                        "found": int(recs["n_found"].astype(np.int64).sum()), "assigned": int((recs["flags"] & 1 != 0).sum()),
                        "low": int((recs["flags"] & 2 != 0).sum()), "assign_call_ms_median": round(1e3 * float(np.median(times)), 3),
                        "assign_call_ms_min": round(1e3 * min(times), 3), "assign_kernel_ms": kt,
                        "assign_kernel_ms_per_1M_reads": {k: round(v * 1e6 / n, 3) for k, v in kt.items()}})
        for a in d + [d_out]:
            a.free()
    ctx.genes_index_build(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), args.k)


def device_probe_alleles(args):
    from badger_amd import _native
    _native.PRELOAD_TORCH = False
    ctx = _native.default_context(0)
    ak, sites_per_tx = 15, 4
    for tx_bases in args.tx_bases:
        n_tx = max(tx_bases // TX_LEN, 1)
        rng = np.random.default_rng(7)
        tx = rng.integers(0, 4, (n_tx, TX_LEN), dtype=np.uint8)
        bases, off = fragments(tx, args.reads)
        n = len(off) - 1
        tx_ascii, tx_off = ACGT[tx].ravel(), (np.arange(n_tx + 1) * TX_LEN).astype(np.uint64)
        ctx.genes_index_build(tx_ascii, tx_off, np.arange(n_tx, dtype=np.uint32), args.k)
        d = [_native.DeviceArray.from_host(ctx, a) for a in (bases, off)]
        d_gene = _native.DeviceArray(ctx, n * 6, np.uint32)
        for every in (1, 10):
            # the allele sequences of sites_per_tx sites in the last 1,500 bases of every `every`-th transcript: 2 k - 1 bases each
            which = np.arange(0, n_tx, every)
            pos = TX_LEN - 1500 + np.sort(rng.integers(ak, 1500 - ak, (len(which), sites_per_tx)), axis=1)
            t_of, p_of = np.repeat(which, sites_per_tx), pos.ravel()
            win = tx[t_of[:, None], p_of[:, None] + np.arange(1 - ak, ak)[None, :]]
            alt = win.copy()
            alt[:, ak - 1] = (alt[:, ak - 1] + rng.integers(1, 4, len(alt), dtype=np.uint8)) & 3
            seqs = ACGT[np.stack([win, alt], axis=1).reshape(-1, 2 * ak - 1)]
            values = np.arange(2 * len(t_of), dtype=np.uint32)
            seq_off = (np.arange(len(seqs) + 1) * (2 * ak - 1)).astype(np.uint64)
            genes = t_of.astype(np.uint32)
            build = lambda: ctx.alleles_index_build(seqs.ravel(), seq_off, values, genes, n_tx, ak)  # noqa: E731
            build()
            ctx.profile(True)
            ctx.profile_reset()
            t0 = time.perf_counter()
            build()
            build_s = time.perf_counter() - t0
            build_kt = {k: round(v[1], 4) for k, v in ctx.profile_read().items() if k.startswith("k_alleles") and v[0]}
            ctx.profile(False)
            stats, per_value = ctx.alleles_index_stats()
            cap = 8 * n
            d_out, d_counts = _native.DeviceArray(ctx, cap * 4, np.uint32), _native.DeviceArray(ctx, 2, np.uint64)

            def call():
                ctx.genes_assign_dev(d[0], d[1], n, args.min_hits, d_gene)
                ctx.alleles_assign_dev(d[0], d[1], n, d_gene, d_out, cap, d_counts)
            call()
            ctx.synchronize()
            per_run = {}
            ctx.profile(True)
            for _ in range(args.reps):
                ctx.profile_reset()
                call()
                ctx.synchronize()
                for k, v in ctx.profile_read().items():
                    if k in ("k_genes_assign", "k_alleles_assign") and v[0]:
                        per_run.setdefault(k, []).append(v[1])
            ctx.profile(False)
            counts = d_counts.to_host()
            recs = d_out.to_host().view(_native.ALLELE_DTYPE)[:int(counts[0])]
            gene_recs = d_gene.to_host().view(_native.GENE_DTYPE)
            emit(args.out, {"what": "bdg_alleles_index_build, bdg_alleles_assign_dev behind bdg_genes_assign_dev, device-resident",
                            "allele_k": ak, "gene_k": args.k, "transcripts": n_tx, "transcripts_with_sites": len(which),
                            "variants": len(t_of), "table_bytes": 16 * int(stats[3]),
                            "stats": dict(zip(("windows", "keys", "ambiguous", "slots", "longest_run", "wrapped"), [int(x) for x in stats])),
                            "values_without_a_key": int((per_value == 0).sum()),
                            "build_wall_s": round(build_s, 4), "build_kernel_ms": build_kt, "reads": n, "read_bases": int(off[-1]),
                            "reads_assigned": int((gene_recs["flags"] & 1 != 0).sum()), "records": int(counts[0]), "crowded": int(counts[1]),
                            "reads_with_a_record": int(len(np.unique(recs["read"]))), "ref_hits": int(recs["ref_hits"].sum(dtype=np.int64)),
                            "alt_hits": int(recs["alt_hits"].sum(dtype=np.int64)), "reps": args.reps,
                            "kernel_ms_median": {k: round(float(np.median(v)), 4) for k, v in per_run.items()},
                            "kernel_ms_runs": {k: [round(x, 4) for x in v] for k, v in per_run.items()},
                            "alleles_over_genes": round(float(np.median(per_run["k_alleles_assign"]) / np.median(per_run["k_genes_assign"])), 4)})
            d_out.free()
            d_counts.free()
        for a in d + [d_gene]:
            a.free()
    ctx.genes_index_build(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), args.k)
    ctx.alleles_index_build(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0, ak)


def device_probe_discover(args):
    from badger_amd import _native
    _native.PRELOAD_TORCH = False
    ctx = _native.default_context(0)
    ak, dk, sites_per_tx = 15, args.discover_k, 4
    for tx_bases in args.tx_bases:
        n_tx = max(tx_bases // TX_LEN, 1)
        rng = np.random.default_rng(7)
        tx = rng.integers(0, 4, (n_tx, TX_LEN), dtype=np.uint8)
        tx_ascii, tx_off = ACGT[tx].ravel(), (np.arange(n_tx + 1) * TX_LEN).astype(np.uint64)
        feat = np.arange(n_tx, dtype=np.uint32)
        ctx.genes_index_build(tx_ascii, tx_off, feat, args.k)
        pos = TX_LEN - 1500 + np.sort(rng.integers(ak, 1500 - ak, (n_tx, sites_per_tx)), axis=1)
        t_of, p_of = np.repeat(np.arange(n_tx), sites_per_tx), pos.ravel()
        win = tx[t_of[:, None], p_of[:, None] + np.arange(1 - ak, ak)[None, :]]
        alt = win.copy()
        alt[:, ak - 1] = (alt[:, ak - 1] + rng.integers(1, 4, len(alt), dtype=np.uint8)) & 3
        seqs = ACGT[np.stack([win, alt], axis=1).reshape(-1, 2 * ak - 1)]
        ctx.alleles_index_build(seqs.ravel(), (np.arange(len(seqs) + 1) * (2 * ak - 1)).astype(np.uint64),
                                np.arange(2 * len(t_of), dtype=np.uint32), t_of.astype(np.uint32), n_tx, ak)
        build = lambda: ctx.sites_index_build(tx_ascii, tx_off, feat, dk)  # noqa: E731
        build()
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        build()
        build_s = time.perf_counter() - t0
        build_kt = {k: round(v[1], 4) for k, v in ctx.profile_read().items() if k.startswith("k_sites") and v[0]}
        ctx.profile(False)
        stats = [int(x) for x in ctx.sites_index_stats()]
        for what, reads_of in (("reads of every transcript", tx), ("every read of one transcript", tx[:1])):
            bases, off = fragments(reads_of, args.reads)
            n = len(off) - 1
            d = [_native.DeviceArray.from_host(ctx, a) for a in (bases, off)]
            d_gene = _native.DeviceArray(ctx, n * 6, np.uint32)
            cap = 8 * n
            d_out, d_counts = _native.DeviceArray(ctx, cap * 4, np.uint32), _native.DeviceArray(ctx, 2, np.uint64)
            selected = []

            def call():
                ctx.genes_assign_dev(d[0], d[1], n, args.min_hits, d_gene)
                ctx.alleles_assign_dev(d[0], d[1], n, d_gene, d_out, cap, d_counts)
                ctx.sites_reset()
                ctx.sites_pileup_dev(d[0], d[1], n, d_gene)
                selected.append(len(ctx.sites_select(args.discover_min_alt, 100000, cap=1 << 16)))
            call()
            ctx.synchronize()
            per_run = {}
            ctx.profile(True)
            for _ in range(args.reps):
                ctx.profile_reset()
                call()
                ctx.synchronize()
                for k, v in ctx.profile_read().items():
                    if k in ("k_genes_assign", "k_alleles_assign", "k_sites_pileup", "k_sites_select") and v[0]:
                        per_run.setdefault(k, []).append(v[1])
            ctx.profile(False)
            counts = ctx.sites_counts(n_tx * TX_LEN)
            gene_recs = d_gene.to_host().view(_native.GENE_DTYPE)
            med = {k: float(np.median(v)) for k, v in per_run.items()}
            emit(args.out, {"what": "bdg_sites_index_build, bdg_sites_pileup_dev behind bdg_genes_assign_dev, bdg_sites_select, device-resident: " + what,
                            "count_layout": args.count_layout, "discover_k": dk, "gene_k": args.k, "allele_k": ak, "transcripts": n_tx,
                            "transcript_bases": int(n_tx * TX_LEN), "table_bytes": 16 * stats[3], "count_bytes": 16 * int(n_tx * TX_LEN),
                            "stats": dict(zip(("windows", "keys", "ambiguous", "slots", "longest_run", "wrapped"), stats)),
                            "build_wall_s": round(build_s, 4), "build_kernel_ms": build_kt, "reads": n, "read_bases": int(off[-1]),
                            "reads_assigned": int((gene_recs["flags"] & 1 != 0).sum()), "evidence": int(counts.sum(dtype=np.int64)),
                            "sites_with_evidence": int((counts.sum(axis=1) > 0).sum()), "largest_count": int(counts.max(initial=0)),
                            "selected": selected[-1], "min_alt": args.discover_min_alt, "ppm": 100000, "reps": args.reps,
                            "kernel_ms_median": {k: round(v, 4) for k, v in med.items()},
                            "kernel_ms_runs": {k: [round(x, 4) for x in v] for k, v in per_run.items()},
                            "pileup_over_genes": round(med["k_sites_pileup"] / med["k_genes_assign"], 4),
                            "pileup_over_alleles": round(med["k_sites_pileup"] / med["k_alleles_assign"], 4)})
            for a in d + [d_gene, d_out, d_counts]:
                a.free()
    ctx.genes_index_build(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), args.k)
    ctx.alleles_index_build(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0, ak)
    ctx.sites_index_build(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), dk)


def device_probe_fusions(args):
    from badger_amd import _native
    from badger_amd import fusions as fu
    _native.PRELOAD_TORCH = False
    ctx = _native.default_context(0)
    for tx_bases in args.tx_bases:
        n_tx = max(tx_bases // TX_LEN, 1)
        rng = np.random.default_rng(7)
        tx = rng.integers(0, 4, (n_tx, TX_LEN), dtype=np.uint8)
        ctx.genes_index_build(ACGT[tx].ravel(), (np.arange(n_tx + 1) * TX_LEN).astype(np.uint64), np.arange(n_tx, dtype=np.uint32), args.k)

        def fused(cut, n_f=1000):                         # fusion transcripts: the first `cut` bases of one, the rest of another
            u, d = rng.integers(0, n_tx, n_f), rng.integers(0, n_tx, n_f)
            return np.concatenate([tx[u, :cut], tx[d, cut:]], axis=1)
        n_few = args.reads // 100
        for what, parts in (("one read in a hundred a fragment of a planted fusion, the junction 1,000 bases from the 3' end",
                             ((tx, args.reads - n_few, 1), (fused(TX_LEN - 1000), n_few, 2))),
                            ("the worst case: every read a fragment of a planted fusion, the junction 300 bases from the 3' end",
                             ((fused(TX_LEN - 300), args.reads, 3),))):
            bases, off = fragments(*parts[0])
            for part in parts[1:]:
                more, more_off = fragments(*part)
                bases, off = np.concatenate([bases, more]), np.concatenate([off, more_off[1:] + off[-1]]).astype(np.uint64)
            n = len(off) - 1
            d = [_native.DeviceArray.from_host(ctx, a) for a in (bases, off)]
            d_gene, d_out = _native.DeviceArray(ctx, n * 6, np.uint32), _native.DeviceArray(ctx, n * 10, np.uint32)

            def call():
                ctx.genes_assign_dev(d[0], d[1], n, args.min_hits, d_gene)
                ctx.fusion_scan_dev(d[0], d[1], n, d_gene, args.fusion_min_hits, d_out)
            call()
            ctx.synchronize()
            per_run = {}
            ctx.profile(True)
            for _ in range(args.reps):
                ctx.profile_reset()
                call()
                ctx.synchronize()
                for k, v in ctx.profile_read().items():
                    if k in ("k_genes_assign", "k_fusion_scan") and v[0]:
                        per_run.setdefault(k, []).append(v[1])
            ctx.profile(False)
            flags = d_out.to_host().view(_native.FUSION_DTYPE)["flags"]
            med = {k: float(np.median(v)) for k, v in per_run.items()}
            emit(args.out, {"what": "bdg_fusion_scan_dev behind bdg_genes_assign_dev, device-resident: " + what, "gene_k": args.k,
                            "gene_min_hits": args.min_hits, "fusion_min_hits": args.fusion_min_hits, "transcripts": n_tx,
                            "transcript_bases": int(n_tx * TX_LEN), "reads": n, "read_bases": int(off[-1]),
                            "scanned": int(((flags & fu.SKIPPED) == 0).sum()), "split": int(((flags & fu.SPLIT) != 0).sum()),
                            "interleaved": int(((flags & fu.INTERLEAVED) != 0).sum()), "reps": args.reps,
                            "kernel_ms_median": {k: round(v, 4) for k, v in med.items()},
                            "kernel_ms_runs": {k: [round(x, 4) for x in v] for k, v in per_run.items()},
                            "fusion_over_genes": round(med["k_fusion_scan"] / med["k_genes_assign"], 4)})
            for a in d + [d_gene, d_out]:
                a.free()
    ctx.genes_index_build(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), args.k)


def _variants_of(tx, path, per_tx=4):
    """per_tx sites, evenly spread, in every transcript of a FASTA (name line, sequence line) that has no N there"""
    with open(tx, "rb") as f, open(path, "wb") as out:
        for name in f:
            name, s = name[1:].strip(), f.readline().strip().upper()
            for j in range(per_tx):
                p = (j + 1) * len(s) // (per_tx + 1)
                if s[p:p + 1] in (b"A", b"C", b"G", b"T"):
                    out.write(b"%s.%d\t%s\t%d\t%s\t%s\n" % (name, j, name, p + 1, s[p:p + 1], b"CGTA"[b"ACGT".index(s[p:p + 1]):][:1]))


def iso_transcriptome(n_tx, seed=7):
    """-> (codes [n_tx', TX_LEN], feature of each uint32, local index of each uint8), n_tx' the first gene count that reaches n_tx"""
    rng = np.random.default_rng(seed)
    tx, feat, local, g = [], [], [], 0
    while len(tx) < n_tx:
        gene = rng.integers(0, 4, TX_LEN, dtype=np.uint8)
        cuts = rng.permutation(7)[:int(rng.integers(1, 4))] * 150 + TX_LEN - 1200          # 1 .. 3 skipping isoforms
        for i, c in enumerate([None] + cuts.tolist()):
            tx.append(gene if c is None else np.concatenate([rng.integers(0, 4, 150, dtype=np.uint8), gene[:c], gene[c + 150:]]))
            feat.append(g)
            local.append(i)
        g += 1
    return np.stack(tx), np.array(feat, dtype=np.uint32), np.array(local, dtype=np.uint8)


def device_probe_iso(args):
    from badger_amd import _native
    _native.PRELOAD_TORCH = False
    ctx = _native.default_context(0)
    for tx_bases in args.tx_bases:
        tx, feat, local = iso_transcriptome(max(tx_bases // TX_LEN, 1))
        n_tx = len(tx)
        bases, off = fragments(tx, args.reads)
        n = len(off) - 1
        tx_ascii, tx_off = ACGT[tx].ravel(), (np.arange(n_tx + 1) * TX_LEN).astype(np.uint64)
        builds = {}
        for name, build in (("plain", lambda: ctx.genes_index_build(tx_ascii, tx_off, feat, args.k)),
                            ("iso", lambda: ctx.genes_index_build_iso(tx_ascii, tx_off, feat, local, args.k))):
            build()                                                       # (warm: the first allocation of this size)
            ctx.profile(True)
            ctx.profile_reset()
            t0 = time.perf_counter()
            build()
            wall = time.perf_counter() - t0
            builds[name] = {"wall_s": round(wall, 3),
                            "kernel_ms": {k: round(v[1], 4) for k, v in ctx.profile_read().items() if k.startswith(("k_genes", "k_iso")) and v[0]}}
            ctx.profile(False)
        stats = [int(x) for x in ctx.genes_index_stats()]
        d = [_native.DeviceArray.from_host(ctx, a) for a in (bases, off)]
        d_gene, d_iso = _native.DeviceArray(ctx, n * 6, np.uint32), _native.DeviceArray(ctx, n * 8, np.uint32)

        def call():
            ctx.genes_assign_dev(d[0], d[1], n, args.min_hits, d_gene)
            ctx.iso_assign_dev(d[0], d[1], n, d_gene, args.margin, d_iso)
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
        for _ in range(args.reps):
            call()
        ctx.synchronize()
        kt = {k: round(v[1] / args.reps, 4) for k, v in ctx.profile_read().items() if k.startswith(("k_genes", "k_iso")) and v[0]}
        ctx.profile(False)
        gene, iso = d_gene.to_host().view(_native.GENE_DTYPE), d_iso.to_host().view(_native.ISO_DTYPE)
        assigned = gene["flags"] & 1 != 0
        emit(args.out, {"what": "bdg_genes_index_build_iso, bdg_genes_assign_dev + bdg_iso_assign_dev, device-resident", "k": args.k,
                        "min_hits": args.min_hits, "margin": args.margin, "transcripts": n_tx, "genes": int(feat.max()) + 1,
                        "transcript_bases": int(n_tx * TX_LEN), "table_bytes": 16 * stats[3], "mask_bytes": 8 * stats[3],
                        "stats": dict(zip(("windows", "keys", "ambiguous", "slots", "longest_run", "wrapped"), stats)),
                        "build": builds, "reads": n, "read_bases": int(off[-1]),
                        "windows_looked_up": int(gene["n_keys"].astype(np.int64).sum()), "found": int(gene["n_found"].astype(np.int64).sum()),
                        "assigned": int(assigned.sum()), "windows_of_the_gene": int(iso["n_gene"].astype(np.int64).sum()),
                        "n_gene_is_hits": bool((iso["n_gene"] == np.where(assigned, gene["hits"], 0)).all()),
                        "unique": int((iso["flags"] & 1 != 0).sum()), "multi": int((iso["flags"] & 2 != 0).sum()),
                        "no_gene": int((iso["flags"] & 4 != 0).sum()),
                        "both_calls_ms_median": round(1e3 * float(np.median(times)), 3), "both_calls_ms_min": round(1e3 * min(times), 3),
                        "assign_kernel_ms": kt, "assign_kernel_ms_per_1M_reads": {k: round(v * 1e6 / n, 3) for k, v in kt.items()}})
        for a in d + [d_gene, d_iso]:
            a.free()
    ctx.genes_index_build(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), args.k)


def raw_reads(bases, off, seed=3, pre=100, suf=60, chunk=50000):
    """every read of (bases, off) inside a raw read of its own: `pre` random bases, the read - every second one
    reverse-complemented - and `suf` random bases -> (raw bases, raw off, spans SPAN_DTYPE)"""
    from badger_amd import _native
    rng = np.random.default_rng(seed)
    n = len(off) - 1
    L = np.diff(off.astype(np.int64))
    raw_off = np.concatenate([[0], np.cumsum(L + pre + suf)])
    raw = ACGT[rng.integers(0, 4, int(raw_off[-1]), dtype=np.uint8)]
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        a, b = int(off[r0]), int(off[r1])
        rid = np.repeat(np.arange(r0, r1), L[r0:r1])
        pos = np.arange(a, b) - off.astype(np.int64)[rid]
        rc = (rid & 1) == 1
        raw[raw_off[rid] + pre + np.where(rc, L[rid] - 1 - pos, pos)] = np.where(rc, comp[bases[a:b]], bases[a:b])
    spans = np.zeros(n, dtype=_native.SPAN_DTYPE)
    spans["begin"], spans["end"], spans["rc"] = pre, pre + L, np.arange(n) & 1
    return raw, raw_off.astype(np.uint64), spans


def device_probe_spans(args):
    from badger_amd import _native
    _native.PRELOAD_TORCH = False
    ctx = _native.default_context(0)
    for tx_bases in args.tx_bases:
        tx, feat, local = iso_transcriptome(max(tx_bases // TX_LEN, 1))
        n_tx = len(tx)
        bases, off = fragments(tx, args.reads)
        raw, raw_off, spans = raw_reads(bases, off)
        n = len(off) - 1
        ctx.genes_index_build_iso(ACGT[tx].ravel(), (np.arange(n_tx + 1) * TX_LEN).astype(np.uint64), feat, local, args.k)
        stats = [int(x) for x in ctx.genes_index_stats()]
        d = [_native.DeviceArray.from_host(ctx, a) for a in (bases, off, raw, raw_off, spans)]
        out = [_native.DeviceArray(ctx, n * w, np.uint32) for w in (6, 8, 6, 8)]

        def forward():
            ctx.genes_assign_dev(d[0], d[1], n, args.min_hits, out[0])
            ctx.iso_assign_dev(d[0], d[1], n, out[0], args.margin, out[1])

        def spanned():
            ctx.genes_assign_spans_dev(d[2], d[3], n, d[4], args.min_hits, out[2])
            ctx.iso_assign_spans_dev(d[2], d[3], n, d[4], out[2], args.margin, out[3])
        walls = {}
        for name, call in (("forward", forward), ("spans", spanned)):
            call()
            ctx.synchronize()
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                call()
                ctx.synchronize()
                times.append(time.perf_counter() - t0)
            walls[name] = round(1e3 * float(np.median(times)), 3)
        # the kernels, one call of each form after the other, every repetition timed on its own: medians
        per = {}
        for _ in range(args.reps):
            ctx.profile(True)
            ctx.profile_reset()
            forward()
            spanned()
            ctx.synchronize()
            for k, v in ctx.profile_read().items():
                if k.startswith(("k_genes_assign", "k_iso_assign")) and v[0]:
                    per.setdefault(k, []).append(v[1])
            ctx.profile(False)
        kt = {k: round(float(np.median(v)), 4) for k, v in per.items()}
        host = [o.to_host() for o in out]
        emit(args.out, {"what": "span kernels on raw reads beside the forward kernels on the materialised cDNA, device-resident",
                        "k": args.k, "min_hits": args.min_hits, "margin": args.margin, "transcripts": n_tx, "transcript_bases": int(n_tx * TX_LEN),
                        "table_bytes": 16 * stats[3], "mask_bytes": 8 * stats[3], "reads": n, "cdna_bases": int(off[-1]),
                        "raw_bases": int(raw_off[-1]), "reverse_complemented": int(spans["rc"].sum()), "reps": args.reps,
                        "gene_records_equal": bool((host[0] == host[2]).all()), "iso_records_equal": bool((host[1] == host[3]).all()),
                        "assigned": int((host[0].view(_native.GENE_DTYPE)["flags"] & 1 != 0).sum()),
                        "both_calls_ms_median": walls, "kernel_ms_median": kt,
                        "spans_over_forward": {"genes": round(kt["k_genes_assign_spans"] / kt["k_genes_assign"], 4),
                                               "iso": round(kt["k_iso_assign_spans"] / kt["k_iso_assign"], 4)}})
        for a in d + out:
            a.free()
    ctx.genes_index_build(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), args.k)


def em_workload(n_prob, t_lo, t_hi, mol_lo, mol_hi, p_multi, extra_max, seed):
    """n_prob problems: T transcripts (t_lo .. t_hi), mol_lo .. mol_hi molecules each of a random transcript of the problem;
    with probability p_multi a molecule is also compatible with 1 .. extra_max other transcripts
    -> (classes, prob_off, out_off) as bdg_em_tcc takes them"""
    from badger_amd import genes as gn
    rng = np.random.default_rng(seed)
    T = rng.integers(t_lo, t_hi + 1, n_prob)
    n_mol = rng.integers(mol_lo, mol_hi + 1, n_prob)
    prob = np.repeat(np.arange(n_prob), n_mol)
    Tm = T[prob]
    cls = np.uint64(1) << (rng.random(len(prob)) * Tm).astype(np.uint64)
    extras = np.where(rng.random(len(prob)) < p_multi, rng.integers(1, extra_max + 1, len(prob)), 0)
    for e in range(extra_max):
        more = np.uint64(1) << (rng.random(len(prob)) * Tm).astype(np.uint64)
        cls = np.where(extras > e, cls | more, cls)
    _, classes, off = gn._em_group(prob[:, None].astype(np.int64), cls)
    return classes, off, gn.em_out_off(classes, off)


def em_probe(args):
    from badger_amd import _native
    from badger_amd import genes as gn
    _native.PRELOAD_TORCH = False
    ctx = _native.default_context(0)
    for what, n_prob, shape in (("cell problems of genes of 2 .. 4 isoforms", args.em_problems, (2, 4, 1, 4, 0.25, 2)),
                                ("problems of 16 .. 64 transcripts", args.em_wide, (16, 64, 20, 200, 0.6, 3))):
        classes, off, out_off = em_workload(n_prob, *shape, seed=24)
        n_out = int(out_off[-1])
        d = [_native.DeviceArray.from_host(ctx, a) for a in (classes.view(np.uint32), off, out_off)]
        d_alpha, d_info = _native.DeviceArray(ctx, max(n_out, 1), np.float32), _native.DeviceArray(ctx, n_prob * 4, np.uint32)
        call = lambda: ctx.em_tcc_dev(d[0], d[1], n_prob, d[2], None, args.em_eps, args.em_max_iter, d_alpha, d_info)  # noqa: E731
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
        for _ in range(args.reps):
            call()
        ctx.synchronize()
        kt = {k: round(v[1] / args.reps, 4) for k, v in ctx.profile_read().items() if k.startswith("k_em") and v[0]}
        ctx.profile(False)
        info, alpha = d_info.to_host().view(_native.EM_INFO_DTYPE), d_alpha.to_host()
        it = info["iters"][info["flags"] != gn.EM_CLOSED].astype(np.int64)
        per_prob = np.diff(off.astype(np.int64))
        emit(args.out, {"what": "bdg_em_tcc_dev, device-resident: " + what, "form": "one problem per wave", "eps": args.em_eps,
                        "max_iter": args.em_max_iter, "problems": n_prob, "classes": int(off[-1]), "classes_per_problem_max": int(per_prob.max()),
                        "transcripts": n_out, "molecules": int(classes["count"].astype(np.int64).sum()),
                        "closed": int((info["flags"] == gn.EM_CLOSED).sum()), "closed_share": round(float((info["flags"] == gn.EM_CLOSED).mean()), 4),
                        "converged": int((info["flags"] == gn.EM_CONVERGED).sum()), "at_cap": int((info["flags"] == gn.EM_MAXITER).sum()),
                        "iterations_total": int(it.sum()), "iterations_median": float(np.median(it)) if len(it) else 0.0,
                        "iterations_max": int(it.max(initial=0)),
                        "class_steps_total": int((info["iters"].astype(np.int64) * per_prob).sum()),
                        "alpha_sum": round(float(alpha[:n_out].astype(np.float64).sum()), 3),
                        "call_ms_median": round(1e3 * float(np.median(times)), 3), "call_ms_min": round(1e3 * min(times), 3), "kernel_ms": kt,
                        "kernel_ms_per_1M_problems": {k: round(v * 1e6 / n_prob, 3) for k, v in kt.items()}})
        for a in d + [d_alpha, d_info]:
            a.free()


def em_split_probe(args, tagged, tx, tx_map):
    """the EM step of the command line once more, in this process: seconds in em_files, and of them in the device calls"""
    from badger_amd import _native
    from badger_amd import genes as gn
    _native.PRELOAD_TORCH = False
    spent = {"em_files_s": 0.0, "device_calls_s": 0.0, "device_calls": 0}
    files_of, device_of = gn.em_files, gn.device_em

    def timed_files(*a, **kw):
        t0 = time.perf_counter()
        try:
            return files_of(*a, **kw)
        finally:
            spent["em_files_s"] += time.perf_counter() - t0

    def timed_device(ctx):
        run = device_of(ctx)

        def call(*a):
            t0 = time.perf_counter()
            try:
                return run(*a)
            finally:
                spent["device_calls_s"] += time.perf_counter() - t0
                spent["device_calls"] += 1
        return call
    gn.em_files, gn.device_em = timed_files, timed_device
    try:
        ctx = _native.default_context(0)
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        counts = gn.count_matrix_of_tagged(tagged, tx, tx_map, os.path.join(os.path.dirname(tagged), "matrix_split"), iso_margin=1,
                                           em=(args.em_eps, args.em_max_iter, "uniform"))
        total = time.perf_counter() - t0
        kt = {k: round(v[1], 4) for k, v in ctx.profile_read().items() if k.startswith("k_em") and v[0]}
        ctx.profile(False)
    finally:
        gn.em_files, gn.device_em = files_of, device_of
    emit(args.out, {"what": "count_matrix_of_tagged with --isoforms --isoform_em, in process: where the EM step's time goes",
                    "whole_call_s": round(total, 3), "em_files_s": round(spent["em_files_s"], 3),
                    "device_calls_s": round(spent["device_calls_s"], 3), "device_calls": spent["device_calls"],
                    "host_numpy_s": round(spent["em_files_s"] - spent["device_calls_s"], 3), "kernel_ms": kt,
                    "counts": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in counts.items() if k.startswith(("em_", "mol_", "classes"))}})


def _transcripts_of(fq, path, n=20000):
    """the middles of the first n reads of a FASTQ file, as they are and reverse-complemented, as a transcript FASTA"""
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    with open(fq, "rb") as f, open(path, "wb") as out:
        for i in range(n):
            f.readline()
            s = f.readline().strip()
            f.readline()
            f.readline()
            if len(s) < 520:
                continue
            mid = s[200:-200]
            out.write(b">t%df\n%s\n>t%dr\n%s\n" % (i, mid, i, mid.translate(comp)[::-1]))


def _isoforms_of(tx, path_fa, path_map):
    """every transcript of a FASTA (name line, sequence line) and, as a second isoform of its gene, the same without its bases
    100 .. 199; the gene map beside it"""
    with open(tx, "rb") as f, open(path_fa, "wb") as out, open(path_map, "wb") as m:
        for name in f:
            name, s = name[1:].strip(), f.readline().strip()
            out.write(b">%s\n%s\n>%s.skip\n%s\n" % (name, s, name, s[:100] + s[200:]))
            m.write(b"%s\tg_%s\n%s.skip\tg_%s\n" % (name, name, name, name))


def cli_probe(args):
    from consensus_probe import _fastq
    tmp = tempfile.mkdtemp(prefix="genes_probe_")
    fq, wl = _fastq(args.cli_reads, tmp)
    tx = os.path.join(tmp, "tx.fa")
    _transcripts_of(fq, tx)
    args_of = lambda out: ["-m", "badger_amd.badger", "-r", fq, "-d", "tenX_v3", "-l", wl, "-c", "5000", "-tr", "4", "-o", os.path.join(tmp, out)]  # noqa: E731

    def run(cwd, out, extra):
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable] + args_of(out) + extra, cwd=cwd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(r.stdout[-2000:] + r.stderr[-2000:])
        return time.perf_counter() - t0, [l.split(" - ")[-1].replace(tmp, "TMP") for l in r.stdout.split("\n") if "Genes: " in l or "Isoforms: " in l or "Isoform EM: " in l or "Alleles: " in l or "Discovery: " in l or "Fusions: " in l]

    def pairs(name_a, a, name_b, b, what):
        walls, said = {name_a: [], name_b: []}, []
        for _ in range(args.pairs):
            for name, (cwd, extra) in ((name_a, a), (name_b, b)):
                t, lines = run(cwd, name.replace(" ", "_"), extra)
                walls[name].append(t)
                said = lines or said
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
    if args.spans:
        tx2, tx_map = os.path.join(tmp, "tx_iso.fa"), os.path.join(tmp, "tx2gene.tsv")
        _isoforms_of(tx, tx2, tx_map)
        for what, gene in (("", ["--transcripts", tx]),
                           (" --tx2gene --isoforms --isoform_em --umi_per_gene",
                            ["--transcripts", tx2, "--tx2gene", tx_map, "--isoforms", "--isoform_em", "--umi_per_gene"])):
            matrix = ["--umi_dedup"] + gene + ["--count_matrix", os.path.join(tmp, "matrix")]
            pairs("tagged_route", (ROOT, matrix + ["--tagged_reads", fa]), "from_reads", (ROOT, matrix + ["--matrix_from_reads"]),
                  "stage2 CLI from FASTQ, --umi_dedup --count_matrix%s: --matrix_from_reads against --tagged_reads" % what)
    elif args.fusions:
        matrix = tagged + ["--transcripts", tx, "--count_matrix", os.path.join(tmp, "matrix")]
        pairs("count_matrix", (ROOT, matrix), "fusions", (ROOT, matrix + ["--fusions"]),
              "stage2 CLI from FASTQ, --umi_dedup --tagged_reads --count_matrix: with --fusions against without")
    elif args.discover:
        matrix = tagged + ["--transcripts", tx, "--count_matrix", os.path.join(tmp, "matrix")]
        pairs("count_matrix", (ROOT, matrix), "discover", (ROOT, matrix + ["--discover_variants"]),
              "stage2 CLI from FASTQ, --umi_dedup --tagged_reads --count_matrix: with --discover_variants against without")
    elif args.alleles:
        var = os.path.join(tmp, "variants.tsv")
        _variants_of(tx, var)
        matrix = tagged + ["--transcripts", tx, "--count_matrix", os.path.join(tmp, "matrix")]
        pairs("count_matrix", (ROOT, matrix), "variants", (ROOT, matrix + ["--variants", var]),
              "stage2 CLI from FASTQ, --umi_dedup --tagged_reads --count_matrix: with --variants (4 sites per transcript) against without")
    elif args.isoforms:
        tx2, tx_map = os.path.join(tmp, "tx_iso.fa"), os.path.join(tmp, "tx2gene.tsv")
        _isoforms_of(tx, tx2, tx_map)
        matrix = tagged + ["--transcripts", tx2, "--tx2gene", tx_map, "--count_matrix", os.path.join(tmp, "matrix")]
        if args.em:
            pairs("isoforms", (ROOT, matrix + ["--isoforms"]), "isoform_em", (ROOT, matrix + ["--isoforms", "--isoform_em"]),
                  "stage2 CLI from FASTQ, --umi_dedup --tagged_reads --count_matrix --tx2gene --isoforms: with --isoform_em against without")
            em_split_probe(args, fa, tx2, tx_map)
        else:
            pairs("count_matrix", (ROOT, matrix), "isoforms", (ROOT, matrix + ["--isoforms"]),
                  "stage2 CLI from FASTQ, --umi_dedup --tagged_reads --count_matrix --tx2gene: with --isoforms against without")
    else:
        pairs("tagged", (ROOT, tagged), "count_matrix", (ROOT, tagged + ["--transcripts", tx, "--count_matrix", os.path.join(tmp, "matrix")]),
              "stage2 CLI from FASTQ, --umi_dedup --tagged_reads: with --count_matrix against without")
    if args.parent:
        parent = os.path.abspath(args.parent)
        pairs("parent", (parent, tagged), "flags_off", (ROOT, tagged), "stage2 CLI from FASTQ, --umi_dedup --tagged_reads: this build with the flags off against the parent commit's")
        pairs("parent_a", (parent, tagged), "parent_b", (parent, tagged), "stage2 CLI from FASTQ, --umi_dedup --tagged_reads: the parent commit's build against itself")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--device", action="store_true")
    p.add_argument("--cli", action="store_true")
    p.add_argument("--reads", type=int, default=1000000)
    p.add_argument("--tx_bases", type=int, nargs="+", default=[4000000, 100000000], help="bases of each transcriptome to measure")
    p.add_argument("--k", type=int, default=21)
    p.add_argument("--min_hits", type=int, default=3)
    p.add_argument("--isoforms", action="store_true", help="the isoform leg of --device and of --cli (DESIGN 4.20)")
    p.add_argument("--margin", type=int, default=1)
    p.add_argument("--spans", action="store_true", help="the span kernels beside the forward ones (--device), --matrix_from_reads (--cli) (DESIGN 4.25)")
    p.add_argument("--alleles", action="store_true", help="the allele leg of --device and of --cli (DESIGN 4.26)")
    p.add_argument("--discover", action="store_true", help="the discovery leg of --device and of --cli (DESIGN 4.29)")
    p.add_argument("--fusions", action="store_true", help="the fusion leg of --device and of --cli (DESIGN 4.31)")
    p.add_argument("--fusion_min_hits", type=int, default=8)
    p.add_argument("--discover_k", type=int, default=11)
    p.add_argument("--discover_min_alt", type=int, default=5)
    p.add_argument("--count_layout", default="[site][4]", help="--discover: what the record says of the library's count layout")
    p.add_argument("--em", action="store_true", help="k_em_tcc alone; with --cli --isoforms the --isoform_em leg (DESIGN 4.21)")
    p.add_argument("--em_problems", type=int, default=1000000)
    p.add_argument("--em_wide", type=int, default=100000)
    p.add_argument("--em_eps", type=float, default=1e-3)
    p.add_argument("--em_max_iter", type=int, default=1000)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--cli_reads", type=int, default=1000000)
    p.add_argument("--pairs", type=int, default=3)
    p.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.device:
        (device_probe_fusions if args.fusions else device_probe_discover if args.discover else device_probe_alleles if args.alleles else device_probe_spans if args.spans else device_probe_iso if args.isoforms else device_probe)(args)
    if args.em and not args.cli:
        em_probe(args)
    if args.cli:
        cli_probe(args)


if __name__ == "__main__":
    main()
