#!/usr/bin/env python3
"""Measurements of the per-molecule consensus, one JSON line each to --out (and stdout).

    python tools/consensus_probe.py --device [--reads 1000000] [--band 64 128 256] [--long_reads 100000] --out profiles/r20_consensus_band.jsonl
        bdg_consensus_dev alone, device-resident: reads in molecules of about 5 reads of about 900 bases (600 .. 1,200, the members
        cut by up to a quarter at the end away from the anchor, synth's error rates): wall time per call (with the call's own
        read-back of the offsets and its planning on the host), and the two kernels from the library's event timers, in every
        --band asked for (bdg_consensus_set_band; 64 alone by default).  With --long_reads N a second workload behind it: N reads
        in molecules of 3,000 .. 6,000 bases, where the band decides how many members vote (--reads 0 leaves the first one out).
    python tools/consensus_probe.py --cli [--cli_reads 1000000] [--pairs 3] [--parent DIR] --out ...
        the stage-2 command line on a FASTQ file in which every read of synth's error model comes with four siblings (the same
        read with 3 % substitutions between its ends, so that barcode and UMI stay), as alternating pairs of fresh processes:
        --tagged_reads --umi_dedup with --molecule_consensus against without; and, with --parent DIR (a built checkout of the
        parent commit), this build with the flag off against the parent, beside parent against parent.
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


def molecules(n_reads, seed=1, per=5, lo=600, hi=1200, chunk=20000):
    """-> (bases uint8, seq_off uint64, grp_off uint64): groups of `per` reads, the untruncated read first"""
    rng = np.random.default_rng(seed)
    parts, lens = [], []
    for g0 in range(0, n_reads // per, chunk):
        m = min(chunk, n_reads // per - g0)
        L = rng.integers(lo, hi + 1, m)
        cut = rng.integers(0, L[:, None] // 4 + 1, (m, per))
        cut[:, 0] = 0
        rl = (L[:, None] - cut).ravel()                               # read lengths before errors: the last rl bases of the truth
        t_off = np.concatenate([[0], np.cumsum(L)])
        truth = rng.integers(0, 4, int(t_off[-1]), dtype=np.uint8)
        r_off = np.concatenate([[0], np.cumsum(rl)])
        rid = np.repeat(np.arange(m * per), rl)
        pos = np.arange(int(r_off[-1])) - r_off[rid]
        codes = truth[t_off[rid // per] + np.repeat(cut.ravel(), rl) + pos]
        u = rng.random(len(codes))
        is_del, is_sub, is_ins = u < 0.03, (u >= 0.03) & (u < 0.06), (u >= 0.06) & (u < 0.08)
        codes = np.where(is_sub, (codes + rng.integers(1, 4, len(codes), dtype=np.uint8)) & 3, codes).astype(np.uint8)
        cnt = (~is_del).astype(np.int64) + is_ins
        at = np.cumsum(cnt) - cnt
        out = np.empty(int(cnt.sum()), dtype=np.uint8)
        out[at[~is_del]] = codes[~is_del]
        out[(at + ~is_del)[is_ins]] = rng.integers(0, 4, int(is_ins.sum()), dtype=np.uint8)
        new_off = np.concatenate([at, [int(cnt.sum())]])[r_off]
        parts.append(ACGT[out])
        lens.append(np.diff(new_off))
    lens = np.concatenate(lens)
    # the longest read of a group first (the election): swap it with the group's first
    lens2 = lens.reshape(-1, per)
    seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    bases = np.concatenate(parts)
    longest = lens2.argmax(axis=1)
    order = np.arange(len(lens)).reshape(-1, per)
    rows = np.arange(len(order))
    order[rows, 0], order[rows, longest] = order[rows, longest].copy(), order[rows, 0].copy()
    order = order.ravel()
    new_lens = lens[order]
    new_off = np.concatenate([[0], np.cumsum(new_lens)]).astype(np.uint64)
    src = np.repeat(seq_off[:-1][order].astype(np.int64) - new_off[:-1].astype(np.int64), new_lens) + np.arange(int(new_off[-1]))
    return bases[src], new_off, (np.arange(len(order) // per + 1) * per).astype(np.uint64)


def device_probe(args):
    from badger_amd import _native
    _native.PRELOAD_TORCH = False
    ctx = _native.default_context(0)
    if args.reads:
        device_workload(args, _native, ctx, "molecules of 600 .. 1,200 bases", molecules(args.reads), (_native.CONS_ANCHOR_END, _native.CONS_ANCHOR_START))
    if args.long_reads:
        device_workload(args, _native, ctx, "molecules of 3,000 .. 6,000 bases", molecules(args.long_reads, seed=2, lo=3000, hi=6000, chunk=2000),
                        (_native.CONS_ANCHOR_END,))


def device_workload(args, _native, ctx, workload, arrays, anchors):
    bases, seq_off, grp_off = arrays
    n_seqs, n_groups = len(seq_off) - 1, len(grp_off) - 1
    out_off = _native.consensus_out_offsets(seq_off, grp_off)
    d = [_native.DeviceArray.from_host(ctx, a) for a in (bases, seq_off, grp_off, out_off)]
    d_out = _native.DeviceArray(ctx, int(out_off[-1]), np.uint8)
    d_len, d_voted = _native.DeviceArray(ctx, n_groups, np.uint32), _native.DeviceArray(ctx, n_groups, np.uint32)
    d_recs = _native.DeviceArray(ctx, n_seqs * 3, np.uint32)
    for band, anchor in ((b, a) for b in args.band for a in anchors):
        ctx.consensus_set_band(band)
        call = lambda: ctx.consensus_dev(d[0], d[1], n_seqs, d[2], n_groups, anchor, 20, d[3], d_out, d_len, d_voted, d_recs)  # noqa: E731
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
        kt = {k: round(v[1], 4) for k, v in ctx.profile_read().items() if k.startswith("k_cons")}
        ctx.profile(False)
        recs = d_recs.to_host().view(_native.CONSENSUS_DTYPE)
        flags = recs["flags"]
        emit(args.out, {"what": "bdg_consensus_dev, device-resident", "workload": workload, "band": band, "anchor": "end" if anchor else "start", "reads": n_seqs,
                        "molecules": n_groups, "bases": int(seq_off[-1]), "accepted": int((flags & 1 != 0).sum()),
                        "rejected_by_distance": int((flags & 2 != 0).sum()), "rejected_by_band": int((flags & 4 != 0).sum()),
                        "consensus_bases": int(d_len.to_host().sum()), "call_ms_median": round(1e3 * float(np.median(times)), 3),
                        "call_ms_min": round(1e3 * min(times), 3), "kernel_ms": kt,
                        "kernel_ms_per_1M_reads": {k: round(v * 1e6 / n_seqs, 3) for k, v in kt.items()}})
    ctx.consensus_set_band(_native.CONS_BAND_DEFAULT)
    for a in d + [d_out, d_len, d_voted, d_recs]:
        a.free()


def _fastq(n, tmp):
    """n reads: n / 5 of the error model with a TSO (5,000 cells), each with four siblings -> FASTQ path, whitelist path"""
    import torch  # noqa: F401  (synth.make_reads on the device)
    from cli_throughput import helper
    from badger_amd import synth
    L = helper(tmp)
    wl = synth.make_whitelist(6000)
    with open(os.path.join(tmp, "wl.txt"), "w") as f:
        f.write("\n".join(synth.rank_to_str(int(r)) for r in wl) + "\n")
    fq = os.path.join(tmp, "reads.fastq")
    rng = np.random.default_rng(4)
    done = 0
    while done < n:
        k = min(100000, (n - done + 4) // 5)
        tb, to = synth.make_reads(k, wl, seed=1 + done, device="cuda", tso=True)
        bases, off = tb.cpu().numpy(), to.cpu().numpy().astype(np.int64)
        off64 = off.astype(np.uint64)                                 # (kept alive across the native calls)
        lens = np.diff(off)
        pos = np.arange(len(bases)) - np.repeat(off[:-1], lens)
        inner = (pos >= 160) & (pos < np.repeat(lens, lens) - 160)
        for _ in range(5):                                            # the read, then four siblings
            assert L.fq_append(fq.encode(), bases.ctypes.data, off64.ctypes.data, k, done, b"read_") > 0
            done += k
            sub = inner & (rng.random(len(bases)) < 0.03)
            code = np.searchsorted(ACGT, bases[sub])
            bases = bases.copy()
            bases[sub] = ACGT[(code + rng.integers(1, 4, int(sub.sum()))) & 3]
    return fq, os.path.join(tmp, "wl.txt")


def cli_probe(args):
    tmp = tempfile.mkdtemp(prefix="consensus_probe_")
    fq, wl = _fastq(args.cli_reads, tmp)
    args_of = lambda out: ["-m", "badger_amd.badger", "-r", fq, "-d", "tenX_v3", "-l", wl, "-c", "5000", "-tr", "4", "-o", os.path.join(tmp, out)]  # noqa: E731

    def run(cwd, out, extra):
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable] + args_of(out) + extra, cwd=cwd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(r.stdout[-2000:] + r.stderr[-2000:])
        return time.perf_counter() - t0, [l.split(" - ")[-1] for l in r.stdout.split("\n") if "Consensus: " in l]

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
                        "ratio_%s_over_%s" % (name_b, name_a): round(mb / ma, 3), "log": said})

    fa, cons = os.path.join(tmp, "tagged.fa"), os.path.join(tmp, "consensus.fa")
    tagged = ["--umi_dedup", "--tagged_reads", fa]
    run(ROOT, "warm", tagged)                                          # (the file into the page cache, the runtime's caches)
    pairs("tagged", (ROOT, tagged), "consensus", (ROOT, tagged + ["--molecule_consensus", cons]),
          "stage2 CLI from FASTQ, --umi_dedup --tagged_reads: with --molecule_consensus against without")
    if args.parent:
        parent = os.path.abspath(args.parent)
        pairs("parent", (parent, tagged), "flag_off", (ROOT, tagged), "stage2 CLI from FASTQ, --umi_dedup --tagged_reads: this build with the flag off against the parent commit's")
        pairs("parent_a", (parent, tagged), "parent_b", (parent, tagged), "stage2 CLI from FASTQ, --umi_dedup --tagged_reads: the parent commit's build against itself")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--device", action="store_true")
    p.add_argument("--cli", action="store_true")
    p.add_argument("--reads", type=int, default=1000000)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--band", type=int, nargs="+", choices=(64, 128, 256), default=[64], help="the bands to measure, each in turn")
    p.add_argument("--long_reads", type=int, default=0, help="reads of the long-molecule workload (3,000 .. 6,000 bases); 0: none")
    p.add_argument("--cli_reads", type=int, default=1000000)
    p.add_argument("--pairs", type=int, default=3)
    p.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.device:
        device_probe(args)
    if args.cli:
        cli_probe(args)


if __name__ == "__main__":
    main()
