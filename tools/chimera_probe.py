#!/usr/bin/env python3
"""Measurements of stage 1's --chimera_cut, one JSON line each to --out (and stdout).

    python tools/chimera_probe.py --rates [--rate_reads 60000] --out profiles/r11_chimera.jsonl
        no GPU: the false-cut and sensitivity tables behind BDG_CHIMERA_MAX_ED_DEFAULT, with the batch checker.  Chimera-free
        reads of synth.make_reads(tso=True), on which every hit is false; and chimeras made of pairs of such reads (so both
        molecules went through the error model), joined head to tail and head to head, on either strand.
    python tools/chimera_probe.py --device [--reads 1000000] --out ...
        synthetic reads, about 3 % of them two reads joined, device-resident: the extraction step, the trim and the search
        behind it, each 3 warm-ups and 10 timed calls with device events, median.
    python tools/chimera_probe.py --cli [--cli_reads 2000000] [--pairs 8] --out ...
        the stage-1 command line on a FASTQ of such reads: --trimmed_reads --chimera_cut against --trimmed_reads alone, and both
        flags off (the number to hold against the commit before), as alternating fresh processes: median and spread.
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


def rates_probe(args):
    from badger_amd import chimera, synth, trim
    from oracle import pyoracle as orc
    eds = list(range(chimera.MAX_ED_RANGE[1] + 1))
    wl = synth.make_whitelist(3000)
    b, o = synth.make_reads(args.rate_reads, wl, seed=1311, umi_len=12, tso=True)
    reads = synth.reads_to_list(b, o)
    bases, off = synth.list_to_reads(reads)
    recs = orc.extract_batch(bases, off, 12, threads=16)
    tr = trim.trim_batch(bases, off, recs)
    emitted = int(((tr["flags"] & trim.TRIM_EMIT) != 0).sum())
    false = [int((c["flags"] != 0).sum()) for c in chimera.chimera_batch_multi(bases, off, recs, tr, eds)]
    emit(args.out, {"what": "false cuts: chimera-free reads of the error model with a hit, per max_ed 0 .. 6", "reads": args.rate_reads,
                    "emitted": emitted, "reads_with_a_hit": false, "fraction": [round(f / emitted, 6) for f in false],
                    "cap": 0.001, "largest_max_ed_within_cap": max(e for e in eds if false[e] * 1000 <= emitted)})
    strand = lambda i: trim.revcomp(reads[i]) if recs[i]["flags"] & 1 else reads[i]      # noqa: E731
    m = min(args.rate_reads // 2, 5000)
    ch = []
    for k in range(m):
        s = strand(2 * k) + (strand(2 * k + 1) if k & 1 else trim.revcomp(strand(2 * k + 1)))
        ch.append(trim.revcomp(s) if k & 2 else s)
    cb, co = synth.list_to_reads(ch)
    crecs = orc.extract_batch(cb, co, 12, threads=16)
    ctr = trim.trim_batch(cb, co, crecs)
    cem = int(((ctr["flags"] & trim.TRIM_EMIT) != 0).sum())
    found = [int((c["flags"] != 0).sum()) for c in chimera.chimera_batch_multi(cb, co, crecs, ctr, eds)]
    emit(args.out, {"what": "sensitivity: planted chimeras (pairs of error-model reads, head to tail / head to head) with a hit", "planted": m,
                    "emitted": cem, "found": found, "fraction": [round(f / cem, 4) for f in found]})


def _merged(o, every):
    """offsets with every `every`-th boundary dropped: the two reads around it become one"""
    import torch
    keep = torch.ones(len(o), dtype=torch.bool, device=o.device)
    keep[every:len(o) - 1:every] = False
    return o[keep]


def device_probe(args):
    import torch
    from badger_amd import _native, synth
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    ctx.set_stream(0)
    wl = synth.make_whitelist(737280)
    b, o = synth.make_reads(args.reads, wl, seed=1, device="cuda", tso=True)
    o = _merged(o, 33)                                                    # about 3 % of the reads are two molecules
    n, total = len(o) - 1, int(o[-1])
    d_bases = torch.zeros((total + 15) // 16 * 16 + 64, dtype=torch.uint8, device=dev)
    d_bases[:total] = b
    d_recs = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_trim = torch.zeros(n * 12, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(n * 12, dtype=torch.uint8, device=dev)

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
    assert ctx.extract_status()[0] == 0
    tr = timed(lambda: ctx.trim_batch_dev(d_bases, o, n, d_recs, 20, d_trim))
    t = d_trim.cpu().numpy().view(_native.TRIM_DTYPE)
    emitted = (t["flags"] & 1) != 0
    for ed in (_native.CHIMERA_MAX_ED_DEFAULT, 0, 6):
        ch = timed(lambda: ctx.chimera_batch_dev(d_bases, o, n, d_recs, d_trim, ed, d_out))
        res = d_out.cpu().numpy().view(_native.CHIMERA_DTYPE)
        med = lambda v: round(float(np.median(v)), 4)                      # noqa: E731
        emit(args.out, {"what": "k_chimera_search behind extraction and trim, device-resident", "reads": n, "max_ed": ed,
                        "emitted": int(emitted.sum()), "interval_bases": int((t["cdna_end"][emitted].astype(np.int64) - t["cdna_start"][emitted]).sum()),
                        "reads_with_a_hit": int((res["flags"] != 0).sum()),
                        "chimera_ms_median": med(ch), "chimera_ms_min": round(min(ch), 4), "chimera_ms_max": round(max(ch), 4),
                        "trim_ms_median": med(tr), "extract_ms_median": med(ext), "chimera_over_extract": round(med(ch) / med(ext), 3),
                        "chimera_ms_per_million_reads": round(med(ch) * 1e6 / n, 4), "warmups": 3, "timed": args.reps,
                        "version": ctx.lib.bdg_version().decode()})


def cli_probe(args):
    import torch  # noqa: F401
    from badger_amd import synth
    tmp = tempfile.mkdtemp(prefix="chimera_probe_", dir=os.environ.get("TMPDIR", "/tmp"))
    n = args.cli_reads
    wl = synth.make_whitelist(737280)
    fq = os.path.join(tmp, "reads.fastq")
    written = 0
    with open(fq, "wb") as f:
        done = 0
        while done < n:
            k = min(250000, n - done)
            b, o = synth.make_reads(k, wl, seed=1 + done // 250000, device="cuda", tso=True)
            o = _merged(o, 33)
            b, o = b.cpu().numpy(), o.cpu().numpy()
            parts = []
            for i in range(len(o) - 1):
                s = b[o[i]:o[i + 1]].tobytes()
                parts.append(b"@read_%d\n%s\n+\n%s\n" % (written + i, s, b"I" * len(s)))
            f.write(b"".join(parts))
            written += len(o) - 1
            done += k
    tsv, fa = os.path.join(tmp, "o.tsv"), os.path.join(tmp, "o.fa")
    base = [sys.executable, "-m", "badger_amd.extract_raw_barcodes", "--mode", "tenX_v3", "-i", fq, "-t", "16", "-o", tsv]
    modes = (("off", []), ("trim", ["--trimmed_reads", fa]), ("trim_chimera", ["--trimmed_reads", fa, "--chimera_cut"]))
    walls = {name: [] for name, _ in modes}
    subprocess.run(base, cwd=ROOT, capture_output=True, text=True, timeout=600)                     # (page cache, clocks)
    for _ in range(args.pairs):
        for name, extra in modes:
            t0 = time.perf_counter()
            r = subprocess.run(base + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
            walls[name].append(time.perf_counter() - t0)
            if r.returncode != 0:
                raise SystemExit(r.stderr[-2000:] + r.stdout[-2000:])
    med = {k: float(np.median(v)) for k, v in walls.items()}
    emit(args.out, {"what": "stage-1 CLI on a FASTQ: flags off / --trimmed_reads / --trimmed_reads --chimera_cut, alternating fresh processes",
                    "reads": written, "rounds": args.pairs, "fastq_bytes": os.path.getsize(fq),
                    "seconds": {k: [round(x, 3) for x in v] for k, v in walls.items()}, "median_s": {k: round(v, 3) for k, v in med.items()},
                    "chimera_over_trim": round(med["trim_chimera"] / med["trim"], 3)})
    for p in (fq, fa, tsv, tsv + ".stats"):
        if os.path.exists(p):
            os.remove(p)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rates", action="store_true")
    p.add_argument("--device", action="store_true")
    p.add_argument("--cli", action="store_true")
    p.add_argument("--rate_reads", type=int, default=60000)
    p.add_argument("--reads", type=int, default=1000000)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--cli_reads", type=int, default=2000000)
    p.add_argument("--pairs", type=int, default=8)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.rates:
        rates_probe(args)
    if args.device:
        device_probe(args)
    if args.cli:
        cli_probe(args)


if __name__ == "__main__":
    main()
