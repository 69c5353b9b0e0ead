#!/usr/bin/env python3
"""Measurements of stage 1's --trimmed_reads, one JSON line each to --out (and stdout).

    python tools/trim_probe.py --device [--reads 1000000] --out profiles/r10_trim.jsonl
        synthetic reads with a TSO, device-resident: the extraction step (bdg_extract_batch_dev) and the trim behind it
        (bdg_trim_batch_dev), each 3 warm-ups and 10 timed calls with device events, median.
    python tools/trim_probe.py --cli [--cli_reads 2000000] [--pairs 8] --out ...
        the stage-1 command line on a FASTQ of such reads with and without --trimmed_reads, as alternating pairs of fresh
        processes: median wall clock of each and the ratio.
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


def device_probe(args):
    import torch
    from badger_amd import _native, synth
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    ctx.set_stream(0)
    wl = synth.make_whitelist(737280)
    for tso in (True, False):
        n = args.reads
        b, o = synth.make_reads(n, wl, seed=1, device="cuda", tso=tso)
        total = int(o[-1])
        d_bases = torch.zeros((total + 15) // 16 * 16 + 64, dtype=torch.uint8, device=dev)
        d_bases[:total] = b
        d_recs = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
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
        for score in (20, 8):
            tr = timed(lambda: ctx.trim_batch_dev(d_bases, o, n, d_recs, score, d_out))
            res = d_out.cpu().numpy().view(_native.TRIM_DTYPE)
            recs = d_recs.cpu().numpy().view(_native.REC_DTYPE)
            emit(args.out, {"what": "k_trim_reads behind the extraction step, device-resident", "reads": n, "synthetic_tso": tso,
                            "tso_min_score": score, "eligible": int(((recs["valid"] == 1) & (recs["polyT"] >= 0)).sum()),
                            "emitted": int(((res["flags"] & 1) != 0).sum()), "tso_cut": int(((res["flags"] & 2) != 0).sum()),
                            "trim_ms_median": round(float(np.median(tr)), 4), "trim_ms_min": round(min(tr), 4), "trim_ms_max": round(max(tr), 4),
                            "extract_ms_median": round(float(np.median(ext)), 4), "extract_ms_min": round(min(ext), 4),
                            "trim_over_extract": round(float(np.median(tr)) / float(np.median(ext)), 3), "warmups": 3, "timed": args.reps,
                            "version": ctx.lib.bdg_version().decode()})
        del d_bases, d_recs, d_out, b, o


def cli_probe(args):
    import torch  # noqa: F401
    from badger_amd import synth
    tmp = tempfile.mkdtemp(prefix="trim_probe_", dir=os.environ.get("TMPDIR", "/tmp"))
    n = args.cli_reads
    wl = synth.make_whitelist(737280)
    fq = os.path.join(tmp, "reads.fastq")
    with open(fq, "wb") as f:
        done = 0
        while done < n:
            k = min(250000, n - done)
            b, o = synth.make_reads(k, wl, seed=1 + done // 250000, device="cuda", tso=True)
            b, o = b.cpu().numpy(), o.cpu().numpy()
            parts = []
            for i in range(k):
                s = b[o[i]:o[i + 1]].tobytes()
                parts.append(b"@read_%d\n%s\n+\n%s\n" % (done + i, s, b"I" * len(s)))
            f.write(b"".join(parts))
            done += k
    base = [sys.executable, "-m", "badger_amd.extract_raw_barcodes", "--mode", "tenX_v3", "-i", fq, "-t", "16", "-o", os.path.join(tmp, "o.tsv")]
    fa = os.path.join(tmp, "o.fa")
    walls = {"off": [], "on": []}
    subprocess.run(base, cwd=ROOT, capture_output=True, text=True, timeout=600)                     # (page cache, clocks)
    for _ in range(args.pairs):
        for name, extra in (("off", []), ("on", ["--trimmed_reads", fa])):
            t0 = time.perf_counter()
            r = subprocess.run(base + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
            walls[name].append(time.perf_counter() - t0)
            if r.returncode != 0:
                raise SystemExit(r.stderr[-2000:] + r.stdout[-2000:])
    m0, m1 = float(np.median(walls["off"])), float(np.median(walls["on"]))
    emit(args.out, {"what": "stage-1 CLI on a FASTQ, --trimmed_reads on against off, alternating pairs of fresh processes", "reads": n,
                    "pairs": args.pairs, "fastq_bytes": os.path.getsize(fq), "tsv_bytes": os.path.getsize(os.path.join(tmp, "o.tsv")),
                    "trimmed_bytes": os.path.getsize(fa), "off_s": [round(x, 3) for x in walls["off"]], "on_s": [round(x, 3) for x in walls["on"]],
                    "median_off_s": round(m0, 3), "median_on_s": round(m1, 3), "ratio": round(m1 / m0, 3)})
    for p in (fq, fa, os.path.join(tmp, "o.tsv"), os.path.join(tmp, "o.tsv.stats")):
        if os.path.exists(p):
            os.remove(p)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--device", action="store_true")
    p.add_argument("--cli", action="store_true")
    p.add_argument("--reads", type=int, default=1000000)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--cli_reads", type=int, default=2000000)
    p.add_argument("--pairs", type=int, default=8)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.device:
        device_probe(args)
    if args.cli:
        cli_probe(args)


if __name__ == "__main__":
    main()
