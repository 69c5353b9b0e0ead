#!/usr/bin/env python3
"""Measurements of the k-nearest whitelist match (bdg_nearest16_topk), one JSON object per line:

  probe   1 M queries x the 737,280-entry list, max_ed 2, probe path (algo 2): top-k (k = 1 and 8) against the best-hit
          call, device time from the library's per-kernel event timers; slot 0 compared with the best-hit answer
  coop    4,096 queries x the same list, cooperative kernel (algo 3), max_ed 2 and 3: top-k (k = 8) against best-hit
  cli     the stage-1 command line on N synthetic FASTQ reads with -b, without and with --bc_candidates 8, alternating,
          process start to TSV on disk

Builder tool (the numbers go to DESIGN.md / profiles/), not the bench contract.

    python tools/nearest_topk_probe.py [--cli-reads N] [--skip-cli]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from badger_amd import _native, common, synth  # noqa: E402
from nearest_coop_probe import queries  # noqa: E402

NW = 737280


def _timed(ctx, call, reps):
    """mean device time per call of every nearest kernel the call launched, summed (ms), and the per-kernel table"""
    ctx.profile(True)
    ctx.profile_only(None)
    call()                                                       # warm: index, plan, workspace
    ctx.profile_reset()
    for _ in range(reps):
        call()
    prof = ctx.profile_read()
    ctx.profile(False)
    per = {k: round(v[1] / reps, 4) for k, v in prof.items() if k.startswith("k_nearest") and v[0]}
    return round(sum(per.values()), 4), per


def _best_arrays(ctx, n):
    return (_native.DeviceArray(ctx, (n,), np.uint32), _native.DeviceArray(ctx, (n,), np.uint8),
            _native.DeviceArray(ctx, (n,), np.uint16))


def _topk_arrays(ctx, n, k):
    return (_native.DeviceArray(ctx, (n * k,), np.uint32), _native.DeviceArray(ctx, (n * k,), np.uint8),
            _native.DeviceArray(ctx, (n,), np.uint16))


def kernel_parts(ctx):
    wl = synth.make_whitelist(NW)
    ctx.whitelist_load(wl)
    for part, algo, nq, max_eds, ks, reps in (("probe", 2, 1000000, (2,), (1, 8), 10), ("coop", 3, 4096, (2, 3), (8,), 3)):
        q = queries(wl, nq, nq)
        d_q = _native.DeviceArray.from_host(ctx, q)
        ctx.nearest16_set_algo(algo)
        for max_ed in max_eds:
            best = _best_arrays(ctx, nq)
            ms_best, per_best = _timed(ctx, lambda: ctx.nearest16_dev(d_q, nq, max_ed, *best), reps)
            bi, be = best[0].to_host(), best[1].to_host()
            for k in ks:
                outs = _topk_arrays(ctx, nq, k)
                ms_k, per_k = _timed(ctx, lambda: ctx.nearest16_topk_dev(d_q, nq, max_ed, k, *outs), reps)
                ti = outs[0].to_host().reshape(nq, k)
                te = outs[1].to_host().reshape(nq, k)
                row = {"part": part, "algo": algo, "nq": nq, "nw": NW, "max_ed": max_ed, "k": k,
                       "best_hit_ms": ms_best, "topk_ms": ms_k, "ratio": round(ms_k / ms_best, 2) if ms_best else None,
                       "best_hit_kernels": per_best, "topk_kernels": per_k,
                       "slot0_equals_best_hit": bool((ti[:, 0] == bi).all() and (te[:, 0] == be).all())}
                print(json.dumps(row), flush=True)
                for a in outs:
                    a.free()
            for a in best:
                a.free()
        d_q.free()
    ctx.nearest16_set_algo(0)


def cli_part(n):
    import cli_throughput as ct
    tmp = os.environ.get("TMPDIR", "/tmp")
    L = ct.helper(tmp)
    wl = synth.make_whitelist(NW)
    wl_path = os.path.join(tmp, "wl737k.txt")
    with open(wl_path, "w") as f:
        f.write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    fq = os.path.join(tmp, "topk_cli_reads.fastq")
    if os.path.exists(fq):
        os.remove(fq)
    done = 0
    while done < n:
        k = min(ct.SLAB, n - done)
        tb, to = synth.make_reads(k, wl, seed=1 + done // ct.SLAB, device="cuda")
        bases, off = tb.cpu().numpy(), to.cpu().numpy().astype(np.uint64)
        assert L.fq_append(fq.encode(), bases.ctypes.data, off.ctypes.data, k, done, b"read_") > 0
        done += k
    timing = os.path.join(tmp, "topk_cli_timing.jsonl")
    out = os.path.join(tmp, "topk_cli_out.tsv")
    for rep in range(2):                                      # alternating, twice: the spread shows in the pairs
        for extra in (("-b", wl_path), ("-b", wl_path, "--bc_candidates", "8")):
            wall, br = ct.run_cli(fq, out, 16, timing, extra)
            rows = sum(1 for _ in open(out, "rb"))
            print(json.dumps({"part": "cli", "reads": n, "rep": rep, "bc_candidates": 8 if len(extra) > 2 else 0,
                              "wall_s": round(wall, 3), "lines": rows, "pipeline": br}), flush=True)
    for p in (fq, out, out + ".stats"):
        if os.path.exists(p):
            os.remove(p)


def main():
    args = sys.argv[1:]
    n_cli = int(args[args.index("--cli-reads") + 1]) if "--cli-reads" in args else 2000000
    print(json.dumps({"version": _native.load().bdg_version().decode()}), flush=True)
    ctx = _native.Context(0)
    t0 = time.perf_counter()
    kernel_parts(ctx)
    ctx.close()
    if "--skip-cli" not in args:
        cli_part(n_cli)
    print(json.dumps({"done_s": round(time.perf_counter() - t0, 1)}), flush=True)


if __name__ == "__main__":
    main()
