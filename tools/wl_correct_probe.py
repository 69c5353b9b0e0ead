#!/usr/bin/env python3
"""Measurements of the abundance-weighted whitelist correction (bdg_nearest16_correct, stage 1's --bc_correct), one JSON
object per line:

  kernels   1 M queries x the 737,280-entry list, max_ed 2 (probe path): device time of k_wl_support and k_wl_resolve from
            the library's per-kernel event timers, for synthetic-read-like queries ("mixed") and for a hot cell - every
            query the same entry, so that every increment goes to one address ("hot") - with the support kernel's wave
            aggregation on (BADGER_AMD_SUPPORT_PEEL unset: 4 rounds) and off (0); each setting in a child process of its own
  memory    device bytes per read that a run keeps until its last chunk, and what the resolve adds
  cli       the stage-1 command line on N synthetic FASTQ reads, -b against -b --bc_correct, alternating pairs, process start
            to files on disk
  accuracy  recall / precision of corrected_barcode and whitelist_barcode for --bc_edit_bits 3, 5, 7 on synthetic reads with
            known cells against a 3 M-entry list (tests/test_wl_correct_gpu.py's accuracy_run)

Builder tool (the numbers go to DESIGN.md / profiles/), not the bench contract.

    python tools/wl_correct_probe.py [--cli-reads N] [--cli-pairs P] [--skip-kernels] [--skip-cli] [--skip-accuracy]
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from badger_amd import _native, common, synth  # noqa: E402

NW = 737280
NQ = 1000000


def _queries(wl, n, seed):
    """like the barcodes of synthetic reads: 60 % exact copies of entries of a few thousand cells, 30 % of them with one
    substitution, 10 % uniform"""
    rng = np.random.default_rng(seed)
    cells = wl[rng.choice(len(wl), size=5000, replace=False)]
    q = cells[rng.integers(0, len(cells), size=n)]
    pos = rng.integers(0, 16, size=n).astype(np.uint32)
    sub = ((q & ~(np.uint32(3) << (2 * pos))) | (rng.integers(0, 4, size=n).astype(np.uint32) << (2 * pos))).astype(np.uint32)
    u = rng.random(n)
    rnd = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    return np.where(u < 0.6, q, np.where(u < 0.9, sub, rnd)).astype(np.uint32)


def kernel_child(kind):
    ctx = _native.Context(0)
    wl = synth.make_whitelist(NW)
    q = _queries(wl, NQ, 3) if kind == "mixed" else np.full(NQ, wl[12345], np.uint32)
    ctx.nearest16_correct(q, wl, 2)                              # warm: index, workspaces
    ctx.profile(True)
    ctx.profile_reset()
    reps = 5
    for _ in range(reps):
        res = ctx.nearest16_correct(q, wl, 2)
    prof = ctx.profile_read()
    ctx.profile(False)
    st = np.bincount(res[4], minlength=5).tolist()
    per = {k: round(v[1] / reps, 4) for k, v in prof.items() if v[0] and (k.startswith("k_wl") or k.startswith("k_nearest"))}
    print(json.dumps({"part": "kernels", "queries": kind, "nq": NQ, "nw": NW, "max_ed": 2,
                      "support_peel": os.environ.get("BADGER_AMD_SUPPORT_PEEL", "4"),
                      "k_wl_support_ms": per.get("k_wl_support"), "k_wl_resolve_ms": per.get("k_wl_resolve"),
                      "match_kernels_ms": {k: v for k, v in per.items() if k.startswith("k_nearest")},
                      "status_counts": dict(zip(("none", "exact", "corrected", "ambiguous", "truncated"), st))}), flush=True)
    ctx.close()


def kernel_part():
    for kind in ("mixed", "hot"):
        for peel in (None, "0"):
            env = dict(os.environ)
            env.pop("BADGER_AMD_SUPPORT_PEEL", None)
            if peel is not None:
                env["BADGER_AMD_SUPPORT_PEEL"] = peel
            subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-child", kind], env=env, check=True, timeout=300)


def memory_part():
    print(json.dumps({"part": "memory", "kept_bytes_per_read": 42, "kept_layout": "idx u32 x 8 | ed u8 x 8 | n_within u16",
                      "resolve_bytes_per_read": 12, "capacity": "doubles from 2^20 reads: at most 2 x 42 bytes per read allocated, "
                      "3 x 42 for a moment while it grows",
                      "reads_12_5M_kept_MB": round(12.5e6 * 42 / 1e6), "reads_12_5M_peak_MB": round((2 ** 24 * 42 + 12.5e6 * 12) / 1e6)}),
          flush=True)


def cli_part(n, pairs=3):
    import cli_throughput as ct
    tmp = os.environ.get("TMPDIR", "/tmp")
    L = ct.helper(tmp)
    wl = synth.make_whitelist(NW)
    wl_path = os.path.join(tmp, "wl737k.txt")
    with open(wl_path, "w") as f:
        f.write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    fq = os.path.join(tmp, "corr_cli_reads.fastq")
    if os.path.exists(fq):
        os.remove(fq)
    done = 0
    while done < n:
        k = min(ct.SLAB, n - done)
        tb, to = synth.make_reads(k, wl, seed=1 + done // ct.SLAB, device="cuda")
        bases, off = tb.cpu().numpy(), to.cpu().numpy().astype(np.uint64)
        assert L.fq_append(fq.encode(), bases.ctypes.data, off.ctypes.data, k, done, b"read_") > 0
        done += k
    timing = os.path.join(tmp, "corr_cli_timing.jsonl")
    out = os.path.join(tmp, "corr_cli_out.tsv")
    for rep in range(pairs):                                  # alternating: the spread shows in the pairs
        for extra in (("-b", wl_path), ("-b", wl_path, "--bc_correct")):
            wall, br = ct.run_cli(fq, out, 16, timing, extra)
            row = {"part": "cli", "reads": n, "rep": rep, "bc_correct": len(extra) > 2, "wall_s": round(wall, 3), "pipeline": br}
            if len(extra) > 2:
                row["corrected_lines"] = sum(1 for _ in open(out + ".corrected.tsv", "rb"))
                row["stats_tail"] = open(out + ".stats").read().strip().split("\n")[-2:]
            print(json.dumps(row), flush=True)
    for p in (fq, out, out + ".stats", out + ".corrected.tsv"):
        if os.path.exists(p):
            os.remove(p)


def accuracy_part():
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_wl_correct_gpu import accuracy_run
    with tempfile.TemporaryDirectory() as d:
        import pathlib
        acc = accuracy_run(pathlib.Path(d))
    for bits, a in acc.items():
        print(json.dumps(dict(part="accuracy", edit_bits=bits, n_wl=3000000, **{k: (round(v, 5) if isinstance(v, float) else v)
                                                                                   for k, v in a.items()})), flush=True)


def main():
    args = sys.argv[1:]
    if "--kernel-child" in args:
        kernel_child(args[args.index("--kernel-child") + 1])
        return
    n_cli = int(args[args.index("--cli-reads") + 1]) if "--cli-reads" in args else 2000000
    print(json.dumps({"version": _native.load().bdg_version().decode()}), flush=True)
    t0 = time.perf_counter()
    if "--skip-kernels" not in args:
        kernel_part()
        memory_part()
    if "--skip-cli" not in args:
        cli_part(n_cli, int(args[args.index("--cli-pairs") + 1]) if "--cli-pairs" in args else 3)
    if "--skip-accuracy" not in args:
        accuracy_part()
    print(json.dumps({"done_s": round(time.perf_counter() - t0, 1)}), flush=True)


if __name__ == "__main__":
    main()
