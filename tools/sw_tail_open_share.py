#!/usr/bin/env python3
"""How many queue-A clusters does k_sw_clusters' tail certificate (tests/sw_bound_cases.py) leave open?  Host only.
The first --reads reads of the bench batch (synth.make_reads(..., seed=1)), their queue-A clusters in read order (the device's
queue order differs by the scan's scheduling; 128 consecutive clusters make a wave, 512 a block).  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import sw_bound_cases as sb                                        # noqa: E402
from badger_amd import synth                                       # noqa: E402
from oracle import pyoracle as orc                                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--whitelist", type=int, default=737280)
    ap.add_argument("--round", type=int, default=128, help="open clusters a tail round takes")
    args = ap.parse_args()
    bases, off = synth.make_reads(args.reads, synth.make_whitelist(args.whitelist), seed=1)
    reads = synth.reads_to_list(bases, off)
    cl = sb.queue_a(orc, reads, off.numpy())
    ndh = sb.wave_head_words(cl)
    st, op, rq, multi = [], [], [], []
    for a in range(0, len(cl), 16384):
        r = sb.evaluate(orc, cl[a:a + 16384], ndh[a:a + 16384])
        st.append(r["state"]); op.append(r["open"]); rq.append(r["requeue"]); multi.append(r["multi"])
    st, op, rq, multi = (np.concatenate(x) for x in (st, op, rq, multi))
    assert not (rq & multi & (st == sb.NO)).any() and (rq | ~multi | (st != sb.YES)).all()
    per_block = np.array([int(op[a:a + 512].sum()) for a in range(0, len(cl) - 511, 512)])
    rounds = lambda cap: float(np.mean(-(-per_block // cap)))
    print(json.dumps({
        "what": "open share of the tail certificate, host model", "reads": args.reads, "clusters": len(cl),
        "multi_hit": int(multi.sum()), "head_words_hist": {int(k): int(v) for k, v in zip(*np.unique(ndh, return_counts=True))},
        "decided_yes": int((multi & (st == sb.YES)).sum()), "decided_no": int((multi & (st == sb.NO)).sum()), "open": int(op.sum()),
        "requeue_true": int(rq.sum()), "open_that_requeue": int((op & rq).sum()),
        "open_share_of_clusters": round(float(op.mean()), 5), "open_share_of_multi_hit": round(float(op.sum() / max(multi.sum(), 1)), 5),
        "blocks_of_512": len(per_block), "open_per_block": {"mean": round(float(per_block.mean()), 2), "min": int(per_block.min()),
                                                            "p50": int(np.median(per_block)), "p99": int(np.percentile(per_block, 99)),
                                                            "max": int(per_block.max())},
        "tail_rounds_per_block": {"of_128": round(rounds(128), 4), "of_64": round(rounds(64), 4), "of_32": round(rounds(32), 4)}}))


if __name__ == "__main__":
    main()
