#!/bin/bash
# One measurement cycle after a library change (the source hash in bdg_version() changes with every edit, and bench.py prints
# roofline.traffic / int_issue only when profiles/traffic.json was taken from the running build):
#
#   on the build host:        tools/round_profile.sh gpu <tag>        # two calls of $RUN: tests + profile passes, then bench lines
#                             tools/round_profile.sh collect <tag> [<old tag>]   # condense into profiles/, drop the old tag's files
#
# <tag> e.g. r03_a.  The docs (README.md, BASELINE.md, profiles/README.md) still have to follow by hand.
# OUT: the directory, relative to the tree, that tools/pmc_profile.sh and tools/ops_profile.sh write under.  RUN (gpu only):
# a command that runs its one argument, a shell command, in a copy of this tree on the GPU host and brings $OUT back.
set -eu
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
mode=$1; tag=$2
OUT=${OUT:?set OUT, see above}
case $mode in
gpu)
    rm -rf $OUT/${tag} $OUT/${tag}_c3 $OUT/${tag}_c5 $OUT/${tag}_ops
    ${RUN:?set RUN, see above} "timeout -k 10 900 python -m pytest tests -x -q -m gpu > $OUT/${tag}_tests.txt 2>&1 && bash tools/pmc_profile.sh ${tag} --no-graph && bash tools/pmc_profile.sh ${tag}_c5 --config 5 && bash tools/pmc_profile.sh ${tag}_c3 --config 3 && bash tools/ops_profile.sh ${tag}_ops; tail -1 $OUT/${tag}_tests.txt"
    python3 tools/summarize_profile.py $OUT/${tag} ${tag} $OUT/${tag}_c5 $OUT/${tag}_c3   # writes profiles/traffic.json (+ valu, lds) for this build BEFORE the bench lines
    ${RUN:?set RUN, see above} "python bench.py --full > $OUT/${tag}_bench.json 2> $OUT/${tag}_bench.err && python bench.py --full --config 3 > $OUT/${tag}_bench_c3.json 2>> $OUT/${tag}_bench.err && python bench.py --full --config 5 > $OUT/${tag}_bench_c5.json 2>> $OUT/${tag}_bench.err && python bench.py --full --no-overlap --no-graph > $OUT/${tag}_bench_ov.json 2>> $OUT/${tag}_bench.err && python tools/stress_parity.py --cases 2 > $OUT/${tag}_stress.txt 2>&1; tail -n 1 $OUT/${tag}_stress.txt"
    ;;
collect)
    old=${3:-}
    if [ -n "$old" ]; then git rm -q --cached profiles/${old}_* 2>/dev/null || true; rm -f profiles/${old}_*; fi
    python3 tools/summarize_profile.py $OUT/${tag} ${tag} $OUT/${tag}_c5 $OUT/${tag}_c3
    for t in c5 c3 ops; do cp "$(find $OUT/${tag}_$t/stats -name '*_kernel_stats.csv' | head -1)" profiles/${tag}_${t}_kernel_stats.csv; done
    cp "$(find $OUT/${tag}/stats -name '*_kernel_stats.csv' | head -1)" profiles/${tag}_kernel_stats.csv
    cp $OUT/${tag}_ops/ops.jsonl profiles/${tag}_ops.jsonl
    round=${tag%%_*}
    cp $OUT/${tag}_bench.json profiles/${round}_bench.json
    cp $OUT/${tag}_bench_c3.json profiles/${round}_bench_config3.json
    cp $OUT/${tag}_bench_c5.json profiles/${round}_bench_config5.json
    cp $OUT/${tag}_bench_ov.json profiles/${round}_bench_no_overlap.json
    python3 - "$tag" "$round" <<'PY'
import json, sys
tag, rnd = sys.argv[1], sys.argv[2]
d = json.load(open("profiles/%s_summary.json" % tag))
for k in ("k_scan_reads", "k_sw_clusters", "k_strict_filter", "k_finalize_reads", "k_nearest_pairs", "k_nearest_delins"):
    v = d[k]
    print(k, "launches", v["calls"], round(v["avg_ns"] / 1e3, 1), "us", round(v.get("SQ_INSTS_VALU", 0) / 1e6, 1), "M vector instructions")
for f in ("bench", "bench_config3", "bench_config5", "bench_no_overlap"):
    x = json.loads(open("profiles/%s_%s.json" % (rnd, f)).read().strip().splitlines()[-1])
    print(f, round(x["value"] / 1e6, 1), x["unit"], round(x["ms_per_step"], 4), "ms", x["parity_sample"], x["roofline"]["kernel"],
          round(x["roofline"]["kernel_ms"], 4), "frac", round(x["roofline"]["frac"], 4), "traffic", x["roofline"].get("traffic"))
PY
    ;;
*) echo "usage: $0 gpu|collect <tag> [<old tag>]"; exit 2;;
esac
