#!/bin/bash
# CPU-only: stage 1's formatters (badger_amd/csrc/stage1_format.cpp, which needs no HIP) under AddressSanitizer + UBSan.
# format_driver.cpp calls every bdg_format_* entry point on one hand-made chunk of edge cases, first for the bound and then into
# a heap block of exactly that size: a bound that is too small is a heap-buffer-overflow report.  Prints the driver's lines
# (length, checksum and counts of each text): they change only when the text does.
set -eu
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
T=${TMPDIR:-/tmp}/bdg_sanitize; mkdir -p $T
g++ -O1 -g -std=c++17 -Wall -I$ROOT/include -I$ROOT/badger_amd/csrc -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    $ROOT/tools/sanitize/format_driver.cpp $ROOT/badger_amd/csrc/stage1_format.cpp -o $T/format_asan
rc=0
out=$($T/format_asan 2>&1) || rc=1
echo "$out"
if echo "$out" | grep -q "Sanitizer\|runtime error\|FAIL"; then rc=1; fi
[ $rc = 0 ] && echo "format sanitizers: clean (asan+ubsan; every bdg_format_* entry point into a block of exactly its bound)"
exit $rc
