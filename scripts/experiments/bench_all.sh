#!/bin/bash
# Every bench config once (C2 with --full: the CPU baseline), one JSON line each -> $BENCH_OUT/bench_<cfg>.log
set -o pipefail
cd "$(dirname "$0")/../.." || exit 1; OUT=${BENCH_OUT:-bench_out}; mkdir -p "$OUT"
timeout -k 10 300 python bench.py --full 2>&1 | grep -v amdgpu.ids | tee "$OUT/bench_c2.log" || exit 1
for c in ${1:-c3 c4 c5 decode decode_long}; do
  timeout -k 10 300 python bench.py --config $c --no-cpu-baseline 2>&1 | grep -v amdgpu.ids | tee "$OUT/bench_$c.log" || exit 1
done
