#!/bin/bash
# End-of-round profiling of the in-tree library on the GPU box: per config a kernel trace + stats
# and the PMC passes of scripts/profile.sh, then a bench line (--full). usage: profile_all.sh <tag> "<cfgs>"
set -o pipefail
TAG=$1; CFGS=${2:-"c2 c3 c4 c5 window decode decode_long decode_padded"}
cd "$(dirname "$0")/../.." || exit 1; OUT=${BENCH_OUT:-bench_out}; mkdir -p "$OUT"
for c in $CFGS; do
  echo "== $c $(date +%T)"
  bash scripts/profile.sh ${TAG}_$c --config $c > "$OUT/prof_${TAG}_$c.out" 2>&1 || { tail -5 "$OUT/prof_${TAG}_$c.out"; exit 1; }
  timeout -k 10 300 python bench.py --full --config $c > "$OUT/${TAG}_bench_$c.json" 2> "$OUT/${TAG}_bench_$c.err" || { tail -5 "$OUT/${TAG}_bench_$c.err"; exit 1; }
  cut -c1-300 "$OUT/${TAG}_bench_$c.json"
done
