#!/bin/bash
# The driver's N = 1 bench command with the row order refreshed every 32 frames (default)
# vs measured once (1000000), interleaved; one JSON line per run into $OUT (kernel_ms
# beside the headline; --full --no-sweep: no steady-state loop or windows before the timed
# region).
set -o pipefail
OUT=${OUT:-${TMPDIR:-/tmp}/ab_row_feedback}
mkdir -p "$OUT"
for rf in 32 1000000 1000000 32 32 1000000; do
  timeout -k 10 240 python3 bench.py --full --steps 20 --warmup 5 --no-sweep --no-cpu-baseline --no-c5 \
      --row-feedback $rf > "$OUT/rf${rf}_$RANDOM.json" 2>> "$OUT/err.log" || exit $?
done
