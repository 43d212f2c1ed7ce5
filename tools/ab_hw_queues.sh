# bench.py --gpus 2/4 --transport ipc with 4 vs 16 hardware queues per rank process, both
# orders; one JSON line per run into $OUT (--full: each run's gather_check beside the headline)
set -o pipefail
OUT=${OUT:-${TMPDIR:-/tmp}/ab_hw_queues}
mkdir -p "$OUT"
for n in 2 4; do
  for q in 4 16 16 4; do
    timeout -k 10 200 python3 bench.py --full --gpus $n --transport ipc --hw-queues $q --steps 20 --warmup 5 --no-sweep --no-cpu-baseline > "$OUT/n${n}_q${q}_$RANDOM.json" 2>> "$OUT/err.log" || exit $?
  done
done
