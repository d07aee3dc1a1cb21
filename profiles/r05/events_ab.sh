#!/bin/bash
# the cost of the timed frames' HIP events: bench.py --full with and without --no-events, lines under $OUT/evab
set -e
O=${OUT:-profiles/out}/evab
mkdir -p $O
for r in 1 2 3; do
  for opt in "" "--no-events"; do
    timeout -k 10 120 python3 bench.py --full --no-cpu-baseline --no-stats $opt > $O/a_${r}_${opt:-ev}.json 2>/dev/null
    python3 -c "import json,sys; d=json.load(open(sys.argv[1])); print(sys.argv[2], d['value'], d['ms_per_step'])" $O/a_${r}_${opt:-ev}.json "100/20 r$r ${opt:-events}"
    timeout -k 10 120 python3 bench.py --full --no-cpu-baseline --no-stats --steps 20 --warmup 5 $opt > $O/b_${r}_${opt:-ev}.json 2>/dev/null
    python3 -c "import json,sys; d=json.load(open(sys.argv[1])); print(sys.argv[2], d['value'], d['ms_per_step'])" $O/b_${r}_${opt:-ev}.json "20/5 r$r ${opt:-events}"
  done
done
