#!/bin/bash
out=$(mktemp)
for cfg in "256 4" "256 2" "512 4" "512 2" "512 1" "1024 2" "1024 1"; do
  set -- $cfg
  SAC_FORCE_SP=$2 python bench.py --batch $1 --no-cpu-baseline --no-stepwise --full --steps 800 --warmup 100 > "$out" || exit 1
  python - "$out" <<PY
import json, sys
d = json.load(open(sys.argv[1]))
print("B=$1 SP=$2", d["value"], {k: v["ms"] for k, v in d["kernels"].items() if k[2] in "fbd"})
PY
done
rm -f "$out"
