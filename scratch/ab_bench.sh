#!/bin/bash
# A/B of two library builds with bench.py itself, on ONE box: scratch/ab/a_parent.so and scratch/ab/b_change.so are copied
# over the package's library in turn, PAIRS times, each run under its own time limit; every result line goes to OUT.jsonl
# tagged with the library, the configuration name and the pair (profiles/row_images_ab.jsonl was made this way).
#   usage: scratch/ab_bench.sh OUT.jsonl PAIRS CONFIG_NAME [bench.py arguments ...]
# (a parent build older than a symbol of robosuite_benchmark_amd/_lib.py SYMBOLS needs a stub of it to load)
out=$1; pairs=$2; cfg=$3; shift 3
keep=$(mktemp) && cp robosuite_benchmark_amd/libsac_hip.so "$keep" || exit 1
res=$(mktemp); err=$(mktemp)
for i in $(seq 1 "$pairs"); do
  for name in a_parent b_change; do
    cp scratch/ab/$name.so robosuite_benchmark_amd/libsac_hip.so || exit 1
    timeout -k 10 150 python3 bench.py --gpus 1 "$@" > "$res" 2> "$err"
    rc=$?
    if [ $rc -ne 0 ]; then
      echo "bench.py failed (exit $rc) with $name, $cfg"; tail -20 "$err"
      cp "$keep" robosuite_benchmark_amd/libsac_hip.so
      exit $rc
    fi
    tail -1 "$res" | sed "s/^{/{\"ab_lib\": \"${name#?_}\", \"ab_config\": \"$cfg\", \"ab_pair\": $i, /" >> "$out"
  done
done
cp "$keep" robosuite_benchmark_amd/libsac_hip.so
python3 - "$out" <<'EOF'
import json, statistics, sys
rows = [json.loads(l) for l in open(sys.argv[1])]
for cfg in dict.fromkeys(r["ab_config"] for r in rows):
    for lib in ("parent", "change"):
        v = [1000.0 * r["ms_per_step"] for r in rows if r["ab_config"] == cfg and r["ab_lib"] == lib]
        if v:
            print(f"{cfg:14s} {lib:7s} n={len(v)}  median {statistics.median(v):7.3f} us  min {min(v):7.3f}  max {max(v):7.3f}")
EOF
