set -o pipefail
OUT=${1:?output directory}
mkdir -p $OUT
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $OUT/gputests.log 2>&1; echo "gpu tests rc=$?" | tee $OUT/rc.txt
tail -5 $OUT/gputests.log
timeout -k 10 300 python bench.py --steps 20 --warmup 5 --no-cpu-baseline --full > $OUT/bench_20.json 2> $OUT/bench_20.err; echo "bench20 rc=$?"
timeout -k 10 400 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err; echo "bench rc=$?"
python - "$OUT" <<'PY'
import json, sys
for f in ("bench_20","bench_default"):
    try:
        d=json.load(open(f"{sys.argv[1]}/{f}.json"))
        print(f, d["value"], d["ms_per_step"], d.get("fixed_call_us"), d.get("short_loop"), d["roofline"]["frac"], d.get("peaks_measured"), d["roofline_gather"]["K1"], d["roofline_gather"]["K1000"], d.get("ingest"), d.get("cpu_baseline",{}) and d["cpu_baseline"].get("value"))
        print({k:v["ms"] for k,v in d["kernels"].items()})
    except Exception as e:
        print(f, "ERR", e)
PY
