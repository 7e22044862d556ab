#!/bin/bash
# GPU box: the persistent iteration kernel's equality test, then the bench line at the headline and the CLIC-sized workload.
# usage: bash tools/run_persist_check.sh <tag> <out dir>   (<out dir>/<tag>_bench.json, <tag>_bench_clic.json)
set -e
TAG=${1:-p}
OUT=${2:?usage: bash tools/run_persist_check.sh <tag> <out dir>}
mkdir -p "$OUT"
timeout -k 10 600 python -m pytest tests/test_configs_at_size.py -x -q -m gpu -k persistent 2>&1 | tail -2
python bench.py --full --no-cpu-baseline > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err"
python bench.py --full --config clic --steps 5 --warmup 1 --no-extras > "$OUT/${TAG}_bench_clic.json" 2> "$OUT/${TAG}_bench_clic.err"
python - "$TAG" "$OUT" <<'PY'
import json, os, sys
for f in ("_bench.json", "_bench_clic.json"):
    d = json.load(open(os.path.join(sys.argv[2], sys.argv[1] + f)))
    print(f, d["ms_per_step"], d["roofline"]["frac"], d["roofline"]["avg_launch_ms"])
PY
