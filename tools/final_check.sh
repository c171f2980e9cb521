#!/bin/bash
# The round's closing check on the GPU box: the whole GPU suite, then a short bench line with its boundary leg.
#   bash tools/final_check.sh OUT_DIR      -> OUT_DIR/t_all.log, OUT_DIR/bench_short.json (+ .err)
OUT=$(mkdir -p "${1:?usage: bash tools/final_check.sh OUT_DIR}" && cd "$1" && pwd)
R=$(cd "$(dirname "$0")/.."; pwd); cd $R
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $OUT/t_all.log 2>&1; echo "pytest rc=$?" >> $OUT/t_all.log; tail -3 $OUT/t_all.log
timeout -k 10 280 python bench.py --full --steps 4 --warmup 2 --cpu-seconds 0 --no-overlap-leg --boundary-batches 8000 > $OUT/bench_short.json 2> $OUT/bench_short.err; echo "bench rc=$?"
python3 - $OUT/bench_short.json <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["value"], d["roofline"].get("rocprofv3_avg_launch_us"), d["roofline"].get("rocprofv3_source"))
b = d["boundary"]
print([(l["mode"], l["batch"], round(l["batches_per_sec"])) for l in b.get("by_batch_size", []) + b.get("slab_only_trainer", {}).get("by_batch_size", [])], b.get("error"))
PY
