#!/bin/bash
# Row-kernel change check on the GPU: parity tests touching LN / dwconv, row-kernel timings, bench x2.
# Results go to $OUT_DIR (default bench_out)/<tag>.
set -euo pipefail
TAG=${1:-rowops}
OUT=${OUT_DIR:-bench_out}/$TAG
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/pytest.log 2>&1
timeout -k 10 120 python tools/rowops_bench.py > $OUT/rowops.txt 2>/dev/null
for r in 1 2; do timeout -k 10 200 python bench.py --full --no-cpu-baseline > $OUT/bench.$r.json 2>/dev/null; done
