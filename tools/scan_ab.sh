#!/bin/bash
# Scan change check on the GPU: scan parity tests, scan alone at 16/32 clips, bench x2.
# Results go to $OUT_DIR (default bench_out)/<tag>.
set -euo pipefail
TAG=${1:-scan}
OUT=${OUT_DIR:-bench_out}/$TAG
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests/test_scan_fma.py tests/test_gpu_parity.py -k "scan or fma" -x -q --timeout 120 --timeout-method thread > $OUT/pytest.log 2>&1
for m in 2 0; do for b in 16 32; do timeout -k 10 60 python tools/scan_bench.py $b 501 384 64 $m 100 2>/dev/null >> $OUT/scan.txt; done; done
for r in 1 2; do timeout -k 10 200 python bench.py --full --no-cpu-baseline > $OUT/bench.$r.json 2>/dev/null; done
