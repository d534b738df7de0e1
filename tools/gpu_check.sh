#!/bin/bash
# GPU parity suite + smoke + the full bench line (run from the repository root on a GPU machine).
# Usage: bash tools/gpu_check.sh <tag> [pytest -k expr]; results go to $OUT_DIR (default bench_out).
set -euo pipefail
TAG=${1:-r02}
K=${2:-}
OUT=${OUT_DIR:-bench_out}
mkdir -p $OUT
if [ -n "$K" ]; then KA=(-k "$K"); else KA=(); fi
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread "${KA[@]}" \
    > $OUT/pytest_gpu_$TAG.log 2>&1
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1
timeout -k 10 400 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
echo done > $OUT/DONE_$TAG
