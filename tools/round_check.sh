#!/bin/bash
# Full GPU check of the tree: parity suite, smoke, the full bench line, rocprofv3 passes.
# Usage (repository root, on a GPU machine): bash tools/round_check.sh <tag>; results go to
# $OUT_DIR (default bench_out).
set -euo pipefail
TAG=${1:-r01}
OUT=${OUT_DIR:-bench_out}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/pytest_gpu_$TAG.log 2>&1
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1
timeout -k 10 300 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
bash tools/profile.sh $TAG
