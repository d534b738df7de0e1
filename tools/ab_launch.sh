set -euo pipefail
OUT=${OUT_DIR:-bench_out}
mkdir -p $OUT
for i in 1 2; do
timeout -k 10 300 python bench.py --full --inproc --no-cpu-baseline --roofline-steps 1 > $OUT/ab_inproc_$i.json 2>/dev/null
timeout -k 10 300 python bench.py --full --no-cpu-baseline --roofline-steps 1 > $OUT/ab_launch_$i.json 2>/dev/null
done
