set -e
OUT=${IC_OUT:-bench_out}/ls
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest -x -v --timeout 120 --timeout-method thread tests/test_stats_gpu.py > $OUT/tests.log 2>&1
for W in 0 4 8; do
  timeout -k 10 200 python bench.py --full --steps 10 --warmup 2 --option rowstat_waves=$W > $OUT/b_$W.json 2> $OUT/b_$W.err
done
