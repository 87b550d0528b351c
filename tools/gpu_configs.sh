#!/bin/bash
# GPU tests for the precision modes, then one full bench line (with the roofline) per BASELINE config.
# Results go to $OUT (default bench_out/ in the repository).  usage: bash tools/gpu_configs.sh TAG
set -o pipefail
TAG=${1:-cfg}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
cd $R; mkdir -p $OUT
timeout -k 10 300 python -m pytest tests/test_bf16_gpu.py tests/test_split_gpu.py -x -q -p no:cacheprovider > $OUT/cfgtests_$TAG.log 2>&1 || { echo "TESTS FAIL"; tail -30 $OUT/cfgtests_$TAG.log; exit 1; }
tail -1 $OUT/cfgtests_$TAG.log
for c in C2 C3 C4 C5; do
  timeout -k 10 300 python bench.py --full --config $c --steps 10 --warmup 3 --no-cpu-baseline > $OUT/bench_${TAG}_$c.json 2> $OUT/bench_${TAG}_$c.err || { echo "BENCH FAIL $c"; tail -20 $OUT/bench_${TAG}_$c.err; exit 1; }
  cut -c1-250 $OUT/bench_${TAG}_$c.json
done
