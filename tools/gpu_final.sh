#!/bin/bash
# end-of-round check: full GPU suite + smoke + C2 full bench + rocprof (gpu_check.sh), C3/C4/C5 full bench lines.
# Results go to $OUT (default bench_out/ in the repository).
#   bash tools/gpu_final.sh TAG
set -o pipefail
TAG=${1:-final}
R=$(cd "$(dirname "$0")/.." && pwd)
export OUT=${OUT:-$R/bench_out}
cd $R
bash tools/gpu_check.sh $TAG || exit 1
grep -q "TESTS EXIT 0" $OUT/tests_$TAG.log || { grep -E "^FAILED" $OUT/tests_$TAG.log | head; exit 1; }
for c in C3 C4 C5; do
  timeout -k 10 300 python bench.py --full --config $c --steps 10 --warmup 3 --no-cpu-baseline > $OUT/bench_${TAG}_$c.json 2> $OUT/bench_${TAG}_$c.err || { echo "BENCH FAIL $c"; exit 1; }
  cut -c1-200 $OUT/bench_${TAG}_$c.json
done
