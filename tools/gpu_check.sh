#!/bin/bash
# One GPU visit: GPU parity tests, smoke, the full bench line (roofline, optimizer step, CPU baseline), rocprof
# kernel stats.  Results go to $OUT (default bench_out/ in the repository).
# usage: bash tools/gpu_check.sh TAG
set -o pipefail
TAG=${1:-run}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
mkdir -p $OUT
cd $R
timeout -k 10 600 python -m pytest tests -m gpu -q -rf -s -p no:cacheprovider > $OUT/tests_$TAG.log 2>&1
echo "TESTS EXIT $?" | tee -a $OUT/tests_$TAG.log
rc=$(tail -1 $OUT/tests_$TAG.log | awk '{print $3}')
case $rc in 0|1) ;; *) echo "abort after tests rc=$rc"; exit $rc;; esac
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1 || { echo SMOKE FAIL; tail -20 $OUT/smoke_$TAG.log; exit 1; }
timeout -k 10 400 python bench.py --full ${BENCH_ARGS:---steps 20 --warmup 5} > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { echo BENCH FAIL; tail -20 $OUT/bench_$TAG.err; exit 1; }
cat $OUT/bench_$TAG.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python3 $R/bench.py --full --steps 10 --warmup 2 --no-cpu-baseline > $OUT/prof_$TAG.log 2>&1 || { echo PROF FAIL; tail -20 $OUT/prof_$TAG.log; exit 1; }
# the dominant kernel's launches the roofline times live (g_a.2 fwd: the first main-queue ig_kernel_x3d of each
# step) from the same trace, to set beside bench's live figure
python3 $R/tools/trace_timeline.py $(find $OUT/prof_$TAG -name "*kernel_trace.csv" | head -1) --first ig_kernel_x3d > $OUT/first_$TAG.txt 2>&1
head -2 $OUT/first_$TAG.txt
echo DONE
