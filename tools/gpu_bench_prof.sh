#!/bin/bash
# GPU call: gpu tests, full bench, rocprofv3 kernel stats of a quick bench, and separate PMC passes
# (FETCH_SIZE, WRITE_SIZE) for the HBM traffic of solve_kernel and feasibility_kernel.
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p $OUT
export TMPDIR=/tmp
if [ -z "$SKIP_TESTS" ]; then
  timeout -k 10 500 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/pytest_gpu.log 2>&1 || { tail -40 $OUT/pytest_gpu.log; exit 1; }
  tail -2 $OUT/pytest_gpu.log
fi
if [ -z "$SKIP_BENCH" ]; then
  timeout -k 10 600 python -u bench.py --full > $OUT/bench.json 2> $OUT/bench.err || { echo "bench rc=$?"; tail -30 $OUT/bench.err; exit 1; }
  cat $OUT/bench.json
fi
rm -rf $OUT/prof $OUT/pmc_fetch $OUT/pmc_write
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run -- python3 bench.py --full --quick --steps 3 --no-cpu-baseline > $OUT/prof.log 2>&1 || { echo "rocprof rc=$?"; tail -20 $OUT/prof.log; exit 1; }
timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -o run -- python3 bench.py --full --quick --steps 3 --warmup 0 --no-cpu-baseline > $OUT/pmc_fetch.log 2>&1 || { echo "pmc fetch rc=$?"; tail -20 $OUT/pmc_fetch.log; exit 1; }
timeout -s KILL 120 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -o run -- python3 bench.py --full --quick --steps 3 --warmup 0 --no-cpu-baseline > $OUT/pmc_write.log 2>&1 || { echo "pmc write rc=$?"; tail -20 $OUT/pmc_write.log; exit 1; }
find $OUT/prof $OUT/pmc_fetch $OUT/pmc_write -name '*.csv' | head -20
