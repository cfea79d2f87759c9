#!/bin/bash
# GPU call (round-6 close): the whole -m gpu suite and smoke, then the default bench line.
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p $OUT; export TMPDIR=/tmp
bash tools/gpu_full_suite.sh || exit 1
timeout -k 10 800 python -u bench.py --full > $OUT/bench_full.json 2> $OUT/bench_full.err || { tail -30 $OUT/bench_full.err; exit 1; }
tail -c 300 $OUT/bench_full.err
