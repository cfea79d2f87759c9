#!/bin/bash
# GPU call: the general-path consolidation leg alone, with the host phase split (KP_HOST_TIMING)
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p $OUT; export TMPDIR=/tmp
KP_HOST_TIMING=1 timeout -k 10 300 python -u bench.py --full --only-general ${GEN_ARGS:-} > $OUT/general.json 2> $OUT/general.err || { tail -20 $OUT/general.err; exit 1; }
cat $OUT/general.json
grep "kp general" $OUT/general.err | tail -5
