#!/bin/bash
# GPU call: A/B of the in-tree library against tools/variants/*: config-2 quick bench and config-5 1M, interleaved
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p $OUT; export TMPDIR=/tmp; rm -f $OUT/ab.txt
[ -n "$AB_PRE_TESTS" ] && { bash tools/gpu_tests.sh $AB_PRE_TESTS || exit $?; }
for round in 1 2; do
  for lib in karpenter-provider-aws_amd/libkp.so tools/variants/*/libkp.so; do
    KP_LIB=$PWD/$lib timeout -k 10 200 python -u bench.py --full --quick --steps 3 --warmup 1 --no-cpu-baseline > $OUT/v.json 2> $OUT/v.err || { echo "$lib failed"; tail -5 $OUT/v.err; exit 1; }
    python3 -c "import json,sys; d=json.load(open('$OUT/v.json')); print(sys.argv[1], 'config2_kernel_ms', d['solve_kernel_ms'], 'step_ms', d['ms_per_step'])" $lib | tee -a $OUT/ab.txt
    if [ -n "$AB_C5" ]; then
      KP_LIB=$PWD/$lib REPS=1 timeout -k 10 200 python -u tools/c5_probe.py 1000000 > $OUT/v5.json 2> $OUT/v5.err || { echo "$lib c5 failed"; tail -5 $OUT/v5.err; exit 1; }
      python3 -c "import json,sys; d=json.load(open('$OUT/v5.json')); print(sys.argv[1], 'config5_kernel_ms', d['runs'][0]['kernel_ms'])" $lib | tee -a $OUT/ab.txt
    fi
  done
done
