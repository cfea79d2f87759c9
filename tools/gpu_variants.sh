#!/bin/bash
# Quick config-2 bench of every built variant (tools/variants/*/libkp.so) and of the in-tree library, interleaved twice.
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p $OUT; export TMPDIR=/tmp; rm -f $OUT/variants.txt
for round in 1 2; do
  for lib in karpenter-provider-aws_amd/libkp.so tools/variants/*/libkp.so; do
    KP_LIB=$PWD/$lib timeout -k 10 200 python -u bench.py --full --quick --steps 3 --warmup 1 --no-cpu-baseline > $OUT/v.json 2> $OUT/v.err || { echo "$lib failed"; tail -5 $OUT/v.err; exit 1; }
    python3 -c "import json,sys; d=json.load(open('$OUT/v.json')); print(sys.argv[1], 'kernel_ms', d['solve_kernel_ms'], 'step_ms', d['ms_per_step'], 'alg_bytes', d['roofline']['algorithmic_bytes_per_launch'])" $lib | tee -a $OUT/variants.txt
  done
done
