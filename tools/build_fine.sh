#!/bin/bash
# Diagnostic FT_FINE build of libkp (the fast-lane phase probes, finer ones included) into tools/fine/libkp.so (KP_LIB=... selects it).
# Extra -D flags (tools/kp_diag.h knobs, e.g. -DMERGE_DIAG=1 -DREQ_CLASSES=0) follow; FINE_NAME=<dir under tools/> names
# another output directory (default: fine).
set -e
cd "$(dirname "$0")/../karpenter-provider-aws_amd"
out=../tools/${FINE_NAME:-fine}
mkdir -p $out build
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I../include -Icsrc -include ../tools/kp_diag.h -Wno-unused-function -mllvm -amdgpu-sched-strategy=max-ilp -DKP_TU=1 -DFT_FINE=1 -DFL_NOTIME=0 "$@" -c csrc/kp_kernels.hip -o build/kp_kernels_${FINE_NAME:-fine}.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $out/libkp.so.tmp build/kp_kernels_${FINE_NAME:-fine}.o build/kp_filter.o build/kp_host.o -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib && mv -f $out/libkp.so.tmp $out/libkp.so
