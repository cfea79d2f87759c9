"""Drift-detection probe: kp_cluster_detect_drift on the config-4 cluster with randomized drift inputs, the whole call
against the plain-Python reference (tests/driftdet_ref.py, CPU) on the same cluster, and the bytes the kernels must
move. usage: drift_probe.py [nodes] [nodeclasses] [amis] [rounds]
  PROFILE=1: two warm-up calls and three calls only (the process a `rocprofv3 --kernel-trace --stats` run wraps); the
  reference is not run."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "karpenter-provider-aws_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import kpamd  # noqa: E402
from kpamd import abi, catalog, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
n_classes = int(sys.argv[2]) if len(sys.argv) > 2 else 4
n_amis = int(sys.argv[3]) if len(sys.argv) > 3 else 8
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 7
lib = kpamd.load_lib()
cat = catalog.build_catalog(lib)
cl = synth.config4(cat, n_nodes=n)
inputs = synth.add_drift_inputs(cl, 4, n_nodeclasses=n_classes, n_amis=n_amis)
ctx = kpamd.Context(0)
plan = kpamd.ClusterPlan(ctx, cl)
arena = abi.Arena()
di = abi.build_drift_in(arena, inputs)  # the binding's marshalling is not timed: a shim fills the structs itself
out = np.zeros(n, dtype=abi.node_drift_dtype())
counts, st = (C.c_uint64 * abi.DRIFT_REASON_COUNT)(), abi.SolveStats()


def call(records=True):
    """One kp_cluster_detect_drift on marshalled inputs: (wall ms, the call's host_ms, device_ms)."""
    t0 = time.perf_counter()
    rc = lib.kp_cluster_detect_drift(plan.h, C.byref(di), out.ctypes.data if records else None, counts, C.byref(st))
    wall = (time.perf_counter() - t0) * 1e3
    assert rc == 0, lib.kp_last_error()
    return wall, st.host_ms, st.device_ms


t0 = time.perf_counter()
call()  # the plan's resident half (DriftBuild), code objects
first_ms = (time.perf_counter() - t0) * 1e3
call()
if os.environ.get("PROFILE"):
    for _ in range(3):
        call()
    plan.close()
    sys.exit(0)


def spread(runs, k):
    v = [r[k] for r in runs]
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


runs = [call() for _ in range(rounds)]
hist = [call(records=False) for _ in range(rounds)]
sgs = sum(len(set(x.instance.security_groups)) for x in inputs.nodes if x.instance is not None)
keys = len({r[0] for p in cl.nodepools for r in p.requirements})
res = {"nodes": n, "pools": len(cl.nodepools), "nodeclasses": len(inputs.nodeclasses), "amis_per_class": n_amis,
       "rounds": rounds, "first_call_ms": round(first_ms, 3),
       "wall_ms": spread(runs, 0), "host_ms": spread(runs, 1), "device_ms": spread(runs, 2),
       "histogram_only_wall_ms": spread(hist, 0), "counts": [int(c) for c in counts],
       # the byte floor of the per-node kernel: pool and type index (8 B), a value id per key of the pool (4 B each, here
       # at most `keys`), the node record (32 B), the security-group CSR (4 B per node and per id), the record out (16 B)
       "node_kernel_floor_bytes": n * (8 + 4 * keys + 32 + 4 + 16) + 4 * sgs,
       "count_kernel_floor_bytes": 16 * n}
import driftdet_ref as ref  # noqa: E402
t0 = time.perf_counter()
want, want_counts = ref.detect(cl)
res["reference_cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
call()
res["equal_to_reference"] = bool(want_counts == [int(c) for c in counts] and all(
    (int(g["reason"]), int(g["status"]), int(g["detail"])) == w for g, w in zip(out, want)))
plan.close()
print(json.dumps(res), flush=True)
