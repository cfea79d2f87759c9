"""Candidate-selection probe: kp_cluster_candidates on the config-4 cluster with randomized controls, the whole call
against the plain-Python reference (tests/candidate_ref.py, CPU) on the same cluster, and the bytes the kernels must
move. usage: candidates_probe.py [nodes] [pdbs] [rounds]
  PROFILE=1: two warm-up calls and one call per method only (the process a `rocprofv3 --kernel-trace --stats` run
  wraps); the reference is not run."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "karpenter-provider-aws_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import kpamd  # noqa: E402
from kpamd import abi, catalog, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
n_pdbs = int(sys.argv[2]) if len(sys.argv) > 2 else 256
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 9
NOW = 1_750_100_000
lib = kpamd.load_lib()
cat = catalog.build_catalog(lib)
cl = synth.config4(cat, n_nodes=n)
synth.add_disruption_controls(cl, 4, n_pdbs=n_pdbs, now=NOW)
ctx = kpamd.Context(0)
plan = kpamd.ClusterPlan(ctx, cl)
arena = abi.Arena()
import ctypes as C  # noqa: E402
import numpy as np  # noqa: E402

out = np.zeros(n, dtype=abi.candidate_dtype())
order = np.zeros(n, dtype=np.uint32)
count, st = C.c_uint32(0), abi.SolveStats()


def call(method):
    """One kp_cluster_candidates on marshalled inputs (the binding's marshalling is not timed: a shim fills the structs
    itself): (wall ms, the call's host_ms, device_ms, candidates)."""
    ci = abi.build_candidates_in(arena, cl.controls, method, NOW)
    t0 = time.perf_counter()
    rc = lib.kp_cluster_candidates(plan.h, C.byref(ci), out.ctypes.data, order.ctypes.data_as(C.POINTER(C.c_uint32)),
                                   C.byref(count), C.byref(st))
    wall = (time.perf_counter() - t0) * 1e3
    assert rc == 0, lib.kp_last_error()
    return wall, st.host_ms, st.device_ms, int(count.value)


call(1), call(1)  # warm-up: the plan's resident half, code objects
if os.environ.get("PROFILE"):
    for m in range(4):
        call(m)
    plan.close()
    sys.exit(0)
res = {"nodes": n, "pods": int(len(cl.pod_shape)), "pod_refs": sum(len(x.pods) for x in cl.nodes), "pdbs": n_pdbs,
       "shapes": len(cl.shapes), "rounds": rounds}
for m, name in enumerate(("emptiness", "single", "multi", "drift")):
    runs = [call(m) for _ in range(rounds)]
    res[name] = {"candidates": runs[0][3], "wall_ms_median": round(statistics.median(r[0] for r in runs), 4),
                 "host_ms_median": round(statistics.median(r[1] for r in runs), 4),
                 "device_ms_median": round(statistics.median(r[2] for r in runs), 4)}
# the byte floor of the per-node kernel: CSR offsets and pod indices, a pod record, shape and verdict per pod reference,
# the node's record in, 24 B per node out and the sort arrays' 12 B; of the order: 4 B per candidate
res["node_kernel_floor_bytes"] = 4 * (n + 1) + res["pod_refs"] * (4 + 16 + 4 + 4) + n * (40 + 4 + 24 + 12)
import candidate_ref as ref  # noqa: E402
t0 = time.perf_counter()
want = ref.candidates(cl, cl.controls, ref.SINGLE, NOW)
res["reference_cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
call(1)
res["equal_to_reference"] = bool([int(x) for x in order[:count.value]] == want[1] and
                                 all((int(g["reason"]), int(g["detail"]), int(g["rescheduling_cost_fx"]),
                                      float(g["disruption_cost"])) == w for g, w in zip(out, want[0])))
plan.close()
print(json.dumps(res), flush=True)
