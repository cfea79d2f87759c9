"""kp_cluster_simulate_explained probe: on the config-4 cluster, the sweep's chunk 0 through
kp_cluster_simulate_budgeted (sim_kernel<4, SimLive>, every budget unlimited) and through kp_cluster_simulate_explained
(sim_kernel<4, SimWhy> + why_count_kernel), alternated in one process, and the whole explained call for the nodes'
singletons. usage: why_probe.py [nodes] [rounds]
  PROFILE=1: one warm-up and one call of each only (the process a `rocprofv3 --kernel-trace --stats` run wraps)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "karpenter-provider-aws_amd"))
import numpy as np  # noqa: E402

import kpamd  # noqa: E402
from kpamd import abi, catalog, disruption, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
lib = kpamd.load_lib()
cl = synth.config4(catalog.build_catalog(lib), n_nodes=n, seed=4)
ctx = kpamd.Context(0)
plan = kpamd.ClusterPlan(ctx, cl)
cands = np.asarray(cl.candidates, dtype=np.uint32)
offs, flat, _ = disruption.sweep_subsets(cands, 1_000_000, 0, 1)  # chunk 0 of the bench's sweep
offs, flat = np.ascontiguousarray(offs, np.uint32), np.ascontiguousarray(flat, np.uint32)
single_offs = np.arange(len(cands) + 1, dtype=np.uint32)
allowed = np.full(len(cl.nodepools), disruption.UNLIMITED, dtype=np.uint32)
P = C.POINTER


def run(explained, o, f):
    """One call on marshalled inputs: (wall ms, device ms, counts or None)."""
    m = len(o) - 1
    out = np.zeros(m, dtype=abi.sim_dtype())
    st, blocked = abi.SolveStats(), C.c_uint64(0)
    head = (plan.h, None, o.ctypes.data_as(P(C.c_uint32)), f.ctypes.data_as(P(C.c_uint32)), m, 1,
            allowed.ctypes.data_as(P(C.c_uint32)), len(allowed), out.ctypes.data_as(P(abi.SimResult)))
    t0 = time.perf_counter()
    if explained:
        why = (abi.SimWhy * m)()
        counts = (C.c_uint64 * abi.UNCONS_COUNT)()
        rc = lib.kp_cluster_simulate_explained(*head, why, counts, C.byref(blocked), C.byref(st))
    else:
        counts = None
        rc = lib.kp_cluster_simulate_budgeted(*head, C.byref(blocked), C.byref(st))
    wall = (time.perf_counter() - t0) * 1e3
    assert rc == 0, lib.kp_last_error()
    return wall, st.device_ms, None if counts is None else [int(c) for c in counts]


run(False, offs, flat), run(True, offs, flat)  # warm-up: code objects, the plan's scratch
if os.environ.get("PROFILE"):
    run(False, offs, flat), run(True, offs, flat)
    plan.close()
    sys.exit(0)
a, b = [], []
for _ in range(rounds):  # old and new alternated
    a.append(run(False, offs, flat))
    b.append(run(True, offs, flat))
s = [run(True, single_offs, cands) for _ in range(rounds)]
m = len(offs) - 1
res = {"nodes": n, "chunk_subsets": m, "rounds": rounds,
       "sim_live": {"device_ms_median": round(statistics.median(x[1] for x in a), 4),
                    "device_ms_min_max": [round(min(x[1] for x in a), 4), round(max(x[1] for x in a), 4)],
                    "wall_ms_median": round(statistics.median(x[0] for x in a), 4)},
       "sim_why": {"device_ms_median": round(statistics.median(x[1] for x in b), 4),
                   "device_ms_min_max": [round(min(x[1] for x in b), 4), round(max(x[1] for x in b), 4)],
                   "wall_ms_median": round(statistics.median(x[0] for x in b), 4), "counts": b[0][2]},
       "record_bytes": 48 * m, "result_bytes": 40 * m,
       "singletons": {"subsets": len(cands), "wall_ms_median": round(statistics.median(x[0] for x in s), 4),
                      "device_ms_median": round(statistics.median(x[1] for x in s), 4), "counts": s[0][2]}}
res["device_ratio_why_over_live"] = round(res["sim_why"]["device_ms_median"] / res["sim_live"]["device_ms_median"], 4)
plan.close()
print(json.dumps(res), flush=True)
