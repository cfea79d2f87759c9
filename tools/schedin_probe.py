"""Scheduler-inputs probe: kp_scheduler_inputs on the config-4 cluster with a synthetic scheduler state (10,000 nodes,
50 daemonsets, about 30 bound pods per node), the whole call against the plain-Python reference
(tests/schedin_ref.py, CPU; order of magnitude only: the reference is not upstream's Go), the host-compile share, and
the bytes each kernel must move as a fraction of 8 TB/s. usage: schedin_probe.py [nodes] [daemonsets] [rounds]
  PROFILE=1: two warm-up calls and three calls only (the process a `rocprofv3 --kernel-trace --stats` run wraps); the
  reference is not run."""
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "karpenter-provider-aws_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import kpamd  # noqa: E402
from kpamd import abi, catalog, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
n_ds = int(sys.argv[2]) if len(sys.argv) > 2 else 50
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 9
lib = kpamd.load_lib()
cat = catalog.build_catalog(lib)
cl = synth.config4(cat, n_nodes=n)
state = synth.add_scheduler_state(cl, 4, n_daemonsets=n_ds)
ctx = kpamd.Context(0)
arena = abi.Arena()
st = abi.build_sched_state(arena, state)  # the binding's marshalling is not timed: a shim fills the structs itself


def call():
    """One kp_scheduler_inputs on the marshalled state: (wall ms, host_ms, the host compile's ms, device_ms), result"""
    t0 = time.perf_counter()
    got = kpamd._scheduler_inputs_raw(lib, ctx.h, st)
    wall = (time.perf_counter() - t0) * 1e3
    s = got[-1]
    return (wall, s.host_ms, s.prepare_ms, s.device_ms), got


t0 = time.perf_counter()
call()  # code objects, the context's arena
first_ms = (time.perf_counter() - t0) * 1e3
call()
if os.environ.get("PROFILE"):
    for _ in range(3):
        call()
    sys.exit(0)


def spread(runs, k):
    v = [r[k] for r in runs]
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


runs = [call()[0] for _ in range(rounds)]
N, D, P, M, R = st.n_nodes, st.n_daemonsets, st.n_nodepools, st.n_pods, st.n_request_rows
W = max(1, (D + 63) // 64)
keys = len({abi_key for d in state.daemonsets for abi_key in
            list(d.node_selector) + [r[0] for r in (d.required_terms[0] if d.required_terms else [])] +
            [r[0] for r in d.volume_requirements]})
RL = 104  # sizeof(kp_resource_list)
floors = {
    # per node its taint set (4 B), one value id per key some template names (4 B each), the words out; tables once
    "schedin_compat_kernel": N * (4 + 4 * keys + 8 * W),
    # the words in, the CSR and the pods (4 B each), allocatable in, the record out; template and request rows once
    "schedin_node_kernel": N * (8 * W + 4 + RL + 2 * RL + 8) + 4 * M + RL * (D + R),
    # the pools' node lists (4 B per node), capacity in, the partials out
    "schedin_pool_kernel": N * (4 + RL) + P * 8 * 12 * 8,
    "schedin_pool_final_kernel": P * (8 * 12 * 8 + RL * 3 + 8) + RL * D,
}
res = {"nodes": N, "daemonsets": D, "pools": P, "bound_pods": M, "request_rows": R, "keys": keys, "rounds": rounds,
       "first_call_ms": round(first_ms, 3), "wall_ms": spread(runs, 0), "host_ms": spread(runs, 1),
       "host_compile_ms": spread(runs, 2), "device_ms": spread(runs, 3),
       "host_compile_share": round(statistics.median(r[2] for r in runs) / statistics.median(r[1] for r in runs), 3),
       "kernel_floor_bytes": floors,
       "kernel_floor_us_at_8TBps": {k: round(v / 8e12 * 1e6, 3) for k, v in floors.items()}}
import schedin_ref as ref  # noqa: E402
t0 = time.perf_counter()
want = ref.compute(state)
res["reference_cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
got = kpamd.SchedulerInputs(*call()[1])
try:
    ref.assert_equal(got, want, "probe")
    res["equal_to_reference"] = True
except AssertionError as e:
    res["equal_to_reference"] = False
    res["difference"] = str(e)[:200]
ones = sum(sum(row) for row in want["matrix"])
res["compatible_share"] = round(ones / max(1, N * D), 3)
print(json.dumps(res), flush=True)
