"""Launch-template probe: kp_launch_run_templates on a burst of launch requests over the 919-type catalogue (three zones,
four AMIs), next to kp_launch_run alone on the same plan in the same process (what the launch cost before the grouping
existed) and the plain-Python reference (tests/ltgroup_ref.py, CPU) on a sample, with equality asserted.
usage: ltgroup_probe.py [requests] [options per request] [rounds] [reference sample] [max_types]
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
from kpamd import abi, catalog  # noqa: E402
from kpamd.model import AMI  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000
n_opts = int(sys.argv[2]) if len(sys.argv) > 2 else 100
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 9
sample = int(sys.argv[4]) if len(sys.argv) > 4 else 64
max_types = int(sys.argv[5]) if len(sys.argv) > 5 else 60
K = "karpenter.k8s.aws/"
AMIS = [AMI("ami-gpu", [(K + "instance-gpu-count", "Exists", [])]), AMI("ami-amd64", [("kubernetes.io/arch", "In", ["amd64"])]),
        AMI("ami-arm64", [("kubernetes.io/arch", "In", ["arm64"])]), AMI("ami-rest", [])]
lib = kpamd.load_lib()
cat = catalog.build_catalog(lib)
T = len(cat)
rng = np.random.default_rng(19)
# NodeClaims as a config-5 burst leaves them: a capacity-type choice, sometimes an architecture or a zone, 100 options
requests = []
for i in range(n):
    reqs = [("karpenter.sh/capacity-type", "In", [["on-demand"], ["spot"], ["on-demand", "spot"]][i % 3])]
    if i % 4 == 1:
        reqs.append(("kubernetes.io/arch", "In", [["amd64", "arm64"][(i // 4) % 2]]))
    if i % 5 == 2:
        reqs.append(("topology.kubernetes.io/zone", "In", [catalog.ZONES[i % 3]]))
    requests.append((reqs, {"cpu": int(rng.choice([500, 2000, 8000])), "memory": int(rng.choice([1, 4, 16])) * 2**30 * 1000},
                     sorted(rng.choice(T, size=min(T, n_opts), replace=False).tolist())))
ctx = kpamd.Context(0)
ch = kpamd.Catalog(ctx, cat)
plan = kpamd.LaunchPlan(ctx, ch, requests, catalog.ZONES, max_types=max_types)
mt, stride = plan.max_types, plan.max_types * len(catalog.ZONES)
arena = abi.Arena()
am, n_amis = abi.amis(arena, AMIS)  # the binding's marshalling is not timed: a shim fills the structs itself
out = (abi.LaunchResult * n)()
types = np.zeros(n * mt, dtype=np.uint32)
flat = np.zeros(n * stride, dtype=np.uint32)
lt = np.zeros(n, dtype=abi.lt_result_dtype())
tcfg = np.zeros(n * mt, dtype=np.int32)
cfgs = np.zeros(n * stride, dtype=abi.lt_config_dtype())
ovr = np.zeros(n * stride, dtype=np.uint32)
st = abi.SolveStats()
u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))


def templates(read=True):
    """One kp_launch_run_templates: (wall ms, host compile ms, device ms); copy-back = wall - device - compile."""
    t0 = time.perf_counter()
    rc = lib.kp_launch_run_templates(plan.h, am, n_amis, out if read else None, u32(types) if read else None,
                                     lt.ctypes.data if read else None, tcfg.ctypes.data if read else None,
                                     cfgs.ctypes.data if read else None, ovr.ctypes.data if read else None, C.byref(st))
    wall = (time.perf_counter() - t0) * 1e3
    assert rc == 0, lib.kp_last_error()
    return wall, st.prepare_ms, st.device_ms


def launch(read=True):
    t0 = time.perf_counter()
    rc = lib.kp_launch_run(plan.h, out if read else None, u32(types) if read else None, u32(flat) if read else None,
                           C.byref(st))
    wall = (time.perf_counter() - t0) * 1e3
    assert rc == 0, lib.kp_last_error()
    return wall, 0.0, st.device_ms


t0 = time.perf_counter()
templates()  # the plan's type table (LtBuild), code objects
first_ms = (time.perf_counter() - t0) * 1e3
templates()
launch()
launch()
if os.environ.get("PROFILE"):
    for _ in range(3):
        templates()
    plan.close()
    sys.exit(0)


def spread(runs, k):
    v = [r[k] for r in runs]
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


runs_t, runs_l, runs_tn, runs_ln = [], [], [], []
for _ in range(rounds):  # alternated: the two share the machine's noise
    runs_t.append(templates())
    runs_l.append(launch())
    runs_tn.append(templates(read=False))
    runs_ln.append(launch(read=False))
templates()
ok = sum(int(r["status"] == abi.LT_OK) for r in lt)
n_cfg = int(lt["n_configs"].sum())
n_ovr = int(sum(int(out[i].n_overrides) for i in range(n) if out[i].status == 0))
n_sel = int(sum(int(out[i].n_types) for i in range(n) if out[i].status == 0))
res = {"requests": n, "options": n_opts, "max_types": max_types, "types": T, "amis": n_amis, "zones": len(catalog.ZONES),
       "rounds": rounds,
       "first_call_ms": round(first_ms, 3), "lt_ok": ok, "configs": n_cfg, "selected_types": n_sel, "overrides": n_ovr,
       "templates": {"wall_ms": spread(runs_t, 0), "host_compile_ms": spread(runs_t, 1), "device_ms": spread(runs_t, 2)},
       "templates_no_copy_back": {"wall_ms": spread(runs_tn, 0), "device_ms": spread(runs_tn, 2)},
       "launch_run_alone": {"wall_ms": spread(runs_l, 0), "device_ms": spread(runs_l, 2)},
       "launch_run_alone_no_copy_back": {"wall_ms": spread(runs_ln, 0), "device_ms": spread(runs_ln, 2)},
       "copy_back_bytes": int(C.sizeof(out) + types.nbytes + lt.nbytes + tcfg.nbytes + cfgs.nbytes + ovr.nbytes),
       # byte floors. lt_ami_kernel: per listed type the rows' counts of the keys the AMIs name (4 B each, at most two
       # keys here) and one value word per named value (8 B), the map out (4 B). lt_group_kernel: per request the launch
       # record and its requirement set (48 + 904 B), per selected type its index, AMI, two capacities and its offering
       # classes and prices (4 + 4 + 16 + 9 + 72 B), the type's config (4 B); per config 32 B, per override 4 B; 16 B out
       "ami_kernel_floor_bytes": T * (2 * 4 + 3 * 8 + 4),
       "group_kernel_floor_bytes": n * (48 + 904 + 16) + n_sel * (4 + 4 + 16 + 9 + 72 + 4) + 32 * n_cfg + 4 * n_ovr}
import ltgroup_ref as ref  # noqa: E402
idx = sorted(rng.choice(n, size=min(n, sample), replace=False).tolist())
t0 = time.perf_counter()
want = ref.launch_templates(cat, [requests[i] for i in idx], catalog.ZONES, AMIS, max_types)
res["reference_cpu_ms_per_request"] = round((time.perf_counter() - t0) * 1e3 / len(idx), 3)
got = []
for i in idx:
    base = abi.launch_result_dict(out[i], types[i * mt:(i + 1) * mt], ovr[:0], catalog.ZONES)
    del base["overrides"]
    base["n_overrides"] = int(out[i].n_overrides)
    got.append(abi.launch_templates_dict(base, lt[i], tcfg[i * mt:(i + 1) * mt], cfgs[i * stride:(i + 1) * stride],
                                         ovr[i * stride:(i + 1) * stride], catalog.ZONES, AMIS, cat))
res["equal_to_reference"] = bool(got == want)
assert got == want, "the device's configs differ from the reference's on the sample"
plan.close()
ch.close()
print(json.dumps(res), flush=True)
