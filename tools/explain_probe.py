"""Explained-Solve probe: kp_solve_run_explained against kp_solve_run on one plan, alternated, on the config-5 limits
problem (cpu limits divided by 10: 38.9 % of 100k pods unschedulable), and the bytes the two explanation kernels must
read. usage: explain_probe.py [pods] [limit_div] [rounds]
  PROFILE=1: one warm-up pair and one explained run only (the process a `rocprofv3 --kernel-trace --stats` run wraps)."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "karpenter-provider-aws_amd"))
import kpamd  # noqa: E402
from kpamd import catalog, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
div = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
lib = kpamd.load_lib()
cat = catalog.build_catalog(lib)
prob = synth.config5(cat, n_pods=n, limit_div=div)
ctx = kpamd.Context(0)
plan = kpamd.Scheduler(ctx, prob).prepare()


def timed(explain):
    t0 = time.perf_counter()
    st = plan.run(read=False, explain=explain)["stats"]
    return (time.perf_counter() - t0) * 1e3, st["host_ms"], st["device_ms"]


timed(False), timed(True)  # warm-up: code objects, first touches of the explanation block
if os.environ.get("PROFILE"):
    timed(True)
    plan.close()
    sys.exit(0)
runs = {False: [], True: []}
for _ in range(rounds):
    for explain in (False, True):
        runs[explain].append(timed(explain))
res = plan.run(explain=True)
plain = plan.run()
failed = [p for p in res["reasons"]]
levels = {tuple((r["code"], r["n_types"], r["n_remaining"]) for r in rows) for rows in res["reasons"].values()}
# the bytes the kernels must read: explain_mark_kernel placement + shape + level per pod (12 B) and writes a row index
# (4 B); explain_kernel per marked (shape-level, template) pair the template's option words and, per limited resource,
# one capacity row of the catalogue (the limits filter), plus the two requirement sets
T = len(cat)
TW = (T + 63) // 64
n_tmpl = len(prob.nodepools)
out = {"pods": n, "limit_div": div, "rounds": rounds, "unschedulable": len(failed),
       "same_placement_as_plain": bool((res["placement"] == plain["placement"]).all()),
       "distinct_reason_rows": len(levels), "failed_shapes": len({int(prob.pod_shape[p]) for p in failed}),
       "shapes": len(prob.shapes), "types": T,
       "codes": sorted({r["code"] for rows in res["reasons"].values() for r in rows}),
       "mark_kernel_bytes": 16 * n,
       "explain_pair_bytes_limits_only": TW * 8 + T * 8 + 2 * 1024,
       "templates": n_tmpl}
for explain, key in ((False, "plain"), (True, "explained")):
    wall = [r[0] for r in runs[explain]]
    host = [r[1] for r in runs[explain]]
    out[key] = {"wall_ms_median": round(statistics.median(wall), 3), "wall_ms_min": round(min(wall), 3),
                "wall_ms_max": round(max(wall), 3), "host_ms_median": round(statistics.median(host), 3),
                "device_ms_median": round(statistics.median(r[2] for r in runs[explain]), 3)}
out["delta_wall_ms_median"] = round(out["explained"]["wall_ms_median"] - out["plain"]["wall_ms_median"], 3)
plan.close()
print(json.dumps(out), flush=True)
