"""Catalogue-compile probe: Context.compile_catalogs (one kp_catalog_compile call) against the way the same tables
were made before it, in one process: N x T calls of kp_instance_type_resolve plus catalog.create_offerings per pair
(Python, over the NodeClass's subnet zones). Prints the whole call, its host-compile share, the kernels' time from
the HIP events, and the bytes each kernel must move (kernel_floor_us_at_8TBps is those bytes as one coalesced stream:
the resolve kernel's stores are 104 bytes apart per lane, so it is not a bound that kernel can reach).
usage: catcomp_probe.py [nodeclasses] [types] [zones] [rounds]
  PROFILE=1: two warm-up calls and three calls only (the process a `rocprofv3 --kernel-trace --stats` run wraps); the
  old way is not run."""
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
import kpamd  # noqa: E402
from kpamd import abi, catalog  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
T = int(sys.argv[2]) if len(sys.argv) > 2 else 919
Z = int(sys.argv[3]) if len(sys.argv) > 3 else 6
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 9
lib = kpamd.load_lib()
rows = catalog.load_ec2_table()[:T]
T = len(rows)
zones = [f"test-zone-1{chr(ord('a') + z)}" for z in range(Z)]
zone_ids = [f"tstz1-1{chr(ord('a') + z)}" for z in range(Z)]
FAMILIES = ["AL2023", "AL2", "Bottlerocket", "Windows2022", "Custom"]


def nodeclass_kwargs(n):
    """NodeClass n: three of the zones, and a mix of families, pod-density knobs and kubelet blocks"""
    pick = sorted({(n + k) % Z for k in range(min(3, Z))})
    kw = dict(zones=[zones[z] for z in pick], zone_ids=[zone_ids[z] for z in pick], ami_family=FAMILIES[n % len(FAMILIES)])
    if n % 3 == 1:
        kw["max_pods"] = 30 + n
    if n % 4 == 2:
        kw["pods_per_core"] = 2 + n % 5
    if n % 2:
        kw["kubelet_cfg"] = dict(kube_reserved={"cpu": f"{100 + n}m"}, system_reserved={"memory": f"{100 + n}Mi"},
                                 eviction_hard={"memory.available": f"{5 + n % 7}.5%", "nodefs.available": "10%"})
    if n % 8 == 7:
        kw["instance_store_policy"] = "RAID0"
    return kw


ncs = [nodeclass_kwargs(n) for n in range(N)]
spot = catalog.default_spot_prices(rows, zones)
unavailable = [("spot", rows[t]["name"], zones[t % Z]) for t in range(0, T, 17)]
ctx = kpamd.Context(0)
arena = abi.Arena()
cin = kpamd.build_compile_in(arena, ctx.opts, rows, ncs, zones, spot_prices=spot, unavailable=unavailable)
# (the binding's marshalling is not timed on either side: a shim fills the structs itself)


def call():
    t0 = time.perf_counter()
    tab = kpamd._catalog_compile_raw(lib, ctx.h, cin)
    wall = (time.perf_counter() - t0) * 1e3
    s = tab["stats"]
    return (wall, s["host_ms"], s["prepare_ms"], s["device_ms"]), tab


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
tab = call()[1]

# the old way: one (NodeClass, type) pair per kp_instance_type_resolve call, createOfferings in Python
infos = [catalog.ec2_info(arena, r) for r in rows]
nodeclasses = [catalog.nodeclass(arena, **kw) for kw in ncs]
cap = (abi.ResourceList * (N * T))()
ovh = (abi.ResourceList * (N * T))()
t0 = time.perf_counter()
for n in range(N):
    for t in range(T):
        lib.kp_instance_type_resolve(C.byref(ctx.opts), C.byref(infos[t]), C.byref(nodeclasses[n]),
                                     C.byref(cap[n * T + t]), C.byref(ovh[n * T + t]))
resolve_ms = (time.perf_counter() - t0) * 1e3
reqs = {}
for kw in ncs:  # the label half is the caller's on both sides: not timed
    key = tuple(kw["zones"])
    if key not in reqs:
        reqs[key] = [catalog.compute_requirements(r, zones=kw["zones"], zone_ids=kw["zone_ids"]) for r in rows]
unav = frozenset(unavailable)
t0 = time.perf_counter()
offerings = [[catalog.create_offerings(r, reqs[tuple(kw["zones"])][t], spot, kw["zones"], kw["zone_ids"], unav)
              for t, r in enumerate(rows)] for kw in ncs]
offerings_ms = (time.perf_counter() - t0) * 1e3

rl = abi.resource_list_dtype()
equal = all((tab[k][f] == np.frombuffer(a, dtype=rl).reshape(N, T)[f]).all()
            for k, a in (("capacity", cap), ("overhead", ovh)) for f in ("milli", "present"))
for n, kw in enumerate(ncs):  # the old offerings cover the subnet zones only
    for t in range(0, T, 7):
        for o in offerings[n][t]:
            z, c = zones.index(o.zone), abi.CAPACITY_TYPES.index(o.capacity_type)
            equal = equal and o.price == tab["price"][t, z, c] and o.available == bool(int(tab["available"][n, t, c]) >> z & 1)

R = cin.n_reservations
RL = 104  # sizeof(kp_resource_list)
W = max(1, (T + 63) // 64)
nbytes = {
    # per pair the five lists out; the type columns (9 x 4 B + 2 x 8 B) and the NodeClass records once each
    "catcomp_resolve_kernel": N * T * 5 * RL + T * 52 + N * 336,
    # per pair it_zones and the two availability words out; per type its zones, on-demand and spot prices in (re-read
    # per NodeClass from cache), the unavailable rows once
    "catcomp_offer_kernel": N * T * 24 + T * (16 + 8 * Z) + 2 * Z * W * 8,
    # per (type, zone) two prices in, two out; per reservation 16 B in, 16 B out
    "catcomp_price_kernel": T * Z * 16 + T * 8 + T * Z * 8 + R * 32,
}
out_bytes = N * T * (5 * RL + 8 + 16) + T * Z * 16 + R * 16
res = {"nodeclasses": N, "types": T, "zones": Z, "pairs": N * T, "unavailable": len(unavailable), "rounds": rounds,
       "first_call_ms": round(first_ms, 3), "wall_ms": spread(runs, 0), "host_ms": spread(runs, 1),
       "host_compile_ms": spread(runs, 2), "device_ms": spread(runs, 3),
       "host_compile_share": round(statistics.median(r[2] for r in runs) / statistics.median(r[1] for r in runs), 3),
       "copy_and_launch_ms": round(statistics.median(r[1] - r[2] - r[3] for r in runs), 4),
       "bytes_copied_back": out_bytes,
       "old_way_ms": {"kp_instance_type_resolve_calls": round(resolve_ms, 2), "create_offerings_python": round(offerings_ms, 2)},
       "equal_to_old_way": bool(equal),
       "kernel_bytes": nbytes, "kernel_floor_us_at_8TBps": {k: round(v / 8e12 * 1e6, 3) for k, v in nbytes.items()}}
print(json.dumps(res), flush=True)
