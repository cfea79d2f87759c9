"""Interruption probe: kp_cluster_interruptions on the reference benchmark's mix (makeDiverseMessagesAndNodes,
R:pkg/controllers/interruption/interruption_benchmark_test.go: a third scheduled_change, a third spot, the rest state
changes, each message naming a node of its own) at 100, 1,000, 5,000 and 15,000 messages, over a cluster of as many
nodes and over one large cluster, next to a single-threaded host hash-map join over the same marshalled inputs (a dict
in this interpreter: a yardstick for the shape of the cost, not for a compiled caller) and the plain-Python reference
(tests/interruption_ref.py) on a sample of the nodes, with equality asserted.
usage: interruption_probe.py [large cluster nodes] [rounds] [reference sample]
  PROFILE=1: the 15,000-message call on the large cluster only, two warm-up calls and three calls (the process a
  `rocprofv3 --kernel-trace --stats` run wraps)."""
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
from kpamd.model import Cluster, ClusterNode, ExistingNode, NodePool, PodShape  # noqa: E402
import interruption_ref as ref  # noqa: E402

big = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
sample = int(sys.argv[3]) if len(sys.argv) > 3 else 2_000
SIZES = (100, 1_000, 5_000, 15_000)
TYPES = ("m5.large", "m5.2xlarge", "c5.large", "t3.large", "r5.large", "c5.xlarge")
lib = kpamd.load_lib()
full = catalog.build_catalog(lib)
cat = [next(it for it in full if it.name == n) for n in TYPES]
ctx = kpamd.Context(0)
ch = kpamd.Catalog(ctx, cat)


def iid(n):
    return "i-" + format(n, "017x")


def cluster(n_nodes):
    """n_nodes spot nodes with the five labels the call and the plan read"""
    nodes = []
    for i in range(n_nodes):
        t = i % len(TYPES)
        labels = {ref.ITYPE: TYPES[t], ref.ZONE: catalog.ZONES[i % 3], "karpenter.sh/capacity-type": "spot",
                  "karpenter.sh/nodepool": "default", "kubernetes.io/hostname": f"node-{i}"}
        nodes.append(ClusterNode(ExistingNode(f"node-{i}", labels, {"cpu": 1000, "memory": 1 << 30, "pods": 100}), 0, t))
    empty = np.zeros(0, dtype=np.uint32)
    return Cluster([cat], [NodePool("default", 0, 0, [])], nodes, [PodShape({"cpu": 100, "memory": 128 << 20})], empty,
                   np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint64), name=f"probe-{n_nodes}")


def mix(n_messages, n_nodes, seed):
    rng = np.random.default_rng(seed)
    targets = rng.permutation(n_nodes)[:n_messages]
    return [((ref.SCHEDULED_CHANGE, ref.SPOT, ref.STOPPED if m % 2 else ref.TERMINATED)[m % 3], [iid(int(targets[m]))])
            for m in range(n_messages)]


def host_join(msgs, node_ids, deleting, pair_of):
    """The caller's join today: a hash map over the nodes' ids, one lookup per message id, the fold per node and the
    two lists. Returns what the device returns, as tuples."""
    by_id = {}
    for n, x in enumerate(node_ids):
        if x is not None:
            by_id.setdefault(x, []).append(n)
    first, kinds, count, matches = {}, {}, {}, []
    for m, (kind, ids) in enumerate(msgs):
        for x in ids:
            hit = by_id.get(x, ()) if kind else ()
            matches.append(len(hit))
            for n in hit:
                kinds[n] = kinds.get(n, 0) | (1 << kind)
                count[n] = count.get(n, 0) + 1
                if kind >= ref.SCHEDULED_CHANGE and n not in first:
                    first[n] = m
    deletes = [(n, first[n], msgs[first[n]][0]) for n in sorted(first) if not deleting[n]]
    carriers = {}
    for n in sorted(kinds):
        if kinds[n] & (1 << ref.SPOT) and pair_of[n] is not None:
            carriers.setdefault(pair_of[n], []).append(n)
    marks = sorted((ns[0], len(ns)) for ns in carriers.values())
    return matches, deletes, marks


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def measure(plan, cl, node_ids, msgs):
    n, e = len(node_ids), sum(len(i) for _, i in msgs)
    arena = abi.Arena()
    t0 = time.perf_counter()
    ii = abi.build_interrupt_in(arena, msgs, node_ids)  # the binding's marshalling: a shim fills the struct itself
    marshal_ms = (time.perf_counter() - t0) * 1e3
    nodes = np.zeros(max(n, 1), dtype=abi.interrupt_node_dtype())
    matches = np.zeros(max(e, 1), dtype=np.uint32)
    deletes = np.zeros(max(n, 1), dtype=abi.interrupt_delete_dtype())
    marks = np.zeros(max(n, 1), dtype=abi.interrupt_mark_dtype())
    nd, nm, st = C.c_uint32(0), C.c_uint32(0), abi.SolveStats()
    counts = (C.c_uint64 * abi.MESSAGE_KIND_COUNT)()

    def call(read=True):
        t0 = time.perf_counter()
        rc = lib.kp_cluster_interruptions(plan.h, C.byref(ii), nodes.ctypes.data if read else None,
                                          matches.ctypes.data if read else None, deletes.ctypes.data if read else None,
                                          C.byref(nd), marks.ctypes.data if read else None, C.byref(nm), counts, C.byref(st))
        wall = (time.perf_counter() - t0) * 1e3
        assert rc == 0, lib.kp_last_error()
        return wall, st.device_ms, st.host_ms

    t0 = time.perf_counter()
    call()  # the plan's pair table (InterruptBuild), code objects
    first_ms = (time.perf_counter() - t0) * 1e3
    call()
    if os.environ.get("PROFILE"):
        for _ in range(3):
            call()
        return None
    runs, runs_n, host = [], [], []
    deleting = [nd_.deleting for nd_ in cl.nodes]
    pair_of = [(nd_.node.labels[ref.ITYPE], nd_.node.labels[ref.ZONE]) for nd_ in cl.nodes]
    for _ in range(rounds):
        runs.append(call())
        runs_n.append(call(read=False))
        t0 = time.perf_counter()
        hj = host_join(msgs, node_ids, deleting, pair_of)
        host.append((time.perf_counter() - t0) * 1e3)
    call()
    got = ([int(x) for x in matches[:e]], [(int(r["node"]), int(r["message"]), int(r["kind"])) for r in deletes[:nd.value]],
           [(int(r["node"]), int(r["n_nodes"])) for r in marks[:nm.value]])
    assert got == hj, "the device differs from the host join"
    # the reference on a sample of the nodes: its records against the device's
    want = ref.resolve(cl, msgs, node_ids)
    idx = sorted(np.random.default_rng(3).choice(n, size=min(n, sample), replace=False).tolist())
    for i in idx:
        assert {f: int(nodes[i][f]) for f in nodes.dtype.names} == want["nodes"][i], i
    assert [int(c) for c in counts] == want["counts"]
    slots = 2
    while slots < 2 * (n + 1):
        slots <<= 1
    return {"messages": len(msgs), "ids": e, "nodes": n, "table_slots": slots, "deletes": int(nd.value), "marks": int(nm.value),
            "first_call_ms": round(first_ms, 3), "marshal_ms": round(marshal_ms, 3),
            "wall_ms": spread([r[0] for r in runs]), "device_ms": spread([r[1] for r in runs]),
            "host_ms": spread([r[2] for r in runs]),
            "no_copy_back": {"wall_ms": spread([r[0] for r in runs_n]), "device_ms": spread([r[1] for r in runs_n])},
            "host_join_python_ms": spread(host),
            "upload_bytes": 33 * n + 36 * e + len(msgs), "copy_back_bytes": 16 * n + 4 * e + 16 * int(nd.value) + 8 * int(nm.value),
            # byte floors: fills 4 B per word of the table and the six accumulator arrays; build a key, a flag and a
            # slot per node; probe a key, a message index, a kind and a count per entry, a slot and a node key per
            # step of a hit (one step at least), three atomics per match; resolve five words in and 16 B out per node;
            # count and scatter the 16 B record per node, scatter also each list record
            "floor_bytes": {"fills": 4 * (slots + 4 * n + 12), "build": 37 * n, "probe": 41 * e + 48 * sum(got[0]),
                            "resolve": 33 * n, "count": 16 * n, "scatter": 16 * n + 16 * int(nd.value) + 8 * int(nm.value)},
            "equal_to_host_join": True, "reference_sample": len(idx)}


res = {"rounds": rounds, "large_cluster": big, "runs": []}
big_cl = cluster(big)
big_ids = [iid(i) for i in range(big)]
t0 = time.perf_counter()
big_plan = kpamd.ClusterPlan(ctx, big_cl, catalogs=[ch])
res["large_cluster_prepare_s"] = round(time.perf_counter() - t0, 3)
if os.environ.get("PROFILE"):
    measure(big_plan, big_cl, big_ids, mix(SIZES[-1], big, 1))
    big_plan.close()
    sys.exit(0)
for m in SIZES:
    cl = cluster(m)
    ids = [iid(i) for i in range(m)]
    plan = kpamd.ClusterPlan(ctx, cl, catalogs=[ch])
    res["runs"].append(measure(plan, cl, ids, mix(m, m, m)))
    plan.close()
    res["runs"].append(measure(big_plan, big_cl, big_ids, mix(m, big, m + 1)))
    print(json.dumps(res["runs"][-2]), flush=True)
    print(json.dumps(res["runs"][-1]), flush=True)
big_plan.close()
ch.close()
print(json.dumps(res), flush=True)
