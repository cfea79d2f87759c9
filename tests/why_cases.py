"""Crafted inputs for kp_cluster_simulate_explained, each with its hand-written expected kp_sim_why record - TEST
INFRASTRUCTURE. The builders take catalogues and helpers from tests/option_order_cases.py and write prices, labels and
pods so that the exit of every subset can be read off the construction; none of the expected records is computed by the
reference (tests/why_ref.py) or by the library - tests/test_why_ref.py holds the reference to them, the GPU tests the
device.

case(name) -> (cluster, subsets, {multi_node: [expected record per subset]})"""
import functools
import math

import numpy as np

import option_order_cases as oc
from why_ref import (MULTIPLE_NODECLAIMS, NONE, NOT_CHEAPER, SAME_TYPE, SPOT_FLEXIBILITY, SPOT_TO_SPOT_DISABLED, UNPRICED,
                     UNSCHEDULABLE, record)

ZONE, IT, CT = oc.ZONE, oc.IT, oc.CT
UP = lambda x: math.nextafter(x, math.inf)  # noqa: E731
BIG = {"cpu": 64_000, "memory": 256 * (1 << 30) * 1000, "pods": 500_000}
FULL = {"cpu": 0, "memory": 0, "pods": 0}


def _pod(cpu=500, mem_mi=1024, **kw):
    return oc._pod_shape((cpu, mem_mi), **kw)


def _cluster(its, nodes, shapes, pools, name, pending=(), spot_to_spot=False):
    """nodes: dicts {type, pods: [shape per pod], ct, zone, available, taints, initialized, deleting, labels}. Pods are
    numbered node by node, then the pending ones; every creation time and UID is distinct, so the queue order is the
    requests' (cpu descending, then memory)."""
    from kpamd import catalog as cmod, synth
    from kpamd.model import Cluster, ClusterNode, ExistingNode
    cnodes, pod_shape = [], []
    for i, n in enumerate(nodes):
        t = n["type"]
        labels = synth.node_labels(its[t], cmod.ZONES.index(n.get("zone", oc.ZA)), n.get("ct", "on-demand"), "default",
                                   f"node-{i:05d}")
        labels.update(n.get("labels", {}))
        pods = list(range(len(pod_shape), len(pod_shape) + len(n["pods"])))
        pod_shape += n["pods"]
        en = ExistingNode(f"node-{i:05d}", labels, dict(n.get("available", FULL)), {}, list(n.get("taints", [])),
                          n.get("initialized", True))
        cnodes.append(ClusterNode(en, 0, t, pods, deleting=n.get("deleting", False)))
    first_pending = len(pod_shape)
    pod_shape += list(pending)
    n = len(pod_shape)
    return Cluster([its], pools, cnodes, shapes, np.asarray(pod_shape, dtype=np.uint32),
                   (1_750_000_000 + np.arange(n)).astype(np.int64), np.arange(1, n + 1, dtype=np.uint64),
                   candidates=[i for i, x in enumerate(cnodes) if not x.deleting], name=name,
                   pending=list(range(first_pending, n)), spot_to_spot=spot_to_spot)


def _pool(reqs, **kw):
    from kpamd.model import NodePool
    return NodePool("default", 0, 0, list(reqs), **kw)


# ---- the price filter across the two lane halves ---------------------------------------------------------------------
LENGTHS = [1, 63, 64, 65, 129]  # options the pod admits; Truncate cuts the last list to 100


def _layout(n):
    """Price by sorted position: three options tie at 0.25, then distinct rising prices."""
    return [0.25 if j < 3 else 0.25 + j / 4096 for j in range(n)]


def build_price(lib, spread=False):
    """One candidate per (list length, candidate price): its pod's node affinity names the first n positions of the
    layout. Candidate prices: exactly the cheapest option (strict <: NOT_CHEAPER with cheapest_launch == the price), one
    ulp above (REPLACE: n_cheaper counts the three ties), the prices at positions 63, 64 and 65 (n_cheaper 63, 64, 65
    where the list is that long: the count crosses the lane halves) and 5.0 (all)."""
    its = oc.fresh(lib)
    pr = _layout(max(LENGTHS))
    cand_prices = [0.25, UP(0.25), pr[63], pr[64], pr[65], 5.0]
    us = oc.usable(its)
    cands = us[:len(cand_prices)]
    ts = oc.shuffled_usable(its, max(LENGTHS), 41, skip=cands)
    oc.price_everywhere(its, ts, pr)
    for c, p in zip(cands, cand_prices):
        oc.price_on_demand(its[c], p)
    shapes = [_pod(required_terms=[[(IT, "In", [its[t].name for t in ts[:n]])]]) for n in LENGTHS]
    if spread:
        oc._spread(shapes)
    nodes, want = [], []
    for li, n in enumerate(LENGTHS):
        m = min(n, 100)
        for c, p in zip(cands, cand_prices):
            nodes.append({"type": c, "pods": [li]})
            k = sum(1 for j in range(m) if pr[j] < p)
            want.append(record(NONE if k else NOT_CHEAPER, n_nodeclaims=1, n_truncated=m, n_cheaper=k, n_same_type=k,
                               cheapest_launch=0.25))
    cl = _cluster(its, nodes, shapes, [_pool([(CT, "In", ["on-demand"])])], "why-price")
    # (no candidate's type is an option, so filterOutSameType passes the set on: the records do not depend on multi_node)
    return cl, [[i] for i in range(len(nodes))], {False: want, True: want}


def build_same_type(lib, spread=False):
    """Two candidates, X and a Y priced 2.0. X is the cheapest option (0.25): filterByPrice keeps the whole
    list, filterOutSameType caps the price at X's own and keeps nothing: SAME_TYPE. Without multi_node the set passes."""
    its = oc.fresh(lib)
    ts = oc.shuffled_usable(its, 120, 42, pods=2)
    pr = [0.25 + j / 4096 for j in range(len(ts))]
    oc.price_everywhere(its, ts, pr)
    x, y = ts[0], ts[110]
    oc.price_on_demand(its[y], 2.0)
    shapes = [_pod(), _pod()]
    if spread:
        oc._spread(shapes)
    cl = _cluster(its, [{"type": x, "pods": [0]}, {"type": y, "pods": [1]}], shapes,
                  [_pool([(CT, "In", ["on-demand"]), (IT, "In", [its[t].name for t in ts])])], "why-same-type")
    base = dict(n_nodeclaims=1, n_truncated=100, cheapest_launch=0.25)
    both = {True: record(SAME_TYPE, n_cheaper=100, n_same_type=0, **base),
            False: record(NONE, n_cheaper=100, n_same_type=100, **base)}
    # X alone: nothing is cheaper than the cheapest option; Y alone: every option but none of its own type
    x_alone = record(NOT_CHEAPER, **base)
    y_alone = record(NONE, n_cheaper=100, n_same_type=100, **base)
    return cl, [[0, 1], [0], [1]], {m: [both[m], x_alone, y_alone] for m in (False, True)}


# ---- the Solve's exits: unpriced candidates, unschedulable pods, uninitialized nodes, a second NodeClaim ---------------
def build_solve_exits(lib, spread=False):
    """One cluster, one exit per subset (see the list below the nodes). `free` is an empty initialized node only pods
    tolerating its taint reach, `fresh` an empty UNINITIALIZED node only the pods selecting its label reach. A pending pod
    no node or NodeClaim can take and a deleting node's pod (it lands on `fresh`: exempt) are queued in every simulation
    behind every other pod (they request the least cpu), and must never be counted."""
    its = oc.fresh(lib)
    ts = oc.shuffled_usable(its, 40, 43, pods=3)
    pr = [0.25 + j / 4096 for j in range(len(ts))]
    cand, cheap = [t for t in oc.usable(its) if t not in set(ts)][:2]
    oc.price_everywhere(its, ts, pr)
    oc.price_on_demand(its[cand], 1.0)
    oc.price_on_demand(its[cheap], 0.25)  # a candidate at exactly the cheapest option's price
    tol = [("why/free", "Equal", "yes", "NoSchedule")]
    nowhere = {ZONE: "test-zone-nowhere"}
    shapes = [_pod(),                                                       # 0: goes to a NodeClaim
              _pod(tolerations=tol),                                         # 1: goes to `free`
              _pod(1, 1, node_selector=nowhere),                             # 2: the pending pod, fits nothing
              _pod(2, 1, node_selector={"why/fresh": "yes"},                 # 3: goes to `fresh` only
                   tolerations=[("why/fresh", "Equal", "yes", "NoSchedule")]),
              _pod(node_selector={ZONE: oc.ZA}), _pod(node_selector={ZONE: oc.ZB}),  # 4, 5: one NodeClaim each
              _pod(4000, 1024, node_selector=nowhere),                       # 6: fails, first in its queue
              _pod(), _pod(), _pod(),                                        # 7-9: as 0 (a shape per pod of a subset, so
              _pod(tolerations=tol), _pod(tolerations=tol),                  # 10, 11: as 1   that the spread variant's
              _pod(2, 1, node_selector={"why/fresh": "yes"},                 # 12: as 3       per-shape hostname spread
                   tolerations=[("why/fresh", "Equal", "yes", "NoSchedule")])]  #           lets them share a node)
    q_good = len(shapes)   # 130 sizes, cpu descending with the index: the queue order is the index order
    shapes += [_pod(200 - k, 16, tolerations=tol) for k in range(130)]
    q_bad = len(shapes)
    shapes += [_pod(200 - k, 16, tolerations=tol, node_selector=nowhere) for k in range(130)]
    if spread:
        oc._spread(shapes)
    unpriced = {"labels": {ZONE: "test-zone-unpriced", "topology.k8s.aws/zone-id": "tstz1-none"}}

    def queue(*bad):
        return [(q_bad if k in bad else q_good) + k for k in range(130)]
    nodes = [{"type": cand, "pods": [0]}, dict(unpriced, type=cand, pods=[7]), {"type": cand, "pods": [8]},   # 0 1 2
             dict(unpriced, type=cand, pods=[9]),                                                             # 3
             {"type": cand, "pods": [], "available": BIG, "taints": [("why/free", "yes", "NoSchedule")]},     # 4 free
             dict(unpriced, type=cand, pods=[1]), {"type": cand, "pods": [10]}, {"type": cand, "pods": [11]}, # 5 6 7
             {"type": cand, "pods": queue(0)}, {"type": cand, "pods": queue(63)},                             # 8 9
             {"type": cand, "pods": queue(64)}, {"type": cand, "pods": queue(129)},                           # 10 11
             {"type": cand, "pods": queue(5, 70)},                                                            # 12
             {"type": cand, "pods": [], "available": BIG, "initialized": False, "labels": {"why/fresh": "yes"},
              "taints": [("why/fresh", "yes", "NoSchedule")]},                                                  # 13 fresh
             {"type": cand, "pods": [3]},                                                                     # 14
             {"type": cand, "pods": [12], "deleting": True},                                                  # 15
             {"type": cand, "pods": [4, 5]}, {"type": cand, "pods": [6, 4, 5]},                               # 16 17
             {"type": cheap, "pods": [0]}]                                                                    # 18
    cl = _cluster(its, nodes, shapes, [_pool([(CT, "In", ["on-demand"]), (IT, "In", [its[t].name for t in ts])])],
                  "why-solve-exits", pending=[2])
    first_pod = {}
    at = 0
    for i, n in enumerate(nodes):
        first_pod[i] = at
        at += len(n["pods"])
    one = dict(n_nodeclaims=1, n_truncated=40, cheapest_launch=0.25)
    cases = [
        ([0], record(NONE, n_cheaper=40, n_same_type=40, **one)),                  # REPLACE: 40 options below 1.0
        ([1, 0, 2], record(UNPRICED, unpriced=0, **one)),                           # the unpriced candidate first
        ([0, 2, 3], record(UNPRICED, unpriced=2, **one)),                           # ... and last of three
        ([5, 6, 7], record(NONE)),                                                  # unpriced, but no NodeClaim: DELETE
        ([8], record(UNSCHEDULABLE, n_unscheduled=1, first_unscheduled=first_pod[8] + 0)),
        ([9], record(UNSCHEDULABLE, n_unscheduled=1, first_unscheduled=first_pod[9] + 63)),
        ([10], record(UNSCHEDULABLE, n_unscheduled=1, first_unscheduled=first_pod[10] + 64)),
        ([11], record(UNSCHEDULABLE, n_unscheduled=1, first_unscheduled=first_pod[11] + 129)),
        ([12], record(UNSCHEDULABLE, n_unscheduled=2, first_unscheduled=first_pod[12] + 5)),   # the lower position wins
        ([14], record(UNSCHEDULABLE, n_unscheduled=1, first_unscheduled=first_pod[14])),        # only `fresh` takes it
        ([16], record(MULTIPLE_NODECLAIMS, n_nodeclaims=2)),
        ([17], record(MULTIPLE_NODECLAIMS, n_nodeclaims=2)),                        # a pod had failed before: not reported
        ([6], record(NONE)),                                                        # DELETE (the exempt and pending pods)
        ([18], record(NOT_CHEAPER, **one)),                                         # strict <: 0.25 is not below 0.25
    ]
    want = [w for _, w in cases]
    return cl, [s for s, _ in cases], {False: want, True: want}


# ---- NodePool limits: the second NodeClaim the limits no longer admit ------------------------------------------------
def build_limits(lib):
    """Two pods of 3 cpu that may only go to 4-cpu types, a remaining cpu limit of 4: the first NodeClaim takes the
    limit (subtractMax), the second pod finds no template and fails. Judged by the limits the pass began with, the second
    pod would open a second NodeClaim; the subset's own Solve says UNSCHEDULABLE with one NodeClaim."""
    its = oc.fresh(lib)
    four = [t for t in oc.usable(its) if its[t].capacity.get("cpu") == 4000 and oc.holds(its[t], 3000, 1024)][:20]
    cand = next(t for t in oc.usable(its) if t not in set(four))
    oc.price_everywhere(its, four, [0.25 + j / 4096 for j in range(len(four))])
    oc.price_on_demand(its[cand], 1.0)
    shapes = [_pod(3000, 1024), _pod(3001, 1024), _pod(500, 512)]
    nodes = [{"type": cand, "pods": [1, 0]}, {"type": cand, "pods": [2]}]
    pool = _pool([(CT, "In", ["on-demand"]), (IT, "In", [its[t].name for t in four])], limits={"cpu": 4000})
    cl = _cluster(its, nodes, shapes, [pool], "why-limits")
    want = [record(UNSCHEDULABLE, n_nodeclaims=1, n_unscheduled=1, first_unscheduled=1),   # pod 1 (3 cpu) is queued second
            record(NONE, n_nodeclaims=1, n_truncated=len(four), n_cheaper=len(four), n_same_type=len(four),
                   cheapest_launch=0.25)]
    return cl, [[0], [1]], {False: want, True: want}


# ---- the order trap: the spot-to-spot gate is off AND the truncated options break minValues ---------------------------
def build_gate_and_min_values(lib, spread=False):
    """option_order_cases.build_min_values_tie(swapped): 101 spot options over k families whose cheapest hundred hold
    k - 1, a NodePool asking for k. The candidate is spot and the feature gate is off, so an implementation that tests
    the gate first says SPOT_TO_SPOT_DISABLED; Truncate's check is the Solve's and comes first: UNSCHEDULABLE, the
    NodeClaim's pod lost. Next to it the unswapped catalogue, where the cut keeps k families: SPOT_TO_SPOT_DISABLED."""
    out = {}
    for swapped in (True, False):
        cats, claims, k, x, y = oc.build_min_values_tie(lib, swapped)
        its = cats[0]
        types = claims[0]["types"]
        for t in types:  # the harness priced on-demand in zone A; the candidates here are spot
            od = next(o.price for o in its[t].offerings if o.capacity_type == "on-demand" and o.zone == oc.ZA)
            for o in its[t].offerings:
                if o.capacity_type == "spot" and o.zone == oc.ZA:
                    o.price = od
        cand = next(t for t in oc.usable(its, capacity_types=("spot",)) if t not in set(types))
        for o in its[cand].offerings:
            o.price = 5.0
        shapes = [oc._pod_shape(oc.TINY, node_selector={ZONE: oc.ZA})]
        if spread:
            oc._spread(shapes)
        pool = _pool([(CT, "In", ["spot"]), (IT, "In", [its[t].name for t in types]), (oc.FAMILY, "Exists", [], k)])
        out[swapped] = _cluster(its, [{"type": cand, "pods": [0], "ct": "spot"}], shapes, [pool],
                                f"why-gate-min-values-{int(swapped)}", spot_to_spot=False)
    broken = record(UNSCHEDULABLE, n_nodeclaims=1, n_unscheduled=1, first_unscheduled=0)
    held = record(SPOT_TO_SPOT_DISABLED, n_nodeclaims=1, n_truncated=100, cheapest_launch=0.25)
    return out, [[0]], {True: {m: [broken] for m in (False, True)}, False: {m: [held] for m in (False, True)}}


def build_min_values_and_failing_pod(lib, spread=False):
    """The swapped catalogue above, on demand: the one NodeClaim's truncated options break minValues, so its pod fails,
    AND another pod of the candidate fits nothing. Both count, and the first in queue order is named: on node 0 the
    NodeClaim's pod is queued first (12m against 11m), on node 1 the pod that fits nothing (13m against 12m)."""
    cats, claims, k, x, y = oc.build_min_values_tie(lib, True)
    its = cats[0]
    types = claims[0]["types"]
    cand = next(t for t in oc.usable(its) if t not in set(types))
    oc.price_on_demand(its[cand], 5.0)
    nowhere = {ZONE: "test-zone-nowhere"}
    shapes = [_pod(12, 16, node_selector={ZONE: oc.ZA}), _pod(11, 16, node_selector=nowhere),
              _pod(13, 16, node_selector=nowhere), _pod(12, 16, node_selector={ZONE: oc.ZA})]
    if spread:
        oc._spread(shapes)
    pool = _pool([(CT, "In", ["on-demand"]), (IT, "In", [its[t].name for t in types]), (oc.FAMILY, "Exists", [], k)])
    cl = _cluster(its, [{"type": cand, "pods": [0, 1]}, {"type": cand, "pods": [2, 3]}], shapes, [pool],
                  "why-min-values-and-failing-pod")
    want = [record(UNSCHEDULABLE, n_nodeclaims=1, n_unscheduled=2, first_unscheduled=0),
            record(UNSCHEDULABLE, n_nodeclaims=1, n_unscheduled=2, first_unscheduled=2)]
    return cl, [[0], [1]], {False: want, True: want}


# ---- MinInstanceTypesForSpotToSpotConsolidation: 14 against 15 cheaper spot options ----------------------------------
def build_spot_flexibility(lib, gate, spread=False):
    """Twenty spot options: fifteen rising from 0.25, five at 2.0. Candidate 0 costs exactly the fifteenth's price, so
    fourteen are cheaper (strict <): one short, SPOT_FLEXIBILITY with n_same_type 14. Candidate 1 costs one ulp more:
    fifteen, REPLACE. gate False: the same two candidates with the feature gate off, SPOT_TO_SPOT_DISABLED."""
    its = oc.fresh(lib)
    pr = [0.25 + j / 4096 if j < 15 else 2.0 for j in range(20)]
    us = oc.usable(its, capacity_types=("spot",))
    cands = us[:2]
    pool_of = set(us)
    ts = [t for t in oc.shuffled_usable(its, 60, 44, skip=cands) if t in pool_of][:20]
    assert len(ts) == 20
    at = {t: j for j, t in enumerate(ts)}
    price = {cands[0]: pr[14], cands[1]: UP(pr[14])}
    for t, it in enumerate(its):
        for o in it.offerings:
            o.price = pr[at[t]] if t in at and o.capacity_type == "spot" else price.get(t, 0.0)
    shapes = [_pod(node_selector={ZONE: oc.ZA}), _pod(node_selector={ZONE: oc.ZA})]
    if spread:
        oc._spread(shapes)
    pool = _pool([(CT, "In", ["spot"]), (IT, "In", [its[t].name for t in ts])])
    cl = _cluster(its, [{"type": cands[0], "pods": [0], "ct": "spot"}, {"type": cands[1], "pods": [1], "ct": "spot"}],
                  shapes, [pool], f"why-spot-flexibility-{int(gate)}", spot_to_spot=gate)
    base = dict(n_nodeclaims=1, n_truncated=20, cheapest_launch=0.25)
    if gate:
        want = [record(SPOT_FLEXIBILITY, n_cheaper=14, n_same_type=14, **base),
                record(NONE, n_cheaper=15, n_same_type=15, **base)]
    else:
        want = [record(SPOT_TO_SPOT_DISABLED, **base), record(SPOT_TO_SPOT_DISABLED, **base)]
    return cl, [[0], [1]], {False: want, True: want}


# ---- named access (built once per process) ---------------------------------------------------------------------------
BATCHED = ("price", "same-type", "solve-exits", "limits", "gate-min-values-broken", "gate-min-values-held",
           "min-values-failing-pod", "spot-flexibility", "spot-flexibility-gate-off")
GENERAL = ("price-spread", "same-type-spread", "solve-exits-spread", "gate-min-values-broken-spread",
           "min-values-failing-pod-spread", "spot-flexibility-spread", "spot-flexibility-gate-off-spread")


@functools.lru_cache(maxsize=None)
def case(name):
    """(cluster, subsets, {multi_node: expected records})."""
    import kpamd
    lib = kpamd.load_lib()
    spread = name.endswith("-spread")
    base = name[:-len("-spread")] if spread else name
    if base == "price":
        return build_price(lib, spread)
    if base == "same-type":
        return build_same_type(lib, spread)
    if base == "solve-exits":
        return build_solve_exits(lib, spread)
    if base == "limits":
        return build_limits(lib)
    if base in ("gate-min-values-broken", "gate-min-values-held"):
        cls, subs, want = build_gate_and_min_values(lib, spread)
        swapped = base.endswith("broken")
        return cls[swapped], subs, want[swapped]
    if base == "min-values-failing-pod":
        return build_min_values_and_failing_pod(lib, spread)
    if base in ("spot-flexibility", "spot-flexibility-gate-off"):
        return build_spot_flexibility(lib, base == "spot-flexibility", spread)
    raise KeyError(name)
