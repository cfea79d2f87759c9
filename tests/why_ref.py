"""The expected kp_sim_why records (kp_cluster_simulate_explained), composed from what the oracle already gives - TEST
INFRASTRUCTURE. It shares no code with kpamd beyond the model dataclasses and abi marshalling (the budget rule is
restated in admissible() below).

  simulation's Solve   command_ref.simulate(cluster, subset): the oracle's WHOLE Solve of SimulateScheduling's Problem
                       (it honours the NodePools' limits NodeClaim by NodeClaim, and has applied Truncate's minValues
                       check: a NodeClaim whose truncated options break minValues stays listed and has lost its pods)
  unscheduled fields   drift_ref.verdict on that Solve
  prices and filters   command_ref.candidate_price, e2e.worst_launch_price, command_ref.satisfies_min_values, restated in
                       the order kp_abi.h gives for enum kp_unconsolidatable

why() returns the record next to the decision it implies, so that tests/test_why_ref.py can hold the restated order to
the oracle's own computeConsolidation for every subset the GPU tests use."""
import copy
import functools
import gzip
import json
import math
import os
import struct

import command_ref
import e2e

CT = e2e.CT
(NONE, BUDGET, MULTIPLE_NODECLAIMS, UNSCHEDULABLE, UNPRICED, SPOT_TO_SPOT_DISABLED, NOT_CHEAPER, SAME_TYPE,
 SPOT_FLEXIBILITY, MIN_VALUES) = range(10)
COUNT = 10
FIELDS = ("reason", "stage", "n_nodeclaims", "n_unscheduled", "first_unscheduled", "unpriced", "n_truncated",
          "n_cheaper", "n_same_type", "cheapest_launch")
DBL_MAX = 1.7976931348623157e308


def record(reason=NONE, **kw):
    """A record with every field at its "stage not reached" value, then kw."""
    r = {"reason": reason, "stage": 0, "n_nodeclaims": 0, "n_unscheduled": 0, "first_unscheduled": -1, "unpriced": -1,
         "n_truncated": 0, "n_cheaper": 0, "n_same_type": 0, "cheapest_launch": 0.0}
    assert set(kw) <= set(r), kw
    r.update(kw)
    return r


def bits(r):
    """A record (or kp_sim_result dict) with its floats as their bit patterns: what == compares in the tests."""
    return tuple((k, struct.pack("<d", v).hex() if isinstance(v, float) else int(v)) for k, v in sorted(r.items()))


def why(cluster, subset, multi_node, verdict, solve):
    """(record, decision) of one simulation from its oracle Solve: the first exit that holds, in kp_abi.h's order."""
    subset = [int(c) for c in subset]
    ncs = solve["nodeclaims"]
    if len(ncs) > 1:  # stated difference from upstream: nothing of the unfinished Solve is reported
        return record(MULTIPLE_NODECLAIMS, n_nodeclaims=2), command_ref.NOOP
    r = record(n_nodeclaims=len(ncs), n_unscheduled=int(verdict["n_unscheduled"]),
               first_unscheduled=int(verdict["first_unscheduled"]))
    if not verdict["feasible"]:
        r["reason"] = UNSCHEDULABLE
        return r, command_ref.NOOP
    if not ncs:
        return r, command_ref.DELETE
    nc = ncs[0]
    cat = cluster.catalogs[cluster.nodepools[nc["nodepool"]].catalog]
    reqs = list(nc["requirements"])
    opts = [int(t) for t in nc["options"]]
    if not opts:  # Truncate broke minValues and the NodeClaim held pending pods only: its pods fail all the same
        r["reason"] = UNSCHEDULABLE
        return r, command_ref.NOOP
    prices = []
    for c in subset:
        n = cluster.nodes[c]
        prices.append(command_ref.candidate_price(cluster.catalogs[n.catalog][n.instance_type], n.node.labels))
    cand_price = 0.0
    for p in prices:  # (summed in candidate order: float addition order matters)
        cand_price += p if p is not None else 0.0
    all_spot = all(cluster.nodes[c].node.labels.get(CT) == "spot" for c in subset)
    s2s = all_spot and e2e._has(reqs, CT, "spot")
    wlp = {t: min(e2e.worst_launch_price(cat[t], reqs, s2s), DBL_MAX) for t in opts}
    r["n_truncated"] = len(opts)
    r["cheapest_launch"] = min(wlp.values())
    if any(p is None for p in prices):
        r.update(reason=UNPRICED, unpriced=next(i for i, p in enumerate(prices) if p is None))
        return r, command_ref.NOOP
    if s2s and not cluster.spot_to_spot:
        r["reason"] = SPOT_TO_SPOT_DISABLED
        return r, command_ref.NOOP
    kept = [t for t in opts if wlp[t] < cand_price]
    r["n_cheaper"] = len(kept)
    if not kept:
        r["reason"] = NOT_CHEAPER
        return r, command_ref.NOOP
    if not command_ref.satisfies_min_values(cat, kept, reqs):
        r.update(reason=MIN_VALUES, stage=1)
        return r, command_ref.NOOP
    if multi_node:  # filterOutSameType: the cheapest candidate of a kept option's type caps the price
        same = {}
        for c, p in zip(subset, prices):
            n = cluster.nodes[c]
            name = cluster.catalogs[n.catalog][n.instance_type].name
            same[name] = min(same.get(name, math.inf), p)
        mx = min([same[cat[t].name] for t in kept if cat[t].name in same] or [math.inf])
        mx = min(mx, DBL_MAX)
        kept = [t for t in kept if wlp[t] < mx]
        r["n_same_type"] = len(kept)
        if not kept:
            r["reason"] = SAME_TYPE
            return r, command_ref.NOOP
        if not command_ref.satisfies_min_values(cat, kept, reqs):
            r.update(reason=MIN_VALUES, stage=2)
            return r, command_ref.NOOP
    else:
        r["n_same_type"] = len(kept)
    if s2s and len(subset) == 1 and len(kept) < 15:
        r["reason"] = SPOT_FLEXIBILITY
        return r, command_ref.NOOP
    return r, command_ref.REPLACE


def reference(cluster, subsets, multi_node=True, allowed=None, solves=None):
    """What ClusterPlan.simulate_explained(subsets, multi_node, allowed) must return as whys and counts, plus the
    decision each record implies. A budget-blocked subset is BUDGET with every count 0. solves: a dict that keeps each
    subset's oracle Solve (it does not depend on multi_node)."""
    adm = [allowed is None or admissible(cluster, s, allowed) for s in subsets]
    whys, decisions = [], []
    for s, ok in zip(subsets, adm):
        if not ok:
            whys.append(record(BUDGET)), decisions.append(command_ref.NOOP)
            continue
        key = tuple(int(c) for c in s)
        if solves is None or key not in solves:
            vs = command_ref.simulate(cluster, s)
            if solves is not None:
                solves[key] = vs
        else:
            vs = solves[key]
        w, d = why(cluster, s, multi_node, *vs)
        whys.append(w), decisions.append(d)
    return whys, histogram(whys), decisions


def admissible(cluster, subset, allowed):
    """The budget rule: no NodePool owns more of the subset's nodes (by their karpenter.sh/nodepool label) than
    allowed[pool]."""
    index = {p.name: i for i, p in enumerate(cluster.nodepools)}
    assert len(allowed) == len(cluster.nodepools)
    owned = {}
    for c in subset:
        p = index[cluster.nodes[int(c)].node.labels["karpenter.sh/nodepool"]]
        owned[p] = owned.get(p, 0) + 1
    return all(n <= int(allowed[p]) for p, n in owned.items())


def histogram(whys):
    counts = [0] * COUNT
    for w in whys:
        counts[w["reason"]] += 1
    return counts


class OracleWhyPlan:
    """The oracle behind ClusterPlan's simulate() and simulate_explained() (kpamd.disruption.unconsolidatable takes
    either)."""

    def __init__(self, cluster):
        self.cluster = cluster
        self.solves = {}

    def simulate(self, subsets, multi_node=True, allowed=None):
        from oracle import pyoracle
        return pyoracle.simulate_batch(self.cluster, subsets, multi_node=multi_node)

    def simulate_explained(self, subsets, multi_node=True, allowed=None, cancel=None):
        from oracle import pyoracle
        whys, counts, decisions = reference(self.cluster, subsets, multi_node, allowed, solves=self.solves)
        sims, _ = pyoracle.simulate_batch(self.cluster, subsets, multi_node=multi_node)
        for s, w in enumerate(whys):
            if w["reason"] == BUDGET:
                sims[s] = {"decision": 0, "nodepool": 0, "candidate_price": 0.0, "replacement_price": 0.0, "savings": 0.0,
                           "n_options": 0, "n_pods": 0}
        return sims, whys, counts, {}

    def close(self):
        pass


# ---- the named cases of the GPU tests (tests/test_gpu_why.py): command_ref's clusters, cut where the issue cuts them ----
BATCHED = ("config4", "min-values", "spot-to-spot-config4", "s2s-off", "host-ports", "budgets", "disruption-state")
GENERAL = ("spread", "spread-budgets", "anti-affinity", "reservations", "reserved-replacement")


@functools.lru_cache(maxsize=None)
def case(name):
    """(cluster, subsets, multi_node values, allowed): command_ref.case, with config4 cut to its first 120 subsets plus
    the one subset of its 399 whose exit is SAME_TYPE."""
    if name == "s2s-off":  # the spot candidates of spot-to-spot-config4 with the feature gate off
        cl, subs, multis, allowed = command_ref.case("spot-to-spot-config4")
        cl = copy.copy(cl)
        cl.spot_to_spot = False
        return cl, subs, multis, allowed
    cl, subs, multis, allowed = command_ref.case(name)
    if name == "config4":
        subs = subs[:120] + [subs[SAME_TYPE_SUBSET]]
    return cl, subs, multis, allowed


SAME_TYPE_SUBSET = 375  # (tests/test_why_ref.py asserts it is the sweep's one SAME_TYPE exit)


@functools.lru_cache(maxsize=None)
def computed(name, multi_node):
    cl, subs, _, allowed = case(name)
    return reference(cl, subs, multi_node, allowed, solves=command_ref._SOLVES.setdefault(name, {}))


GOLDEN = command_ref.GOLDEN


def _golden_path(name, multi_node):
    return os.path.join(GOLDEN, f"why_{name}_{int(bool(multi_node))}.json.gz")


def write_golden(name, multi_node):
    whys, counts, decisions = computed(name, multi_node)
    doc = {"whys": [dict(w, cheapest_launch=float(w["cheapest_launch"]).hex()) for w in whys], "counts": counts,
           "decisions": decisions}
    os.makedirs(GOLDEN, exist_ok=True)
    with gzip.GzipFile(_golden_path(name, multi_node), "wb", mtime=0) as f:
        f.write(json.dumps(doc, sort_keys=True).encode())


@functools.lru_cache(maxsize=None)
def expected(name, multi_node):
    """(whys, counts, decisions) of a named case as recorded under tests/golden/ (floats stored as hex: exact)."""
    with gzip.open(_golden_path(name, multi_node), "rb") as f:
        doc = json.loads(f.read().decode())
    whys = [dict(w, cheapest_launch=float.fromhex(w["cheapest_launch"])) for w in doc["whys"]]
    return whys, doc["counts"], doc["decisions"]
