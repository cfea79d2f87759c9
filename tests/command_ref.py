"""The expected consolidation command (kp_cluster_command), composed from what the oracle already gives - TEST
INFRASTRUCTURE.

  decision           pyoracle.simulate_batch (the oracle's computeConsolidation)
  simulation's Solve simulate(cluster, subset): the oracle Solve of SimulateScheduling's Problem as drift_ref builds it
                     (same queue, existing nodes, strict reservations, 100 instance types), with the bound pods' host
                     ports on their nodes as kp_cluster has them
  filters            restated here in the order of the library's GeneralDecide / the oracle's kpo_simulate_batch:
                     minValues on the truncated options (the Solve has applied it: a NodeClaim whose truncated options
                     break minValues has lost its pods), e2e.worst_launch_price(...) < candidate price (filterByPrice),
                     filterOutSameType when multi_node, the 15 / 100 spot-to-spot cut; minValues re-checked after each
                     filter

reference() returns the sim dict the restatement arrives at next to the command, so that tests/test_command_ref.py can
hold the restatement to the oracle's own decision for every subset the GPU tests use."""
import copy
import functools
import gzip
import json
import math
import os

import numpy as np

import drift_ref
import e2e
from kpamd import abi

NOOP, DELETE, REPLACE = 0, 1, 2
CT = e2e.CT


def candidate_price(it, labels):
    """Offerings.Compatible(NewLabelRequirements(node labels)).Cheapest().Price, or None when no offering is
    label-compatible (availability does not matter: getCandidatePrices)."""
    reqs = [(k, "In", [v]) for k, v in labels.items()]
    ps = [o.price for o in it.offerings if e2e._offering_compatible(reqs, o)]
    return min(ps) if ps else None


def satisfies_min_values(cat, types, reqs):
    """InstanceTypes.SatisfiesMinValues: every key with minValues has that many distinct values over the types."""
    mins = [(r[0], r[3]) for r in reqs if len(r) > 3 and r[3] is not None]
    if not mins:
        return True
    if not types:
        return False
    for key, mv in mins:
        vals = set()
        for t in types:
            for r in cat[t].requirements:
                if r[0] == key:
                    vals.update(r[2])
        if len(vals) < mv:
            return False
    return True


def narrow_to_spot(reqs):
    """The spot-to-spot branch: karpenter.sh/capacity-type In [spot] replaces any other capacity-type requirement (keys
    stay in byte order, as the requirements are rendered)."""
    return sorted([r for r in reqs if r[0] != CT] + [(CT, "In", ["spot"], None)], key=lambda r: r[0])


def _has_topology(cluster):
    return any(sh.topology_spread or sh.required_anti_affinity or sh.preferred_anti_affinity or sh.required_affinity
               or sh.preferred_affinity for sh in cluster.shapes)


def simulate(cluster, subset):
    """(verdict dict, Solve result) of one subset's simulation on the oracle: drift_ref's Problem with the kp_cluster
    convention for host ports (a node's HostPortUsage holds its own entries plus those of every pod bound to it, as
    abi.build_cluster marshals it for the oracle's kpo_simulate_batch). Bound pods only seed topology domain counts, so
    a cluster without topology spread and pod (anti-)affinity passes none."""
    from oracle import pyoracle
    prob, kind, pods, ex_nodes = drift_ref.simulation_problem(cluster, subset)
    existing = []
    for i, ex in zip(ex_nodes, prob.existing):
        used = [hp for p in cluster.nodes[i].pods for hp in (cluster.shapes[int(cluster.pod_shape[p])].host_ports or [])]
        if used:
            ex = copy.copy(ex)
            ex.host_ports = list(ex.host_ports or []) + used
        existing.append(ex)
    prob.existing = existing
    if not _has_topology(cluster):
        prob.bound_pods = []
    res = _solve(prob)
    return drift_ref.verdict(prob, kind, pods, res), res


class _Arena(abi.Arena):
    """abi.Arena that marshals a catalogue once per process (a simulation's Problem carries the cluster's catalogues
    unchanged; marshalling the 919 types costs more than the oracle's Solve)."""
    descs = {}

    def catalog_desc(self, its):
        hit = _Arena.descs.get(id(its))
        if hit is None or hit[0] is not its:
            own = abi.Arena()
            hit = _Arena.descs[id(its)] = (its, own, own.catalog_desc(its))
        return hit[2]


def _solve(prob):
    """pyoracle.solve with the cached catalogue marshalling."""
    import ctypes as C
    from kpamd import read_result
    from oracle import pyoracle
    lib = pyoracle.load()
    arena = _Arena()
    si = abi.build_solve_in(arena, prob, catalog_handles=None)
    res = C.c_void_p()
    rc = lib.kpo_solve(C.byref(si), C.byref(res))
    assert rc == 0, f"kpo_solve = {rc}"
    try:
        return read_result(lib, res, prob.n_pods, prefix="kpo_result_")
    finally:
        lib.kpo_result_destroy(res)


def decide(cluster, subset, multi_node, verdict, solve):
    """(sim dict, command or None, info) from one simulation's oracle Solve."""
    subset = [int(c) for c in subset]
    prices = []
    for c in subset:
        n = cluster.nodes[c]
        prices.append(candidate_price(cluster.catalogs[n.catalog][n.instance_type], n.node.labels))
    priced = all(p is not None for p in prices)
    cand_price = 0.0
    for p in prices:  # (summed in candidate order: float addition order matters)
        cand_price += p if p is not None else 0.0
    sim = {"decision": NOOP, "nodepool": 0, "candidate_price": cand_price if priced else 0.0, "replacement_price": 0.0,
           "savings": 0.0, "n_options": 0, "n_pods": int(verdict["n_pods"])}
    info = {"truncated": 0, "after_price": 0, "after_same_type": 0, "kept": 0, "price_hole": False, "s2s": False,
            "on_existing": 0, "on_nodeclaim": 0}
    ncs = solve["nodeclaims"]
    if not verdict["feasible"]:
        return sim, None, info
    placement = np.asarray(solve["placement"], dtype=np.int32)
    info["on_existing"] = int((placement <= -2).sum())
    info["on_nodeclaim"] = int((placement >= 0).sum())
    if not ncs:
        sim.update(decision=DELETE, savings=sim["candidate_price"])
        return sim, {"placement": placement, "nodeclaims": []}, info
    if len(ncs) != 1 or not priced:
        return sim, None, info
    nc = ncs[0]
    cat = cluster.catalogs[cluster.nodepools[nc["nodepool"]].catalog]
    reqs = list(nc["requirements"])
    all_spot = all(cluster.nodes[c].node.labels.get(CT) == "spot" for c in subset)
    s2s = all_spot and e2e._has(reqs, CT, "spot")
    if s2s and not cluster.spot_to_spot:
        return sim, None, info
    info["s2s"] = s2s
    opts = [int(t) for t in nc["options"]]
    info["truncated"] = len(opts)
    wlp = {t: e2e.worst_launch_price(cat[t], reqs, s2s) for t in opts}
    keep = [wlp[t] < cand_price for t in opts]
    kept = [t for t, k in zip(opts, keep) if k]
    info["after_price"] = len(kept)
    info["price_hole"] = any((not keep[i]) and any(keep[i + 1:]) for i in range(len(keep)))
    if not satisfies_min_values(cat, kept, reqs) or not kept:
        return sim, None, info
    if multi_node:  # filterOutSameType: the cheapest candidate of a kept option's type caps the price
        same = {}
        for c, p in zip(subset, prices):
            if p is None:
                continue
            n = cluster.nodes[c]
            name = cluster.catalogs[n.catalog][n.instance_type].name
            same[name] = min(same.get(name, math.inf), p)
        mx = min([same[cat[t].name] for t in kept if cat[t].name in same] or [math.inf])
        mx = min(mx, 1.7976931348623157e308)
        kept = [t for t in kept if wlp[t] < mx]
        if not satisfies_min_values(cat, kept, reqs) or not kept:
            return sim, None, info
    info["after_same_type"] = len(kept)
    if s2s and len(subset) == 1:
        if len(kept) < 15:
            return sim, None, info
        has_min = any(len(r) > 3 and r[3] is not None for r in reqs)
        kept = kept[:100 if has_min else 15]
    info["kept"] = len(kept)
    best = min(wlp[t] for t in kept)
    sim.update(decision=REPLACE, nodepool=int(nc["nodepool"]), replacement_price=best, savings=cand_price - best,
               n_options=len(kept))
    out = dict(nc)
    out["options"] = kept
    out["requirements"] = narrow_to_spot(reqs) if s2s else reqs
    return sim, {"placement": placement, "nodeclaims": [out]}, info


def reference(cluster, subsets, multi_node=True, allowed=None, solves=None):
    """What ClusterPlan.command(subsets, multi_node, allowed) must return (without stats): (sim dicts, commands, infos).
    A budget-blocked subset is the zero no-op without a command. solves: a dict that keeps each subset's oracle Solve
    (the Solve does not depend on multi_node, so both values share it)."""
    from kpamd import disruption
    adm = [True] * len(subsets)
    if allowed is not None:
        offs = np.zeros(len(subsets) + 1, dtype=np.uint32)
        offs[1:] = np.cumsum([len(s) for s in subsets])
        flat = np.concatenate([np.asarray(s, dtype=np.uint32) for s in subsets] + [np.zeros(0, dtype=np.uint32)])
        adm = list(disruption.admissible(cluster, offs, flat, allowed))
    sims, cmds, infos = [], [], []
    for s, ok in zip(subsets, adm):
        if not ok:
            sims.append({"decision": 0, "nodepool": 0, "candidate_price": 0.0, "replacement_price": 0.0, "savings": 0.0,
                         "n_options": 0, "n_pods": 0})
            cmds.append(None), infos.append(None)
            continue
        key = tuple(int(c) for c in s)
        if solves is None or key not in solves:
            vs = simulate(cluster, s)
            if solves is not None:
                solves[key] = vs
        else:
            vs = solves[key]
        sim, cmd, info = decide(cluster, s, multi_node, *vs)
        sims.append(sim), cmds.append(cmd), infos.append(info)
    return sims, cmds, infos


def command_fields(cmd):
    """What the tests compare of a command: every placement, and per NodeClaim the NodePool, pods in add order, options,
    n_remaining, requirements and requests."""
    if cmd is None:
        return None
    return ([int(p) for p in cmd["placement"]],
            [(n["nodepool"], list(n["pods"]), list(n["options"]), n["n_remaining"], [tuple(r) for r in n["requirements"]],
              dict(n["requests"])) for n in cmd["nodeclaims"]])


class OracleCommandPlan:
    """The oracle behind ClusterPlan's simulate() and command() (kpamd.disruption.Controller takes either)."""

    def __init__(self, cluster):
        self.cluster = cluster
        self.calls = []

    def simulate(self, subsets, multi_node=True):
        from oracle import pyoracle
        self.calls.append("simulate")
        return pyoracle.simulate_batch(self.cluster, subsets, multi_node=multi_node)

    def command(self, subsets, multi_node=True, allowed=None, cancel=None):
        self.calls.append("command")
        sims, cmds, _ = reference(self.cluster, subsets, multi_node, allowed)
        return sims, cmds, {}

    def close(self):
        pass


# ---- the clusters and subsets of the GPU tests (tests/test_gpu_command.py), built once per process ------------------
POOL = "karpenter.sh/nodepool"
K = "karpenter.k8s.aws/"


def _spot_subsets(cl, n_single, n_multi, seed):
    spot = [c for c in cl.candidates if cl.nodes[c].node.labels.get(CT) == "spot"]
    rng = np.random.default_rng(seed)
    subs = [[c] for c in spot[:n_single]]
    subs += [sorted(rng.choice(spot, 3, replace=False).tolist(), key=cl.candidates.index) for _ in range(n_multi)]
    return subs


@functools.lru_cache(maxsize=None)
def _catalog():
    import kpamd
    from kpamd import catalog as cmod
    return cmod.build_catalog(kpamd.load_lib())


@functools.lru_cache(maxsize=None)
def case(name):
    """(cluster, subsets, multi_node values, allowed) of a named case."""
    from kpamd import synth
    from kpamd.model import NodePool
    catalog = _catalog()
    if name == "config4":
        cl = synth.config4(catalog, n_nodes=120, seed=4, loose=0.05)
        return cl, synth.consolidation_subsets(cl, 300, seed=5), (False, True), None
    if name == "disruption-state":  # pending and deleting-node pods (the placement index convention), binding limits
        base = synth.config4(catalog, n_nodes=120, seed=4, loose=0.05)
        cl = synth.with_disruption_state(base, 7, cpu_limit_m=4000)
        subs = [[c for c in s if not cl.nodes[c].deleting] for s in synth.consolidation_subsets(base, 30, seed=5)]
        subs = [s for s in subs if s][::3] + [[c] for c in cl.candidates[:12]]
        return cl, subs, (False, True), None
    if name == "spot-to-spot":
        cl = synth.random_cluster(catalog, 201, n_nodes=40)
        cl.spot_to_spot = True
        subs = _spot_subsets(cl, 15, 6, 1) + synth.consolidation_subsets(cl, 10, seed=1, max_size=10)
        return cl, [s for s in subs if s], (False, True), None
    if name == "spot-to-spot-config4":  # single spot candidates with more than 15 cheaper spot options: the cut
        cl = synth.config4(catalog, n_nodes=200, seed=11)
        cl.spot_to_spot = True
        return cl, _spot_subsets(cl, 12, 6, 1), (False, True), None
    if name == "host-ports":
        from test_hostports_volumes import cluster_with_ports
        cl = cluster_with_ports(catalog, 1)
        subs = synth.consolidation_subsets(cl, 25, seed=1, max_size=30) + [[c] for c in cl.candidates[:15]]
        return cl, subs, (True,), None
    if name == "min-values":  # a NodePool with instance-family minValues 40 on a 30-node config-4 cluster
        cl = synth.config4(catalog, n_nodes=30, seed=4, loose=0.05)
        cl.nodepools = [NodePool(p.name, p.weight, p.catalog, list(p.requirements) + [(K + "instance-family", "Exists", [], 40)])
                        for p in cl.nodepools]
        cl.spot_to_spot = True
        subs = synth.consolidation_subsets(cl, 20, seed=5, max_size=12) + [[c] for c in cl.candidates]
        return cl, subs, (False, True), None
    if name == "budgets":  # the two-pool relabelling of tests/test_gpu_budget_sweep.py
        cl = synth.config4(catalog, n_nodes=120, seed=4, loose=0.05)
        for i, n in enumerate(cl.nodes):
            n.node.labels[POOL] = "burst" if i % 3 == 0 else "default"
        subs = synth.consolidation_subsets(cl, 40, seed=5, max_size=24, prefixes=False) + [cl.candidates[:k] for k in range(2, 12)]
        return cl, subs, (True,), (6, 2)
    # ---- general-path plans (tests/test_gpu_command_general.py) ----
    if name in ("spread", "spread-budgets"):  # the 120-node spread cluster of tests/test_gpu_general_launches.py
        from test_gpu_budget_sweep import _two_pools
        from test_gpu_general_launches import _subsets
        cl = _two_pools(synth.spread_cluster(catalog, 120, seed=4))
        return cl, _subsets(cl), (True,), ((3, 0) if name == "spread-budgets" else None)
    if name == "anti-affinity":  # some subsets remove every owner of an inverse anti-affinity term: compiled alone
        from test_gpu_general_launches import anti_affinity_cluster
        cl, subs = anti_affinity_cluster(catalog)
        return cl, subs, (False, True), None
    if name == "reservations":
        import kpamd
        from test_reserved_consolidation import _reserve_nodes, reservation_cluster
        cl, crs = reservation_cluster(catalog, 70)
        cl = _reserve_nodes(kpamd.load_lib(), cl, crs, launch_into=True)
        subs = synth.consolidation_subsets(cl, 12, seed=70, max_size=4) + [[c] for c in cl.candidates[:8]]
        return cl, subs, (False, True), None
    if name == "reserved-replacement":  # an on-demand m5.xlarge replaced into an m5.large reservation: held ids
        import kpamd
        from kpamd import catalog as cmod
        from test_reserved_consolidation import ZONE_A, _catalogue, _cluster
        cr = cmod.CapacityReservation("cr-m5.large-1a", "m5.large", ZONE_A, "default", 1)
        cat = _catalogue(kpamd.load_lib(), ["m5.large", "m5.xlarge", "m5.2xlarge"], [cr])
        return _cluster(cat, "m5.xlarge", "on-demand", 2), [[0]], (False, True), None
    raise KeyError(name)


GENERAL_CASES = ("spread", "anti-affinity", "reservations", "reserved-replacement")
BATCHED_CASES =("config4", "disruption-state", "spot-to-spot", "spot-to-spot-config4", "host-ports", "min-values", "budgets")
_SOLVES = {}


@functools.lru_cache(maxsize=None)
def computed(name, multi_node):
    """reference() of a named case, computed once per process (one oracle Solve per subset)."""
    cl, subs, _, allowed = case(name)
    return reference(cl, subs, multi_node, allowed, solves=_SOLVES.setdefault(name, {}))


# The GPU tests read the expected commands from tests/golden/ (recorded results of computed(); written by
# write_golden()), so that GPU time goes to the device; tests/test_command_ref.py holds every recorded file to
# computed() on the CPU.
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL_CASES = BATCHED_CASES + GENERAL_CASES + ("spread-budgets",)


def _golden_path(name, multi_node):
    return os.path.join(GOLDEN, f"command_{name}_{int(bool(multi_node))}.json.gz")


def write_golden(name, multi_node):
    sims, cmds, _ = computed(name, multi_node)
    doc = {"sims": sims, "commands": [None if c is None else {
        "placement": [int(p) for p in c["placement"]],
        "nodeclaims": [{"nodepool": n["nodepool"], "pods": list(n["pods"]), "options": list(n["options"]),
                        "n_remaining": n["n_remaining"], "requirements": [list(r) for r in n["requirements"]],
                        "requests": n["requests"]} for n in c["nodeclaims"]]} for c in cmds]}
    os.makedirs(GOLDEN, exist_ok=True)
    with gzip.GzipFile(_golden_path(name, multi_node), "wb", mtime=0) as f:
        f.write(json.dumps(doc, sort_keys=True).encode())


@functools.lru_cache(maxsize=None)
def expected(name, multi_node):
    """(sim dicts, commands, None) of a named case as recorded under tests/golden/ (floats round-trip exactly)."""
    with gzip.open(_golden_path(name, multi_node), "rb") as f:
        doc = json.loads(f.read().decode())
    cmds = []
    for c in doc["commands"]:
        if c is not None:
            c["placement"] = np.asarray(c["placement"], dtype=np.int32)
            for n in c["nodeclaims"]:
                n["requirements"] = [(r[0], r[1], list(r[2]), r[3]) for r in n["requirements"]]
        cmds.append(c)
    return doc["sims"], cmds, None
