"""The oracle of a Drift simulation (kp_cluster_drift): pyoracle.solve on the Problem SimulateScheduling builds for one
candidate subset, the construction of oracle/oracle.cpp's kpo_simulate_batch restated in Python:

  queue      the pending pods, the pods of the nodes being deleted (node order), the subset's pods (subset order)
  existing   every node that is neither in the subset nor being deleted, cluster order
  bound pods the pods of those nodes, as (namespace, labels, existing index, required anti-affinity)
  strict reservations (reserved_offering_mode 1), 100 instance types, the NodePools' remaining limits, UIDs passed on

and AllNonPendingPodsScheduled on its result: a non-pending pod in error, or a candidate pod on an uninitialized node,
is unscheduled. first_unscheduled is the first such pod in the Solve's Queue order (cpu desc, memory desc, creation,
UID, input index)."""
import numpy as np

CANDIDATE, DELETING, PENDING = 0, 1, 2
FIELDS = ("feasible", "n_nodeclaims", "n_pods", "n_unscheduled", "first_unscheduled", "blocked")
BLOCKED = {"feasible": 0, "n_nodeclaims": 0, "n_pods": 0, "n_unscheduled": 0, "first_unscheduled": -1, "blocked": 1}


def simulation_problem(cluster, subset):
    """(Problem, kind per queued pod, cluster pod per queued pod, cluster node per existing node)."""
    from kpamd.model import Problem
    sub = set(int(c) for c in subset)
    assert len(sub) == len(subset) and not any(cluster.nodes[c].deleting for c in sub)
    ex_nodes = [i for i, n in enumerate(cluster.nodes) if i not in sub and not n.deleting]
    pods, kind = [], []
    for p in cluster.pending:
        pods.append(int(p)), kind.append(PENDING)
    for n in cluster.nodes:
        if n.deleting:
            for p in n.pods:
                pods.append(int(p)), kind.append(DELETING)
    for c in subset:
        for p in cluster.nodes[int(c)].pods:
            pods.append(int(p)), kind.append(CANDIDATE)
    bound = []
    for e, i in enumerate(ex_nodes):
        for p in cluster.nodes[i].pods:
            sh = cluster.shapes[int(cluster.pod_shape[p])]
            bound.append((sh.namespace, dict(sh.labels or {}), e, list(sh.required_anti_affinity or [])))
    idx = np.asarray(pods, dtype=np.int64)
    uid_str = getattr(cluster, "pod_uid_str", None)
    prob = Problem(cluster.catalogs, cluster.nodepools, cluster.shapes, np.asarray(cluster.pod_shape)[idx].astype(np.uint32),
                   np.asarray(cluster.pod_creation)[idx].astype(np.int64), np.asarray(cluster.pod_uid)[idx].astype(np.uint64),
                   existing=[cluster.nodes[i].node for i in ex_nodes], max_instance_types=100, name="drift-sim",
                   bound_pods=bound, namespaces=getattr(cluster, "namespaces", {}) or {}, reserved_offering_mode=1,
                   pod_uid_str=[uid_str[p] for p in pods] if uid_str is not None else None)
    return prob, kind, pods, ex_nodes


def queue_order(prob):
    """The Solve's Queue order over the Problem's pods: byCPUAndMemoryDescending, then creation, UID, input index."""
    def key(p):
        rq = prob.shapes[int(prob.pod_shape[p])].requests
        uid = prob.pod_uid_str[p] if prob.pod_uid_str is not None else int(prob.pod_uid[p])
        return (-rq.get("cpu", 0), -rq.get("memory", 0), int(prob.pod_creation[p]), uid, p)
    return sorted(range(prob.n_pods), key=key)


def verdict(prob, kind, pods, result):
    """The kp_drift_result fields of one simulation from its Solve result."""
    pl = result["placement"]
    bad = []
    for p in queue_order(prob):
        if kind[p] == PENDING:
            continue
        t = int(pl[p])
        if t == -1 or (kind[p] == CANDIDATE and t <= -2 and not prob.existing[-2 - t].initialized):
            bad.append(p)
    return {"feasible": 0 if bad else 1, "n_nodeclaims": len(result["nodeclaims"]), "n_pods": prob.n_pods,
            "n_unscheduled": len(bad), "first_unscheduled": pods[bad[0]] if bad else -1, "blocked": 0}


def simulate(cluster, subset):
    """(verdict dict, Solve result) of one subset's drift simulation on the oracle."""
    from oracle import pyoracle
    prob, kind, pods, _ = simulation_problem(cluster, subset)
    res = pyoracle.solve(prob)
    return verdict(prob, kind, pods, res), res


def drift(cluster, subsets, allowed=None):
    """What ClusterPlan.drift(subsets, allowed, read_all=True) must return (without stats): every subset simulated on
    the oracle, the budget rule applied as kpamd.disruption.admissible states it."""
    from kpamd import disruption
    adm = [True] * len(subsets)
    if allowed is not None:
        offs = np.zeros(len(subsets) + 1, dtype=np.uint32)
        offs[1:] = np.cumsum([len(s) for s in subsets])
        flat = np.concatenate([np.asarray(s, dtype=np.uint32) for s in subsets] + [np.zeros(0, dtype=np.uint32)])
        adm = list(disruption.admissible(cluster, offs, flat, allowed))
    results, solves = [], []
    for s, ok in zip(subsets, adm):
        if not ok:
            results.append(dict(BLOCKED)), solves.append(None)
            continue
        v, r = simulate(cluster, s)
        results.append(v), solves.append(r)
    first = next((i for i, v in enumerate(results) if v["feasible"]), -1)
    return {"first": first, "replacements": solves[first] if first >= 0 else None, "results": results,
            "blocked": sum(1 for a in adm if not a)}


def nodeclaims(result):
    """What the tests compare of a Solve result's NodeClaims: NodePool, pods in add order, options, remaining count and
    final requirements."""
    return [(n["nodepool"], n["pods"], n["options"], n["n_remaining"], n["requirements"]) for n in result["nodeclaims"]]


class OracleDriftPlan:
    """The oracle behind ClusterPlan's simulate() and drift() (kpamd.disruption.Controller takes either); calls counts
    the plan calls made."""

    def __init__(self, cluster):
        self.cluster = cluster
        self.calls = []

    def simulate(self, subsets, multi_node=True):
        from oracle import pyoracle
        self.calls.append("simulate")
        return pyoracle.simulate_batch(self.cluster, subsets, multi_node=multi_node)

    def drift(self, subsets, allowed=None, cancel=None, read_all=False):
        self.calls.append("drift")
        out = drift(self.cluster, subsets, allowed)
        if not read_all:
            out["results"] = None
        out["stats"] = {}
        return out

    def close(self):
        pass
