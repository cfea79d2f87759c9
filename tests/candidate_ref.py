"""Plain-Python reference of candidate selection (the rule of DESIGN 14 / include/kp/kp_abi.h, kp_cluster_candidates):
dict and set label matching, Python ints for the eviction cost, Python floats for the product, and `sorted` with a
comparator that uses `<` on the floats and then the node name's bytes. It shares nothing with kpamd but the model
dataclasses it reads (Cluster, DisruptionControls, PodDisruptionBudget, LabelSelector)."""
import functools

EMPTINESS, SINGLE, MULTI, DRIFT = range(4)
METHODS = (EMPTINESS, SINGLE, MULTI, DRIFT)
(CANDIDATE, NOT_MANAGED, NODE_DO_NOT_DISRUPT, NOT_INITIALIZED, DELETING, NOMINATED, POD_DO_NOT_DISRUPT, PDB_BLOCKED,
 CONSOLIDATION_DISABLED, POLICY_WHEN_EMPTY, NOT_CONSOLIDATABLE, NOT_EMPTY, NOT_DRIFTED) = range(13)
ONE = 1 << 27
POOL_LABEL = "karpenter.sh/nodepool"


def selects(selector, labels):
    """metav1.LabelSelector against a pod's labels: nil selects nothing, empty everything."""
    if selector is None:
        return False
    for k, v in selector.match_labels.items():
        if labels.get(k) != v:
            return False
    for key, op, values in selector.match_expressions:
        if op == "In":
            if key not in labels or labels[key] not in set(values):
                return False
        elif op == "NotIn":
            if key in labels and labels[key] in set(values):
                return False
        elif op == "Exists":
            if key not in labels:
                return False
        elif op == "DoesNotExist":
            if key in labels:
                return False
        else:
            raise ValueError(op)
    return True


def blocking_pdb(pdbs, namespace, labels):
    """The lowest PDB that blocks a pod (its namespace, selecting its labels, no disruption allowed), or None."""
    for i, b in enumerate(pdbs):
        if b.disruptions_allowed == 0 and b.namespace == namespace and selects(b.selector, labels):
            return i
    return None


def eviction_cost_fx(priority, deletion_cost):
    return max(-10 * ONE, min(10 * ONE, ONE + int(deletion_cost) + 4 * int(priority)))


def lifetime_remaining(node, now):
    if node.expire_after is None:
        return 1.0
    if node.expire_after == 0:
        return 0.0
    x = float(node.expire_after - (now - node.created)) / float(node.expire_after)
    return 0.0 if x < 0.0 else 1.0 if x > 1.0 else x


def node_record(cluster, controls, i, method, now):
    """(reason, detail, rescheduling_cost_fx, disruption_cost) of node i."""
    n, c = cluster.nodes[i], controls.nodes[i]
    fx = sum(eviction_cost_fx(controls.pod_priority[p], controls.pod_deletion_cost[p]) for p in n.pods)
    cost = (float(fx) * 2.0 ** -27) * lifetime_remaining(c, now)
    pools = {p.name: k for k, p in enumerate(cluster.nodepools)}
    pool = pools.get(n.node.labels.get(POOL_LABEL))
    pods_pass = method == DRIFT and c.termination_grace_period
    consolidation = method in (EMPTINESS, SINGLE, MULTI)

    def first_dnd():
        return next((int(p) for p in n.pods if controls.pod_do_not_disrupt[p]), None)

    def first_blocked():
        for p in n.pods:
            sh = cluster.shapes[int(cluster.pod_shape[p])]
            b = blocking_pdb(controls.pdbs, sh.namespace, sh.labels)
            if b is not None:
                return b
        return None

    def ladder():
        if pool is None:
            return NOT_MANAGED, 0
        if c.do_not_disrupt:
            return NODE_DO_NOT_DISRUPT, 0
        if not n.node.initialized:
            return NOT_INITIALIZED, 0
        if n.deleting:
            return DELETING, 0
        if c.nominated:
            return NOMINATED, 0
        if not pods_pass:
            p = first_dnd()
            if p is not None:
                return POD_DO_NOT_DISRUPT, p
            b = first_blocked()
            if b is not None:
                return PDB_BLOCKED, b
        pc = controls.pools[pool]
        if consolidation and pc.consolidate_after is None:
            return CONSOLIDATION_DISABLED, 0
        if method in (SINGLE, MULTI) and pc.policy == "WhenEmpty":
            return POLICY_WHEN_EMPTY, 0
        if consolidation and now - c.last_pod_event < pc.consolidate_after:
            return NOT_CONSOLIDATABLE, 0
        if method == EMPTINESS and len(n.pods) > 0:
            return NOT_EMPTY, 0
        if method == DRIFT and c.drifted is None:
            return NOT_DRIFTED, 0
        return CANDIDATE, 0

    reason, detail = ladder()
    return reason, detail, fx, cost


def candidates(cluster, controls, method, now):
    """(records, order): one record per node, and the candidates in disruption order."""
    recs = [node_record(cluster, controls, i, method, now) for i in range(len(cluster.nodes))]

    def compare(a, b):
        ka = controls.nodes[a].drifted if method == DRIFT else recs[a][3]
        kb = controls.nodes[b].drifted if method == DRIFT else recs[b][3]
        if ka < kb:
            return -1
        if kb < ka:
            return 1
        na, nb = cluster.nodes[a].node.name.encode(), cluster.nodes[b].node.name.encode()
        if na != nb:
            return -1 if na < nb else 1
        return (a > b) - (a < b)

    order = sorted((i for i, r in enumerate(recs) if r[0] == CANDIDATE), key=functools.cmp_to_key(compare))
    return recs, order


class RefPlan:
    """plan.candidates(method, now) from the reference, for callers that take a ClusterPlan (disruption.candidates)."""

    def __init__(self, cluster, inner=None):
        self.cluster, self.inner = cluster, inner

    def candidates(self, method, now):
        recs, order = candidates(self.cluster, self.cluster.controls, method, now)
        return recs, order, {}

    def __getattr__(self, name):  # simulate / drift / command: the plan behind it (the oracle's)
        return getattr(self.inner, name)
