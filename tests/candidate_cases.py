"""Inputs of tests/test_candidates.py: clusters with DisruptionControls built for one edge of candidate selection each
(DESIGN 14), every one with the expectation written out by hand from the rule, so that the CPU half of the test
shows the reference lands on the edge the builder claims and the GPU half compares the device with the reference.

Reasons are the kp_candidate_reason values (candidate_ref names them)."""
import math

import numpy as np

import candidate_ref as ref
from kpamd.model import (Cluster, ClusterNode, DisruptionControls, ExistingNode, LabelSelector, NodeControls, NodePool,
                         PodDisruptionBudget, PodShape, PoolControls)

NOW = 1_750_100_000
ONE = 1 << 27
E, S, M, D = ref.METHODS
TILE = 2048  # CAND_TILE of csrc/kp_cand.h: the keys one workgroup sorts in LDS


def tiny_catalog(catalog):
    """Three small on-demand-capable types of the real catalogue: candidate selection reads none of them."""
    out = [it for it in catalog if any(o.available and o.capacity_type == "on-demand" for o in it.offerings)][:3]
    assert len(out) == 3
    return out


class Builder:
    """A cluster node by node. pods: a list of shape indices or (shape, priority, deletion_cost, do_not_disrupt)
    tuples, in the node's `pods` order; reverse=True gives the node's pods descending cluster indices, so that "first
    in pods order" and "lowest pod index" differ."""

    def __init__(self, catalog, shapes, pools=None, pdbs=()):
        self.cat = tiny_catalog(catalog)
        self.shapes = shapes
        self.pools = pools or {"default": PoolControls()}
        self.pdbs = list(pdbs)
        self.nodes, self.ctl, self.names = [], [], {}
        self.pod_shape, self.prio, self.cost, self.dnd = [], [], [], []

    def node(self, name, pods=(), pool="default", initialized=True, deleting=False, reverse=False, **ctl):
        it = self.cat[len(self.nodes) % len(self.cat)]
        labels = {"kubernetes.io/hostname": name, "topology.kubernetes.io/zone": "test-zone-1a",
                  "karpenter.sh/capacity-type": "on-demand", "node.kubernetes.io/instance-type": it.name}
        if pool is not None:
            labels["karpenter.sh/nodepool"] = pool
        first = len(self.pod_shape)
        for p in pods:
            sh, pr, dc, dnd = (p, 0, 0, False) if isinstance(p, int) else p
            self.pod_shape.append(sh), self.prio.append(pr), self.cost.append(dc), self.dnd.append(dnd)
        idx = list(range(first, len(self.pod_shape)))
        if reverse:  # pods[k] of the node is cluster pod idx[-1 - k]: re-file the records to follow
            for arr in (self.pod_shape, self.prio, self.cost, self.dnd):
                arr[first:] = arr[first:][::-1]
            idx = idx[::-1]
        self.names[name] = len(self.nodes)
        self.nodes.append(ClusterNode(ExistingNode(name, labels, {"cpu": 1000, "memory": 1 << 30, "pods": 1000}, {}, [],
                                                   initialized), 0, self.cat.index(it), idx, deleting))
        self.ctl.append(NodeControls(**ctl))
        return idx

    def build(self, name):
        P = len(self.pod_shape)
        pools = [NodePool(n, 0, 0, [("karpenter.sh/capacity-type", "In", ["on-demand"])]) for n in self.pools]
        controls = DisruptionControls(list(self.pools.values()), self.ctl, np.asarray(self.prio, dtype=np.int32),
                                      np.asarray(self.cost, dtype=np.int32), np.asarray(self.dnd, dtype=bool), self.pdbs)
        return Cluster([self.cat], pools, self.nodes, self.shapes, np.asarray(self.pod_shape, dtype=np.uint32),
                       np.full(P, 1_750_000_000, dtype=np.int64), np.arange(P, dtype=np.uint64), name=name,
                       controls=controls)


def shape(labels=None, namespace="default"):
    return PodShape({"cpu": 10, "memory": 1 << 20, "pods": 1000}, labels=dict(labels or {}), namespace=namespace)


# ---- the docs' example (disruption.md:342-349) -----------------------------------------------------------------------
def docs_example(catalog, pdb2_only=False):
    """Pods A, B, C; PDB-1 (maxUnavailable 0) and PDB-2 (maxUnavailable 1) select A, PDB-3 (minAvailable 100%) selects
    B. PDB_BLOCKED with detail PDB-1 (index 0). pdb2_only: the node holds A alone and PDB-1 is gone - the
    maxUnavailable-style disruptions_allowed 1 does not block."""
    shapes = [shape({"app": "a"}), shape({"app": "b"}), shape({"app": "c"})]
    pdbs = [PodDisruptionBudget("default", "PDB-1", LabelSelector({"app": "a"}), 0),
            PodDisruptionBudget("default", "PDB-2", LabelSelector({"app": "a"}), 1),
            PodDisruptionBudget("default", "PDB-3", LabelSelector({"app": "b"}), 0)]
    b = Builder(catalog, shapes, pdbs=pdbs[1:2] if pdb2_only else pdbs)
    b.node("docs", [0] if pdb2_only else [0, 1, 2])
    want = {"docs": (ref.CANDIDATE, 0) if pdb2_only else (ref.PDB_BLOCKED, 0)}
    return b.build("docs-example"), want


# ---- pods per node at the chunk edges, costs, lifetime, the ladder: one cluster ---------------------------------------
PLAIN, WEB, WEB_OTHER_NS, DB, API, SPECIAL, SPECIAL_TIER, ISO = range(8)
EDGE_SHAPES = [({}, "default"), ({"app": "web"}, "default"), ({"app": "web"}, "other"), ({"app": "db", "tier": "x"}, "default"),
               ({"app": "api"}, "default"), ({"app": "cache", "kind": "special"}, "default"),
               ({"app": "cache", "kind": "special", "tier": "gold"}, "default"), ({}, "iso")]


def edge_pdbs():
    return [
        PodDisruptionBudget("default", "nil", None, 0),                                        # 0 selects nothing
        PodDisruptionBudget("default", "db-allows", LabelSelector({"app": "db"}), 1),          # 1 allows
        PodDisruptionBudget("default", "api-allows", LabelSelector({"app": "api"}), 3),        # 2 allows
        PodDisruptionBudget("default", "web", LabelSelector({"app": "web"}), 0),               # 3 blocks WEB only
        PodDisruptionBudget("default", "api-blocks", LabelSelector({"app": "api"}), 0),        # 4 blocks API (2 allows it)
        PodDisruptionBudget("default", "special", LabelSelector({"kind": "special"}, [("app", "NotIn", ["web"]),
                                                                                       ("tier", "DoesNotExist", [])]), 0),  # 5
        PodDisruptionBudget("elsewhere", "empty-elsewhere", LabelSelector(), 0),               # 6 a namespace without pods
        PodDisruptionBudget("iso", "empty-iso", LabelSelector(), 0),                           # 7 every pod of "iso"
    ]


def edges(catalog):
    """(cluster, want): want[node name][method] = (reason, detail), and want_cost[node name] = (sum fx, cost)."""
    pools = {"default": PoolControls(), "never": PoolControls(consolidate_after=None),
             "whenempty": PoolControls("WhenEmpty", 0), "slow": PoolControls(consolidate_after=3600)}
    b = Builder(catalog, [shape(l, ns) for l, ns in EDGE_SHAPES], pools, edge_pdbs())
    want, cost = {}, {}
    C0 = (ref.CANDIDATE, 0)

    def plain(n_pods, drifted=False):
        """A node nothing stops: a consolidation candidate, an Emptiness candidate only when empty, Drift's only when
        drifted."""
        return {E: C0 if n_pods == 0 else (ref.NOT_EMPTY, 0), S: C0, M: C0, D: C0 if drifted else (ref.NOT_DRIFTED, 0)}

    def every(r, d=0):
        return {m: (r, d) for m in ref.METHODS}

    # 0, 1, 63, 64, 65, 128 and 129 pods: the lanes' last chunk empty, one short, full, one over
    for k in (0, 1, 63, 64, 65, 128, 129):
        b.node(f"n-{k}", [PLAIN] * k)
        want[f"n-{k}"], cost[f"n-{k}"] = plain(k), (k * ONE, float(k))
    # the first blocking pod at position 0, 63, 64 and last: the PDB-blocked WEB pod, then a do-not-disrupt pod
    for tag, size, pos in (("0", 65, 0), ("63", 65, 63), ("64", 65, 64), ("last", 129, 128)):
        pods = [PLAIN] * size
        pods[pos] = WEB
        b.node(f"blk-{tag}", pods)
        want[f"blk-{tag}"] = every(ref.PDB_BLOCKED, 3)
        pods = [PLAIN] * size
        pods[pos] = (PLAIN, 0, 0, True)
        idx = b.node(f"dnd-{tag}", pods)
        want[f"dnd-{tag}"] = every(ref.POD_DO_NOT_DISRUPT, idx[pos])
    # a do-not-disrupt pod behind an earlier PDB-blocked pod: every pod is checked for the annotation first
    pods = [PLAIN] * 70
    pods[2], pods[66] = WEB, (PLAIN, 0, 0, True)
    idx = b.node("both", pods)
    want["both"] = every(ref.POD_DO_NOT_DISRUPT, idx[66])
    # two blocked pods and two do-not-disrupt pods, the node's pods listed against their cluster indices: the first in
    # `pods` order decides, which here is the one with the HIGHER pod index
    pods = [PLAIN] * 8
    pods[3], pods[5] = WEB, API
    b.node("two-blocked", pods, reverse=True)
    want["two-blocked"] = every(ref.PDB_BLOCKED, 3)
    pods = [PLAIN] * 8
    pods[1] = pods[6] = (PLAIN, 0, 0, True)
    idx = b.node("two-dnd", pods, reverse=True)
    want["two-dnd"] = every(ref.POD_DO_NOT_DISRUPT, idx[1])
    assert idx[1] > idx[6]
    # PDB forms: the same selector in another namespace, an allowing PDB alone, one allowing and one blocking, NotIn and
    # DoesNotExist, the empty selector
    for name, sh, w in (("web-other-ns", WEB_OTHER_NS, None), ("db-allowed", DB, None), ("api-mixed", API, 4),
                        ("special", SPECIAL, 5), ("special-tier", SPECIAL_TIER, None), ("iso", ISO, 7)):
        b.node(name, [PLAIN, sh])
        want[name] = plain(2) if w is None else every(ref.PDB_BLOCKED, w)
    # eviction cost: the clamp at both ends from the priority and from the deletion cost, and sums
    for name, pods, fx in (("prio-hi", [(PLAIN, 1_000_000_000, 0, False)], 10 * ONE),
                           ("prio-lo", [(PLAIN, -2**31, 0, False)], -10 * ONE),
                           ("dc-hi", [(PLAIN, 0, 2_147_483_647, False)], 10 * ONE),
                           ("dc-lo", [(PLAIN, 0, -2_147_483_647, False)], -10 * ONE),
                           ("unclamped", [(PLAIN, 100, 1000, False)], ONE + 1400),
                           ("all-hi-129", [(PLAIN, 1_000_000_000, 0, False)] * 129, 1290 * ONE),
                           ("neg-sum", [(PLAIN, -2**31, 0, False)] * 2 + [PLAIN], -19 * ONE)):
        b.node(name, pods)
        want[name], cost[name] = plain(len(pods)), (fx, fx / ONE)
    cost["unclamped"] = (ONE + 1400, 1.0 + 1400 / ONE)
    # lifetime: Never, age 0, age == and > expireAfter, created in the future (clamps to 1), expireAfter 0
    for name, ctl, life in (("never", {}, 1.0), ("age0", dict(created=NOW, expire_after=1000), 1.0),
                            ("age-half", dict(created=NOW - 500, expire_after=1000), 0.5),
                            ("age-eq", dict(created=NOW - 1000, expire_after=1000), 0.0),
                            ("age-over", dict(created=NOW - 5000, expire_after=1000), 0.0),
                            ("future", dict(created=NOW + 500, expire_after=1000), 1.0),
                            ("expire0", dict(created=NOW, expire_after=0), 0.0)):
        b.node(name, [PLAIN] * 3, **ctl)
        want[name], cost[name] = plain(3), (3 * ONE, 3.0 * life)
    # two products one ulp apart, the smaller under the later name
    b.node("ulp-b", [PLAIN], created=NOW - (2**53 - (2**52 + 1)), expire_after=2**53)   # 0.5 + 2^-53
    b.node("ulp-a", [PLAIN], created=NOW - (2**52 - (2**51 + 1)), expire_after=2**52)   # 0.5 + 2^-52
    want["ulp-a"] = want["ulp-b"] = plain(1)
    cost["ulp-b"], cost["ulp-a"] = (ONE, 0.5 + 2.0**-53), (ONE, math.nextafter(0.5 + 2.0**-53, math.inf))
    # -0.0 (a negative sum at lifetime 0) between two empty nodes at +0.0: the names decide, in both directions
    b.node("nz-a"), b.node("nz-c")
    b.node("nz-b", [(PLAIN, -2**31, 0, False)], created=NOW - 5000, expire_after=1000)
    want["nz-a"], want["nz-c"], want["nz-b"] = plain(0), plain(0), plain(1)
    cost["nz-b"] = (-10 * ONE, -0.0)
    # the ladder: one node per reason, nodes under several reasons, terminationGracePeriod under Drift
    b.node("r1-nolabel", [PLAIN], pool=None), b.node("r1-unknown", [PLAIN], pool="gone")
    want["r1-nolabel"] = want["r1-unknown"] = every(ref.NOT_MANAGED)
    b.node("r2", [PLAIN], do_not_disrupt=True), b.node("r3", [PLAIN], initialized=False)
    b.node("r4", [PLAIN], deleting=True), b.node("r5", [PLAIN], nominated=True)
    want["r2"], want["r3"] = every(ref.NODE_DO_NOT_DISRUPT), every(ref.NOT_INITIALIZED)
    want["r4"], want["r5"] = every(ref.DELETING), every(ref.NOMINATED)
    b.node("r8", [PLAIN], pool="never", drifted=NOW - 70)
    want["r8"] = {E: (ref.CONSOLIDATION_DISABLED, 0), S: (ref.CONSOLIDATION_DISABLED, 0), M: (ref.CONSOLIDATION_DISABLED, 0), D: C0}
    b.node("r9", [PLAIN], pool="whenempty"), b.node("r9-empty", [], pool="whenempty")
    want["r9"] = {E: (ref.NOT_EMPTY, 0), S: (ref.POLICY_WHEN_EMPTY, 0), M: (ref.POLICY_WHEN_EMPTY, 0), D: (ref.NOT_DRIFTED, 0)}
    want["r9-empty"] = {E: C0, S: (ref.POLICY_WHEN_EMPTY, 0), M: (ref.POLICY_WHEN_EMPTY, 0), D: (ref.NOT_DRIFTED, 0)}
    b.node("r10", [PLAIN], pool="slow", last_pod_event=NOW - 3599)
    b.node("r10-edge", [PLAIN], pool="slow", last_pod_event=NOW - 3600)  # now - event == consolidateAfter: consolidatable
    want["r10"] = {E: (ref.NOT_CONSOLIDATABLE, 0), S: (ref.NOT_CONSOLIDATABLE, 0), M: (ref.NOT_CONSOLIDATABLE, 0),
                   D: (ref.NOT_DRIFTED, 0)}
    want["r10-edge"] = plain(1)
    b.node("several-1", [(PLAIN, 0, 0, True)], pool=None, initialized=False, deleting=True, do_not_disrupt=True, nominated=True)
    b.node("several-2", [WEB], initialized=False, do_not_disrupt=True)
    b.node("several-5", [WEB, (PLAIN, 0, 0, True)], nominated=True)
    b.node("several-8", [PLAIN], pool="never", last_pod_event=NOW)
    want["several-1"], want["several-2"], want["several-5"] = every(ref.NOT_MANAGED), every(ref.NODE_DO_NOT_DISRUPT), every(ref.NOMINATED)
    want["several-8"] = {E: (ref.CONSOLIDATION_DISABLED, 0), S: (ref.CONSOLIDATION_DISABLED, 0), M: (ref.CONSOLIDATION_DISABLED, 0),
                         D: (ref.NOT_DRIFTED, 0)}
    b.node("tgp-blocked", [PLAIN, WEB], termination_grace_period=True, drifted=NOW - 50)
    idx = b.node("tgp-dnd", [PLAIN, (PLAIN, 0, 0, True)], termination_grace_period=True, drifted=NOW - 50)
    b.node("notgp-blocked", [PLAIN, WEB], drifted=NOW - 50)
    want["tgp-blocked"] = {E: (ref.PDB_BLOCKED, 3), S: (ref.PDB_BLOCKED, 3), M: (ref.PDB_BLOCKED, 3), D: C0}
    want["tgp-dnd"] = {m: (ref.POD_DO_NOT_DISRUPT, idx[1]) for m in (E, S, M)}
    want["tgp-dnd"][D] = C0
    want["notgp-blocked"] = every(ref.PDB_BLOCKED, 3)
    # Drift: ordered by the transition time, ties by name
    for name, t in (("d-1", NOW - 50), ("d-3", NOW - 100), ("d-2", NOW - 100), ("d-0", NOW - 50), ("d-neg", -5)):
        b.node(name, [PLAIN], drifted=t)
        want[name] = plain(1, drifted=True)
    return b.build("candidate-edges"), want, cost


# what the edges cluster's order must contain, by hand: Drift's whole list, and the consolidation order around zero
EDGES_DRIFT_ORDER = ["d-neg", "d-2", "d-3", "r8", "d-0", "d-1", "tgp-blocked", "tgp-dnd"]
EDGES_SINGLE_HEAD = ["neg-sum", "dc-lo", "prio-lo"]                                  # -19, -10, -10 (names)
EDGES_SINGLE_ZEROS = ["age-eq", "age-over", "expire0", "n-0", "nz-a", "nz-b", "nz-c"]  # +0.0 and -0.0 tie: names
EDGES_SINGLE_ULP = ["ulp-b", "ulp-a"]                                                # cost, against the names


# ---- the order: many candidates, names in an order of their own --------------------------------------------------------
ORDER_NODES = 4200  # past two LDS tiles: the sort pads to 8,192 keys, three merge stages in global memory


def order_name(i):
    """Names whose byte order is neither the index order nor the numeric order ("n10" < "n9")."""
    return f"n{(i * 7919) % 10007}"


def order_cluster(catalog):
    """ORDER_NODES nodes of 0..3 plain pods (node i: i % 4), every one a candidate when nothing is set."""
    b = Builder(catalog, [shape()])
    for i in range(ORDER_NODES):
        b.node(order_name(i), [0] * (i % 4))
    return b.build("candidate-order")


def order_controls(cluster, k):
    """The cluster's controls with every node but k of them marked do-not-disrupt: k candidates. The k are spread over
    the index range (every node i with i * k // N stepping), so that candidates and non-candidates interleave."""
    N = len(cluster.nodes)
    keep = {(j * N) // k for j in range(k)}
    assert len(keep) == k
    c = cluster.controls
    return DisruptionControls(c.pools, [NodeControls(do_not_disrupt=i not in keep) for i in range(N)], c.pod_priority,
                              c.pod_deletion_cost, c.pod_do_not_disrupt, c.pdbs), sorted(keep)


ORDER_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000, TILE - 1, TILE, TILE + 1, ORDER_NODES)


def equal_costs(catalog):
    """257 empty nodes: every cost +0.0, the name decides everything."""
    b = Builder(catalog, [shape()])
    for i in range(257):
        b.node(order_name(i))
    return b.build("candidate-equal-costs")


# ---- PDB counts ---------------------------------------------------------------------------------------------------------
def pdb_cluster(catalog):
    """Eight nodes, node j holding two pods labelled app-j."""
    b = Builder(catalog, [shape({"app": f"app-{j}"}) for j in range(8)])
    for j in range(8):
        b.node(f"p-{j}", [j, j])
    return b.build("candidate-pdbs")


def pdb_controls(cluster, n, blocking):
    """n PDBs, PDB i selecting app-(i % 8); the ones in `blocking` allow no disruption, the others one."""
    c = cluster.controls
    pdbs = [PodDisruptionBudget("default", f"pdb-{i}", LabelSelector({"app": f"app-{i % 8}"}), 0 if i in blocking else 1)
            for i in range(n)]
    return DisruptionControls(c.pools, c.nodes, c.pod_priority, c.pod_deletion_cost, c.pod_do_not_disrupt, pdbs)


# (PDB count, blocking PDBs, {node: PDB}) - the last PDB alone (lane 0 / 63 / 0 of the second round / 63 of the last),
# and two blocking PDBs of one shape found by different lanes: the lower wins
PDB_CASES = [(0, (), {}), (1, (0,), {0: 0}), (64, (63,), {7: 63}), (65, (64,), {0: 64}), (1024, (1023,), {7: 1023}),
             (1024, (64, 1), {0: 64, 1: 1}), (1024, (1016, 72, 8), {0: 8}), (200, (), {})]


# ---- the controller -----------------------------------------------------------------------------------------------------
def controller_cluster(catalog):
    """Twelve config-4 nodes. The node with the fewest pods is PDB-blocked (its first pod's shape is labelled and a PDB
    on that label allows nothing) and the next carries a high-priority pod, so the disruption order differs from the
    pod-count order at its head. Returns (cluster, fewest, next)."""
    from kpamd import synth
    cl = synth.config4(catalog, n_nodes=12, seed=11, loose=0.5, loose_fill=(0.2, 0.5), topup=False)
    by_count = sorted(range(12), key=lambda i: (len(cl.nodes[i].pods), cl.nodes[i].node.name))
    fewest, nxt = by_count[0], by_count[1]
    assert cl.nodes[fewest].pods and cl.nodes[nxt].pods
    # a shape of its own for the blocked pod (a copy of the one it has), labelled for the PDB
    import copy
    p0 = cl.nodes[fewest].pods[0]
    sh = copy.deepcopy(cl.shapes[int(cl.pod_shape[p0])])
    sh.labels = {"app": "inflate"}
    cl.shapes.append(sh)
    cl.pod_shape[p0] = len(cl.shapes) - 1
    controls = DisruptionControls.default(cl)
    controls.pdbs = [PodDisruptionBudget("default", "inflate-pdb", LabelSelector({"app": "inflate"}), 0)]
    controls.pod_priority[cl.nodes[nxt].pods[0]] = 1_000_000_000
    cl.controls = controls
    return cl, fewest, nxt
