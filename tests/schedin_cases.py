"""Hand-written cases of kp_scheduler_inputs, each with its expectation written out by hand - TEST
INFRASTRUCTURE. A case is (SchedulerState, want): want maps a table of schedin_ref.compute() to its expected value
("matrix": node x template, "pool_matrix": NodePool x template). tests/test_schedin.py holds the reference to these
on the CPU, tests/test_gpu_schedin.py the device to the reference."""
from kpamd.model import NodePool, PodShape, SchedNode, SchedulerState

POOL = "karpenter.sh/nodepool"
ZONE = "topology.kubernetes.io/zone"
CPUS = "karpenter.k8s.aws/instance-cpu"
GPU = "nvidia.com/gpu"
NS, PNS = "NoSchedule", "PreferNoSchedule"


def ds(cpu_m, **kw):
    return PodShape({"cpu": cpu_m}, **kw)


def node(name, pool, labels=None, **kw):
    lab = dict(labels or {})
    if pool is not None:
        lab[POOL] = pool
    return SchedNode(name, lab, **kw)


def taints():
    """A taint excludes a template that does not tolerate it; Exists with an empty key tolerates every taint; a
    PreferNoSchedule taint excludes on a node and not on a NodePool's template."""
    pools = [NodePool("a"), NodePool("b", taints=[("dedicated", "x", NS)]), NodePool("c", taints=[("soft", "", PNS)])]
    dss = [ds(100), ds(10, tolerations=[("", "Exists", "", "")]), ds(1, tolerations=[("dedicated", "Equal", "x", NS)])]
    nodes = [node("n0", "a"), node("n1", "b", taints=[("dedicated", "x", NS)]), node("n2", "c", taints=[("soft", "", PNS)])]
    want = {"matrix": [[True, True, True], [False, True, True], [False, True, False]],
            "pool_matrix": [[True, True, True], [False, True, True], [True, True, True]],
            "requests": [{"cpu": 111}, {"cpu": 11}, {"cpu": 10}],
            "daemon_requests": [{"cpu": 111}, {"cpu": 11}, {"cpu": 111}],
            "node_compatible": [3, 2, 1], "pool_compatible": [3, 2, 3],
            "compat": [[0b111], [0b110], [0b010]]}
    return SchedulerState(pools, dss, nodes), want


def selectors():
    """A key the node lacks: excluded under In, kept under NotIn. The same on a well-known key: kept on the template
    (AllowUndefinedWellKnownLabels), excluded on the node."""
    pools = [NodePool("a")]
    dss = [ds(1, node_selector={"team": "x"}), ds(2, required_terms=[[("team", "NotIn", ["x"])]]),
           ds(4, node_selector={ZONE: "z1"})]
    nodes = [node("n0", "a", {"team": "x"}), node("n1", "a"), node("n2", "a", {ZONE: "z1"})]
    want = {"matrix": [[True, False, False], [False, True, False], [False, True, True]],
            "pool_matrix": [[False, True, True]],
            "requests": [{"cpu": 1}, {"cpu": 2}, {"cpu": 6}], "daemon_requests": [{"cpu": 6}]}
    return SchedulerState(pools, dss, nodes), want


def gt_lt():
    """Gt and Lt on a numeric label; a node without the label fails both (Exists with bounds is not a negative
    operator)."""
    pools = [NodePool("a", requirements=[(CPUS, "In", ["4"])])]
    dss = [ds(1, required_terms=[[(CPUS, "Gt", ["8"])]]), ds(2, required_terms=[[(CPUS, "Lt", ["8"])]])]
    nodes = [node("n0", "a", {CPUS: "4"}), node("n1", "a", {CPUS: "16"}), node("n2", "a"), node("n3", "a", {CPUS: "8"})]
    want = {"matrix": [[False, True], [True, False], [False, False], [False, False]], "pool_matrix": [[False, True]],
            "requests": [{"cpu": 2}, {"cpu": 1}, {}, {}], "daemon_requests": [{"cpu": 2}]}
    return SchedulerState(pools, dss, nodes), want


def terms():
    """Two required terms where only the second fits: the template keeps it through the relax loop, the node tests
    the first term alone. A preferred term that would exclude is ignored on both sides. Volume requirements count."""
    pools = [NodePool("a", requirements=[(ZONE, "In", ["z1"])], labels={"team": "x"})]
    dss = [ds(1, required_terms=[[("team", "In", ["y"])], [("team", "In", ["x"])]]),
           ds(2, preferred_terms=[(10, [("team", "In", ["nope"])])]),
           ds(4, volume_requirements=[(ZONE, "In", ["z2"])]),
           ds(8, volume_requirements=[(ZONE, "In", ["z1"])]),
           ds(16, required_terms=[[("team", "In", ["x"])], [("team", "In", ["y"])]],
              volume_requirements=[(ZONE, "In", ["z2"])])]
    nodes = [node("n0", "a", {"team": "x", ZONE: "z1"})]
    want = {"matrix": [[False, True, False, True, False]], "pool_matrix": [[True, True, False, True, False]],
            "requests": [{"cpu": 10}], "daemon_requests": [{"cpu": 11}]}
    return SchedulerState(pools, dss, nodes), want


def arithmetic():
    """The clamp (bound daemonset pods exceed the expectation on cpu and pods, fall short on memory), a resource
    present in a template and absent from allocatable, available going negative, a pool without limits, limits on cpu
    only, the remainder going negative, a node whose pool label names no pool, a node without the label, a node
    without pods."""
    pools = [NodePool("a", limits={"cpu": 10000}), NodePool("b"), NodePool("c", limits={"cpu": 1000, "memory": 5000})]
    dss = [PodShape({"cpu": 100, "memory": 50, "pods": 1000}), PodShape({"cpu": 50, GPU: 1000})]
    nodes = [
        node("n0", "a", allocatable={"cpu": 4000, "memory": 8000, "pods": 10000},
             capacity={"cpu": 4100, "memory": 8100, "pods": 10000},
             pods=[({"cpu": 1000, "memory": 1000, "pods": 1000}, False), ({"cpu": 200, "memory": 20, "pods": 1000}, True)]),
        node("n1", "a", allocatable={"cpu": 1000}, capacity={"cpu": 7000}, pods=[({"cpu": 1500, "memory": 10}, False)]),
        node("n2", "c", allocatable={"cpu": 2000, "memory": 4000}, capacity={"cpu": 2000, "memory": 4000, "pods": 5000}),
        node("n3", "ghost", allocatable={"cpu": 1}, capacity={"cpu": 99999}),
        node("n4", None, allocatable={"cpu": 500}, capacity={"cpu": 500}, pods=[({"cpu": 100}, True)]),
    ]
    full = {"cpu": 150, "memory": 50, "pods": 1000, GPU: 1000}
    want = {"matrix": [[True, True]] * 5, "pool_matrix": [[True, True]] * 3,
            "available": [{"cpu": 2800, "memory": 6980, "pods": 8000}, {"cpu": -500}, {"cpu": 2000, "memory": 4000},
                          {"cpu": 1}, {"cpu": 400}],
            "requests": [{"cpu": 0, "memory": 30, "pods": 0, GPU: 1000}, full, full, full,
                         {"cpu": 50, "memory": 50, "pods": 1000, GPU: 1000}],
            "daemon_requests": [full, full, full],
            "remaining": [{"cpu": -1100}, None, {"cpu": -1000, "memory": 1000}],
            "node_compatible": [2] * 5, "pool_compatible": [2] * 3}
    return SchedulerState(pools, dss, nodes), want


def no_daemonsets():
    """D = 0: no requests anywhere, one zero compatibility word per node; available and remaining as before."""
    st, w = arithmetic()
    st.daemonsets = []
    want = {"matrix": [[]] * 5, "pool_matrix": [[]] * 3, "available": w["available"], "remaining": w["remaining"],
            "requests": [{}] * 5, "daemon_requests": [{}] * 3, "node_compatible": [0] * 5, "pool_compatible": [0] * 3,
            "compat": [[0]] * 5}
    return SchedulerState(st.nodepools, [], st.nodes), want


ALL = (taints, selectors, gt_lt, terms, arithmetic, no_daemonsets)


# ---- the kernels' size edges: states whose expectation comes from the reference, with the part that matters by hand
def template_count(D):
    """D templates of which only the last is compatible with the node: the last lane, or the last word"""
    dss = [ds(1 + d, node_selector={"team": "x" if d == D - 1 else "other"}) for d in range(D)]
    nodes = [node("n0", "a", {"team": "x"}, allocatable={"cpu": 1000}, capacity={"cpu": 1000})]
    want = {"matrix": [[d == D - 1 for d in range(D)]], "requests": [{"cpu": D} if D else {}],
            "node_compatible": [1 if D else 0]}
    return SchedulerState([NodePool("a", labels={"team": "x"})], dss, nodes), want


def node_count(N, n_pools=3):
    """N nodes over n_pools pools (the last pool owns none), labels, taints and pod rows cycling with co-prime periods"""
    pools = [NodePool(f"p{p}", limits={"cpu": 1000 * N} if p % 2 == 0 else {}) for p in range(n_pools)]
    dss = [ds(1, node_selector={"team": "t0"}), ds(2, required_terms=[[("team", "NotIn", ["t1"])]]),
           ds(4, tolerations=[("", "Exists", "", "")]), ds(8, required_terms=[[(CPUS, "Gt", ["3"])]])]
    nodes = []
    for i in range(N):
        labels = {CPUS: str(i % 7)}
        if i % 4:
            labels["team"] = f"t{i % 3}"
        nodes.append(node(f"n{i}", f"p{i % max(1, n_pools - 1)}", labels,
                          taints=[("k", "v", NS)] if i % 5 == 0 else [],
                          allocatable={"cpu": 4000 + i, "pods": 110000}, capacity={"cpu": 4100 + i, "memory": i},
                          pods=[({"cpu": 100 + j, "pods": 1000}, j % 2 == 1) for j in range(i % 4)]))
    return SchedulerState(pools, dss, nodes)


def pod_rows():
    """pod rows of 0, 1, 64, 65 and 300 pods on one snapshot"""
    dss = [PodShape({"cpu": 5000, "memory": 7, "pods": 1000})]
    nodes = [node(f"n{i}", "a", allocatable={"cpu": 100000, "memory": 1000, "pods": 110000}, capacity={"cpu": 100000},
                  pods=[({"cpu": 10 + (j % 9), "memory": j % 2, "pods": 1000}, j % 3 == 0) for j in range(k)])
             for i, k in enumerate((0, 1, 64, 65, 300))]
    want = {"available": [{"cpu": 100000 - sum(10 + (j % 9) for j in range(k)), "memory": 1000 - k // 2,
                           "pods": 110000 - 1000 * k} for k in (0, 1, 64, 65, 300)]}
    return SchedulerState([NodePool("a")], dss, nodes), want


def value_count(V):
    """a label key with V distinct values, one node each; the template admits the last value alone"""
    dss = [ds(3, node_selector={"shard": f"s{V - 1}"}), ds(5, required_terms=[[("shard", "NotIn", [f"s{V - 1}"])]])]
    nodes = [node(f"n{v}", "a", {"shard": f"s{v}"}) for v in range(V)]
    want = {"matrix": [[v == V - 1, v != V - 1] for v in range(V)]}
    return SchedulerState([NodePool("a")], dss, nodes), want


def expectations_rule(np_, d):
    """R:test/pkg/environment/common/expectations.go:1100-1140 GetDaemonSetOverhead, restated: the daemonset counts
    for a NodePool when Taints(template taints).ToleratesPod(pod) and template.Requirements.Compatible(
    NewPodRequirements(pod), AllowUndefinedWellKnownLabels). For a pod with at most one required term and no preferred
    term NewPodRequirements is the node selector plus that term."""
    import schedin_ref as ref
    from oracle import pyoracle
    assert len(d.required_terms) <= 1 and not d.preferred_terms and all(t[2] != PNS for t in np_.taints)
    reqs = [(k, "In", [v]) for k, v in d.node_selector.items()] + (list(d.required_terms[0]) if d.required_terms else [])
    return all(ref.tolerates(d.tolerations, t) for t in np_.taints) and \
        pyoracle.requirements_compatible(ref.template_requirements(np_), reqs, allow_wellknown=True)


def pinned():
    """The pinned subset: NodePools without PreferNoSchedule taints against daemonsets with at most one required term
    and no preferred term or volume; the expected matrix written by hand."""
    pools = [NodePool("a"), NodePool("b", taints=[("dedicated", "x", NS)]),
             NodePool("c", requirements=[(CPUS, "In", ["4"]), (ZONE, "In", ["z1", "z2"])], labels={"team": "x"})]
    dss = [ds(1), ds(2, tolerations=[("", "Exists", "", "")]), ds(4, tolerations=[("dedicated", "Equal", "x", NS)]),
           ds(8, node_selector={"team": "x"}), ds(16, required_terms=[[("team", "NotIn", ["x"])]]),
           ds(32, node_selector={ZONE: "z1"}), ds(64, required_terms=[[(CPUS, "Gt", ["8"])]]),
           ds(128, required_terms=[[(CPUS, "Lt", ["8"])]]), ds(256, node_selector={ZONE: "z3"})]
    want = [[True, True, True, False, True, True, True, True, True],
            [False, True, True, False, False, False, False, False, False],
            [True, True, True, True, False, True, False, True, False]]
    return SchedulerState(pools, dss, []), want
