"""Requirement classes: shape-levels whose compiled requirements are equal share the merged tag. Once one
member of a class is merged into a NodeClaim, NodeClaim.Add of every other member there is Fits alone
(Requirement.Intersection is idempotent), so the device tags the whole class merged on that NodeClaim; a permanent
failure of Compatible fails the whole class there; a Fits failure and the undefined-key rule stay the level's own.
A wrong tag changes placements silently, so every case is a crafted queue held to the one-pod-at-a-time oracle
under the default overrides and with kp_overrides.fast_lane forced to 1, 2 and 3.

Every case is a builder, a CPU-only `_inputs` test that proves from the oracle's result alone that the queue contains
the situation (the count it asserts is stated with the case), and a gpu test that re-asserts it. No number asserted
here comes from the device."""
import numpy as np
import pytest

from test_run_length_edges import EPH, MI_M, _problem, _queue, _requests, _shape
from test_run_length_mixed import ARCH, M5, ZONE

K = "karpenter.k8s.aws/"
LINUX = [("kubernetes.io/os", "In", ["linux"])]
SIZES = [(1000, 2048), (500, 1024), (250, 512)]  # three request rows, queue order (cpu descending)


_CASES = {}


def _case(catalog, builder):
    """(problem, oracle result) of a builder, computed once for the CPU-only test and the gpu tests."""
    from oracle import pyoracle
    if builder.__name__ not in _CASES:
        prob = builder(catalog)
        _CASES[builder.__name__] = (prob, pyoracle.solve(prob))
    return _CASES[builder.__name__]


def _pool8(name="m5", weight=0, extra=()):
    """m5.2xlarge on-demand only: NodeClaims of 8 vCPU, so a few hundred pods make many of them."""
    from kpamd.model import NodePool
    return NodePool(name, weight, 0, list(M5) + [(K + "instance-cpu", "In", ["8"])] + list(extra))


def _zone(i):
    from kpamd.catalog import ZONES
    return {ZONE: ZONES[i]}


def _row(shape, level0=True):
    """The shape's requirement row (nodeSelector, required terms; at level 0 the preferred terms as well)."""
    terms = tuple(tuple((r[0], r[1], tuple(r[2])) for r in t) for t in shape.required_terms)
    pref = tuple(tuple((r[0], r[1], tuple(r[2])) for r in t) for _, t in shape.preferred_terms) if level0 else ()
    return (tuple(sorted(shape.node_selector.items())), terms, pref)


def _replay(prob, want):
    """The oracle's placement in queue order (every pod placed on its first pop): per pod (queue index, pod,
    NodeClaim, shape, creates the NodeClaim, first meeting of its shape with it, its row already on the NodeClaim)."""
    assert int(want["stats"]["pops"]) == prob.n_pods and bool((want["placement"] >= 0).all())
    rows = [_row(s) for s in prob.shapes]
    seen, on_nc, out = set(), {}, []
    for i, p in enumerate(int(x) for x in _queue(prob)):
        nc, s = int(want["placement"][p]), int(prob.pod_shape[p])
        out.append((i, p, nc, s, nc not in on_nc, (nc, s) not in seen, rows[s] in on_nc.get(nc, ())))
        seen.add((nc, s))
        on_nc.setdefault(nc, set()).add(rows[s])
    return out


def _redundant(prob, want):
    """First meetings (creations aside) that bring a requirement row the NodeClaim already carries."""
    return sum(1 for _, _, _, _, creates, first, there in _replay(prob, want) if first and not creates and there)


def _redundant_on_nodeclaims(prob, want):
    """_redundant for a Solve that leaves pods unplaced or puts some on existing nodes: the pods on NodeClaims, in
    queue order (no pod of these cases is relaxed)."""
    rows = [_row(s) for s in prob.shapes]
    seen, on_nc, n = set(), {}, 0
    for p in (int(x) for x in _queue(prob)):
        nc, s = int(want["placement"][p]), int(prob.pod_shape[p])
        if nc < 0:
            continue
        if (nc, s) not in seen and nc in on_nc and rows[s] in on_nc[nc]:
            n += 1
        seen.add((nc, s))
        on_nc.setdefault(nc, set()).add(rows[s])
    return n


def _shapes_on(prob, want):
    """Per NodeClaim: the set of shapes placed on it."""
    on = {}
    for p, nc in enumerate(want["placement"]):
        if nc >= 0:
            on.setdefault(int(nc), set()).add(int(prob.pod_shape[p]))
    return on


def _variants(ctx, ov, prob, want, **ov_kw):
    """Device == oracle (placements, NodeClaims, their summed requests) under the default overrides and with the
    fast lane forced plain (1), with the continuation round (2) and with the run-length commit alone (3)."""
    import kpamd
    from test_gpu_parity import check_same
    for v in (0, 1, 2, 3):
        ov(fast_lane=v, **ov_kw)
        got = kpamd.Scheduler(ctx, prob).solve()
        print(prob.name, "fast_lane", v, "attempts", got["stats"]["attempts"], "run_length_pods",
              got["stats"]["run_length_pods"], "nodeclaims", len(got["nodeclaims"]))
        check_same(got, want)
        assert _requests(got) == _requests(want), f"fast_lane {v}: NodeClaim requests differ"


def _interleave(groups, n_each):
    """Per group (shapes of one request row, in queue order) n_each pods, the group's shapes in turn."""
    return [g[i % len(g)] for g in groups for i in range(n_each)]


# ---- 1. equal requirements, different requests ------------------------------------------------------------------
def build_equal_requirements(catalog):
    """Two requirement rows x three request rows, the rows interleaved within each request row. The smaller pods
    fill what the larger left on every NodeClaim, so their shapes meet NodeClaims that carry their row already."""
    shapes = [_shape(c, m, required_terms=[list(r)]) for c, m in SIZES for r in (ARCH, LINUX)]
    order = _interleave([(0, 1), (2, 3), (4, 5)], 120)
    return _problem([catalog], [_pool8()], shapes, order, "rqc-equal")


def _pre_equal_requirements(prob, want):
    assert len({_row(s) for s in prob.shapes}) == 2 and len({tuple(s.requests.items()) for s in prob.shapes}) == 3
    n = _redundant(prob, want)
    assert n >= 10, n  # stated with the case: at least 10 first meetings bring a row already on the NodeClaim
    return n


def test_equal_requirements_inputs(catalog):
    _pre_equal_requirements(*_case(catalog, build_equal_requirements))


@pytest.mark.gpu
def test_equal_requirements(ctx, catalog, ov):
    prob, want = _case(catalog, build_equal_requirements)
    print(prob.name, "redundant first meetings", _pre_equal_requirements(prob, want))
    _variants(ctx, ov, prob, want)


# ---- 2. the empty requirement set ------------------------------------------------------------------------------
def build_empty_set(catalog):
    """Zone-selector shapes (two zones) create NodeClaims pinned to their zone; shapes without requirements (three
    request rows) fill them: tagged at the NodeClaim's creation, whatever created it."""
    shapes = [_shape(1000, 2048, node_selector=_zone(0)), _shape(1000, 2048, node_selector=_zone(1)),
              _shape(1000, 2048), _shape(500, 1024), _shape(250, 512)]
    order = _interleave([(0, 1, 2)], 60) + [3] * 60 + [4] * 120
    return _problem([catalog], [_pool8()], shapes, order, "rqc-empty")


def _pre_empty_set(prob, want):
    on = _shapes_on(prob, want)
    free = {2, 3, 4}
    a = sum(1 for s in on.values() if 0 in s and s & free)
    b = sum(1 for s in on.values() if 1 in s and s & free)
    assert not any(0 in s and 1 in s for s in on.values())  # pinned: no NodeClaim holds both zones
    assert a >= 2 and b >= 2, (a, b)  # stated with the case: requirement-free pods on >= 2 NodeClaims of each zone
    return a, b


def test_empty_set_inputs(catalog):
    _pre_empty_set(*_case(catalog, build_empty_set))


@pytest.mark.gpu
def test_empty_set(ctx, catalog, ov):
    prob, want = _case(catalog, build_empty_set)
    print(prob.name, "zone NodeClaims with requirement-free pods", _pre_empty_set(prob, want))
    _variants(ctx, ov, prob, want)


# ---- 3. a class-wide NC_NEVER stays inside the class -----------------------------------------------------------
def build_never_in_class(catalog):
    """Zone-b pods (the largest) create NodeClaims first; zone-a shapes of three request rows meet them and fail
    Compatible for good, as a class. A shape of another class with the smallest zone-a request row still lands on
    the zone-b NodeClaims."""
    shapes = [_shape(2000, 4096, node_selector=_zone(1))] + \
             [_shape(c, m, node_selector=_zone(0)) for c, m in SIZES] + [_shape(250, 512, required_terms=[list(ARCH)])]
    order = [0] * 14 + [1] * 10 + [2] * 20 + _interleave([(3, 4)], 160)
    return _problem([catalog], [_pool8()], shapes, order, "rqc-never")


def _pre_never_in_class(prob, want):
    on = _shapes_on(prob, want)
    zb = [nc for nc, s in on.items() if 0 in s]
    assert len(zb) >= 3 and not any(on[nc] & {1, 2, 3} for nc in zb)  # zone-a pods never join a zone-b NodeClaim
    ev = _replay(prob, want)
    born = {nc: i for i, _, nc, _, creates, _, _ in ev if creates}
    met = {s for i, _, _, s, _, _, _ in ev if s in (1, 2, 3) and any(born[nc] < i for nc in zb)}
    assert met == {1, 2, 3}  # every zone-a shape is placed while zone-b NodeClaims exist (it scanned them)
    other = sum(1 for nc in zb if 4 in on[nc])
    assert other >= 3, other  # stated with the case: the other class lands on >= 3 zone-b NodeClaims
    assert dict(prob.shapes[4].requests) == dict(prob.shapes[3].requests)
    return other


def test_never_in_class_inputs(catalog):
    _pre_never_in_class(*_case(catalog, build_never_in_class))


@pytest.mark.gpu
def test_never_in_class(ctx, catalog, ov):
    prob, want = _case(catalog, build_never_in_class)
    print(prob.name, "zone-b NodeClaims with the other class", _pre_never_in_class(prob, want))
    _variants(ctx, ov, prob, want)


# ---- 4. Fits failures stay per level ---------------------------------------------------------------------------
def build_fits_per_level(catalog):
    """One class, three shapes: a large one (cpu and memory as the others, plus ephemeral storage: the queue keeps
    the input order) and two small ones. The large shape fills NodeClaim X's storage and moves on to a new NodeClaim
    (a Fits failure on X: NC_NEVER for its level alone). Then the second small shape meets X for the first time and
    is merged there: the class is tagged on X, and the large shape must stay failed on X. A shape of another class
    is merged into X as well."""
    big = {EPH: 4096 * MI_M}
    shapes = [_shape(extra=big, required_terms=[list(LINUX)]), _shape(required_terms=[list(LINUX)]),
              _shape(required_terms=[list(LINUX)], labels={"app": "second"}), _shape(required_terms=[list(ARCH)])]
    order = [0] * 6 + [1] * 3 + [2] * 12 + [3] * 4 + [0] * 6 + [1] * 10 + [2] * 10 + [0] * 4
    return _problem([catalog], [_pool8()], shapes, order, "rqc-fits")


def _pre_fits_per_level(prob, want):
    assert _row(prob.shapes[0]) == _row(prob.shapes[1]) == _row(prob.shapes[2]) != _row(prob.shapes[3])
    ev = _replay(prob, want)
    x = ev[0][2]
    assert ev[0][3] == 0 and ev[0][4]  # X: the first NodeClaim, created by the large shape
    # the large shape creates another NodeClaim: it failed on every NodeClaim there was, X included
    t1 = next(i for i, _, nc, s, creates, _, _ in ev if s == 0 and creates and nc != x)
    # after that the second small shape meets X for the first time (a merge of a member of the large shape's class)
    t2 = next(i for i, _, nc, s, creates, first, _ in ev if i > t1 and s == 2 and nc == x and first and not creates)
    assert any(i > t1 and s == 3 and nc == x and first for i, _, nc, s, _, first, _ in ev)  # the other class on X too
    assert any(i > t2 and s == 1 and nc == x for i, _, nc, s, _, _, _ in ev)  # the small shape keeps appending to X
    later = [nc for i, _, nc, s, _, _, _ in ev if i > t2 and s == 0]
    assert len(later) >= 8 and x not in later, later  # stated with the case: >= 8 large pods afterwards, none on X
    return len(later)


def test_fits_per_level_inputs(catalog):
    _pre_fits_per_level(*_case(catalog, build_fits_per_level))


@pytest.mark.gpu
def test_fits_per_level(ctx, catalog, ov):
    prob, want = _case(catalog, build_fits_per_level)
    print(prob.name, "large pods after the class tag, none on X:", _pre_fits_per_level(prob, want))
    _variants(ctx, ov, prob, want)


# ---- 5. the undefined-key rule ---------------------------------------------------------------------------------
def build_undefined_key(catalog):
    """Two shapes share the row `team Exists` (a custom key). The heavier pool does not define the key, so they fail
    on its NodeClaim A by Compatible's undefined-key rule (not for good) and open NodeClaim B in the pool that defines
    it. A third shape's `team NotIn` is merged into A and defines the key there: the pair's next pods land on A."""
    pools = [_pool8("plain", 10), _pool8("teams", 1, [("team", "In", ["a", "b"])])]
    pair = [[("team", "Exists", [])]]
    shapes = [_shape(), _shape(required_terms=pair), _shape(required_terms=pair, labels={"app": "second"}),
              _shape(required_terms=[[("team", "NotIn", ["x"])]])]
    order = [0] * 2 + [1, 2] * 3 + [3] + [1, 2] * 5 + [0] * 4
    return _problem([catalog], pools, shapes, order, "rqc-undefined-key")


def _pre_undefined_key(prob, want):
    ev = _replay(prob, want)
    a = ev[0][2]
    assert ev[0][3] == 0 and ev[0][4] and want["nodeclaims"][a]["nodepool"] == 0
    t_def = next(i for i, _, nc, s, _, _, _ in ev if s == 3)
    assert ev[t_def][2] == a  # the third shape is merged into A
    before = [(s, nc) for i, _, nc, s, _, _, _ in ev if s in (1, 2) and i < t_def]
    assert len(before) >= 2 and all(nc != a for _, nc in before)  # the pair failed on A before the key was defined
    after = {s for i, _, nc, s, _, _, _ in ev if s in (1, 2) and i > t_def and nc == a}
    assert after == {1, 2}, after  # stated with the case: both shapes of the pair land on A afterwards
    return len(before)


def test_undefined_key_inputs(catalog):
    _pre_undefined_key(*_case(catalog, build_undefined_key))


@pytest.mark.gpu
def test_undefined_key(ctx, catalog, ov):
    prob, want = _case(catalog, build_undefined_key)
    print(prob.name, "pods of the pair that failed on A first:", _pre_undefined_key(prob, want))
    _variants(ctx, ov, prob, want)


# ---- 6. relaxation levels --------------------------------------------------------------------------------------
def build_relaxation(catalog):
    """Shapes 0 and 1 prefer a family the pool does not have: level 0 fails everywhere, the pod is relaxed and queued
    again, and its relaxed level carries exactly shape 2's requirements, so one class spans levels of different
    shapes. Shape 2's pods (3 vCPU, two to a NodeClaim) leave room on every NodeClaim for the relaxed pods behind."""
    pref = [(1, [(K + "instance-family", "In", ["c5"])])]
    shapes = [_shape(500, 1024, required_terms=[list(ARCH)], preferred_terms=pref),
              _shape(250, 512, required_terms=[list(ARCH)], preferred_terms=pref),
              _shape(3000, 4096, required_terms=[list(ARCH)]), _shape(250, 512, required_terms=[list(LINUX)])]
    order = [2] * 20 + [0] * 30 + _interleave([(1, 3)], 60)
    return _problem([catalog], [_pool8()], shapes, order, "rqc-relax")


def _pre_relaxation(prob, want):
    assert bool((want["placement"] >= 0).all()) and int(want["stats"]["pops"]) > prob.n_pods  # relaxed pods pop twice
    assert _row(prob.shapes[0], level0=False) == _row(prob.shapes[1], level0=False) == _row(prob.shapes[2])
    on = _shapes_on(prob, want)
    both = sum(1 for s in on.values() if s & {0, 1} and 2 in s)
    assert both >= 5, both  # stated with the case: >= 5 NodeClaims hold relaxed pods and pods of the plain shape
    return both


def test_relaxation_inputs(catalog):
    _pre_relaxation(*_case(catalog, build_relaxation))


@pytest.mark.gpu
def test_relaxation(ctx, catalog, ov):
    prob, want = _case(catalog, build_relaxation)
    print(prob.name, "NodeClaims with relaxed and plain pods:", _pre_relaxation(prob, want))
    _variants(ctx, ov, prob, want)


# ---- 7. host ports ---------------------------------------------------------------------------------------------
def build_host_ports(catalog):
    """A shape with a host port and the requirements of two others: a class of its own, placed by the full path (one
    NodeClaim per pod of it: the port conflicts)."""
    shapes = [_shape(required_terms=[list(ARCH)]), _shape(required_terms=[list(ARCH)], labels={"app": "second"}),
              _shape(required_terms=[list(ARCH)], host_ports=[(None, 8080, "TCP")])]
    order = [2 if i % 12 == 11 else i % 2 for i in range(240)]
    return _problem([catalog], [_pool8()], shapes, order, "rqc-hostports")


def _pre_host_ports(prob, want):
    on = _shapes_on(prob, want)
    hp = [int(nc) for p, nc in enumerate(want["placement"]) if prob.pod_shape[p] == 2]
    assert len(hp) == 20 and len(set(hp)) == 20  # stated with the case: 20 host-port pods on 20 distinct NodeClaims
    shared = sum(1 for nc in set(hp) if on[nc] & {0, 1})
    assert shared >= 5, shared  # ... at least 5 of which also hold pods of the other shapes
    return shared


def test_host_ports_inputs(catalog):
    _pre_host_ports(*_case(catalog, build_host_ports))


@pytest.mark.gpu
def test_host_ports(ctx, catalog, ov):
    prob, want = _case(catalog, build_host_ports)
    print(prob.name, "host-port NodeClaims shared with the class:", _pre_host_ports(prob, want))
    _variants(ctx, ov, prob, want)


# ---- 8. a minValues pool ---------------------------------------------------------------------------------------
def build_min_values(catalog):
    """The pool asks for two instance families (minValues): its NodeClaims take NodeClaim.Add in full for every pod,
    tagged or not."""
    from kpamd.model import NodePool
    pool = NodePool("mv", 0, 0, [("karpenter.sh/capacity-type", "In", ["on-demand"]),
                                 (K + "instance-family", "In", ["m5", "c5", "r5"], 2),
                                 (K + "instance-cpu", "In", ["8"])])
    shapes = [_shape(c, m, required_terms=[list(r)]) for c, m in SIZES for r in (ARCH, LINUX)] + \
             [_shape(250, 512), _shape(250, 512, required_terms=[[(K + "instance-family", "In", ["m5"])]])]
    order = _interleave([(0, 1), (2, 3)], 60) + _interleave([(4, 5, 6)], 120) + [7] * 6
    return _problem([catalog], [pool], shapes, order, "rqc-minvalues")


def _pre_min_values(prob, want):
    n = _redundant_on_nodeclaims(prob, want)
    assert n >= 5, n  # stated with the case: >= 5 first meetings bring a row already on the NodeClaim
    unplaced = {int(prob.pod_shape[p]) for p in np.nonzero(want["placement"] < 0)[0]}
    # the m5-only shape leaves one family (< minValues 2): unschedulable, every other pod is placed
    assert unplaced == {7} and int(np.sum(want["placement"] < 0)) == 6
    return n


def test_min_values_inputs(catalog):
    _pre_min_values(*_case(catalog, build_min_values))


@pytest.mark.gpu
def test_min_values(ctx, catalog, ov):
    prob, want = _case(catalog, build_min_values)
    print(prob.name, "redundant first meetings", _pre_min_values(prob, want))
    _variants(ctx, ov, prob, want)


# ---- 9. a topology Solve ---------------------------------------------------------------------------------------
def build_topology(catalog):
    """Zone spread over the deployment's own pods, and shapes of equal requirements beside it: with topology groups
    every level is its own class, results unchanged."""
    from kpamd.model import LabelSelector, TopologySpread
    spread = [TopologySpread(ZONE, 1, LabelSelector({"app": "spread"}))]
    shapes = [_shape(500, 1024, required_terms=[list(ARCH)], labels={"app": "spread"}, topology_spread=spread),
              _shape(500, 1024, required_terms=[list(ARCH)]), _shape(250, 512, required_terms=[list(ARCH)]),
              _shape(250, 512, required_terms=[list(LINUX)])]
    order = _interleave([(0, 1)], 90) + _interleave([(2, 3)], 120)
    return _problem([catalog], [_pool8()], shapes, order, "rqc-topology")


def _pre_topology(prob, want):
    from kpamd.catalog import ZONES
    assert bool((want["placement"] >= 0).all())
    on = _shapes_on(prob, want)
    spread_ncs = sum(1 for s in on.values() if 0 in s)
    assert spread_ncs >= len(ZONES), spread_ncs  # stated with the case: the spread pods cover >= one NodeClaim a zone
    mixed = sum(1 for s in on.values() if len(s & {1, 2}) == 2 or len(s & {0, 2}) == 2)
    assert mixed >= 3, mixed  # ... and >= 3 NodeClaims hold two shapes of the same requirements
    return mixed


def test_topology_inputs(catalog):
    _pre_topology(*_case(catalog, build_topology))


@pytest.mark.gpu
def test_topology(ctx, catalog, ov):
    prob, want = _case(catalog, build_topology)
    print(prob.name, "NodeClaims with two shapes of equal requirements:", _pre_topology(prob, want))
    _variants(ctx, ov, prob, want)


# ---- 10. existing nodes ----------------------------------------------------------------------------------------
def build_existing(catalog):
    """Case 1's queue with a few existing nodes in the Solve (the instantiation with existing nodes)."""
    from kpamd import synth
    from kpamd.model import ExistingNode
    prob = build_equal_requirements(catalog)
    it = next(t for t in catalog if t.name == "m5.2xlarge")
    for e in range(3):
        name = f"node-{e}"
        alloc = it.allocatable()
        prob.existing.append(ExistingNode(name, synth.node_labels(it, e % 3, "on-demand", "m5", name),
                                          {r: alloc[r] for r in ("cpu", "memory", "pods")}, {}, [], True))
    prob.name = "rqc-existing"
    return prob


def _pre_existing(prob, want):
    assert bool((want["placement"] != -1).all())
    on_existing = int(np.sum(want["placement"] < -1))
    assert on_existing >= 10, on_existing  # stated with the case: >= 10 pods on the existing nodes
    n = _redundant_on_nodeclaims(prob, want)
    assert n >= 10, n  # ... and >= 10 first meetings on NodeClaims bring a row already there
    return on_existing, n


def test_existing_inputs(catalog):
    _pre_existing(*_case(catalog, build_existing))


@pytest.mark.gpu
def test_existing(ctx, catalog, ov):
    prob, want = _case(catalog, build_existing)
    print(prob.name, "pods on existing nodes, redundant first meetings:", _pre_existing(prob, want))
    _variants(ctx, ov, prob, want)


# ---- 11. the chunked order -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sort_cap", [1, 5])
def test_chunked_order(ctx, catalog, ov, sort_cap):
    """Cases 1 and 3 with the sorted order forced out of LDS after a few NodeClaims (kp_overrides.sort_capacity, as
    test_chunked_order does): the chunked instantiation's writers, and its dead marks beside a class-wide NC_NEVER."""
    import kpamd
    for builder, pre in ((build_equal_requirements, _pre_equal_requirements), (build_never_in_class, _pre_never_in_class)):
        prob, want = _case(catalog, builder)
        pre(prob, want)
        assert len(want["nodeclaims"]) > 2 * sort_cap  # the order spills: more NodeClaims than the LDS order holds
        _variants(ctx, ov, prob, want, sort_capacity=sort_cap, chunk_capacity=0)
        ov(sort_capacity=sort_cap, chunk_capacity=0)
        got = kpamd.Scheduler(ctx, prob).solve()
        assert got["stats"]["order_chunks"][4] == 2, list(got["stats"]["order_chunks"])  # the Solve ended chunked
