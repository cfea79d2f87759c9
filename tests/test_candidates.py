"""Candidate selection (kp_cluster_candidates). CPU half: every builder of tests/candidate_cases.py against
its hand-written expectation through the plain-Python reference (tests/candidate_ref.py), so that each case is shown to
be the edge it claims. GPU half: the device against the reference with == on every record field and on the order."""
import copy
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import candidate_cases as cases  # noqa: E402
import candidate_ref as ref  # noqa: E402

NOW = cases.NOW
E, S, M, D = ref.METHODS


def names_of(cluster, order):
    return [cluster.nodes[i].node.name for i in order]


# ---- CPU: the builders are the edges they claim ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edges(catalog):
    return cases.edges(catalog)


def test_docs_example(catalog):
    """disruption.md:342-349: pods A, B, C with PDB-1, PDB-2, PDB-3 give PDB_BLOCKED, detail PDB-1; with PDB-2 alone
    (maxUnavailable 1: disruptions_allowed 1) pod A's node is a candidate."""
    cl, want = cases.docs_example(catalog)
    recs, order = ref.candidates(cl, cl.controls, S, NOW)
    assert recs[0][:2] == want["docs"] == (ref.PDB_BLOCKED, 0) and order == []
    assert cl.controls.pdbs[0].name == "PDB-1"
    cl, want = cases.docs_example(catalog, pdb2_only=True)
    recs, order = ref.candidates(cl, cl.controls, S, NOW)
    assert recs[0][:2] == want["docs"] == (ref.CANDIDATE, 0) and order == [0]


def test_edges_reasons(edges):
    cl, want, _ = edges
    assert set(want) == {n.node.name for n in cl.nodes}
    seen = set()
    for m in ref.METHODS:
        recs, _ = ref.candidates(cl, cl.controls, m, NOW)
        for i, n in enumerate(cl.nodes):
            assert recs[i][:2] == want[n.node.name][m], (n.node.name, m)
            seen.add((m, recs[i][0]))
    for m in ref.METHODS:  # one node per reason code a method can give
        codes = set(range(8)) | ({8, 10} if m != D else {12}) | ({9} if m in (S, M) else set()) | ({11} if m == E else set())
        assert {r for mm, r in seen if mm == m} == codes, m


def test_edges_costs(edges):
    cl, _, cost = edges
    recs, _ = ref.candidates(cl, cl.controls, S, NOW)
    by = {n.node.name: recs[i] for i, n in enumerate(cl.nodes)}
    for name, (fx, c) in cost.items():
        assert by[name][2] == fx and by[name][3] == c, name
    assert math.copysign(1.0, by["nz-b"][3]) == -1.0 and by["nz-b"][3] == 0.0      # -0.0
    assert math.copysign(1.0, by["nz-a"][3]) == 1.0
    a, b = by["ulp-a"][3], by["ulp-b"][3]
    assert a != b and a == math.nextafter(b, math.inf)                             # one ulp apart
    assert by["all-hi-129"][2] == 129 * 10 * (1 << 27) and by["neg-sum"][2] < 0


def test_edges_order(edges):
    cl, _, _ = edges
    _, order = ref.candidates(cl, cl.controls, D, NOW)
    assert names_of(cl, order) == cases.EDGES_DRIFT_ORDER
    _, order = ref.candidates(cl, cl.controls, S, NOW)
    names = names_of(cl, order)
    assert names[:3] == cases.EDGES_SINGLE_HEAD
    assert names[3:3 + len(cases.EDGES_SINGLE_ZEROS)] == cases.EDGES_SINGLE_ZEROS
    k = names.index("ulp-b")
    assert names[k:k + 2] == cases.EDGES_SINGLE_ULP
    assert names[-1] == "all-hi-129"


def test_order_builders(catalog):
    cl = cases.order_cluster(catalog)
    names = [n.node.name for n in cl.nodes]
    assert len(set(names)) == cases.ORDER_NODES
    by_bytes = sorted(range(len(names)), key=lambda i: names[i].encode())
    assert by_bytes != list(range(len(names)))                                     # not the index order
    assert by_bytes != sorted(range(len(names)), key=lambda i: int(names[i][1:]))  # nor the numeric order
    for k in (1, 65, cases.TILE + 1):
        ctl, keep = cases.order_controls(cl, k)
        recs, order = ref.candidates(cl, ctl, S, NOW)
        assert sorted(order) == keep and len(order) == k
        assert order == sorted(keep, key=lambda i: (i % 4, names[i].encode()))
    eq = cases.equal_costs(catalog)
    recs, order = ref.candidates(eq, eq.controls, S, NOW)
    assert {r[3] for r in recs} == {0.0} and len(order) == 257
    assert names_of(eq, order) == [x.decode() for x in sorted(n.node.name.encode() for n in eq.nodes)]


def test_pdb_builders(catalog):
    cl = cases.pdb_cluster(catalog)
    for n, blocking, want in cases.PDB_CASES:
        recs, order = ref.candidates(cl, cases.pdb_controls(cl, n, blocking), S, NOW)
        for j in range(8):
            assert recs[j][:2] == ((ref.PDB_BLOCKED, want[j]) if j in want else (ref.CANDIDATE, 0)), (n, blocking, j)


def _initialized(cl):
    for n in cl.nodes:
        n.node.initialized = True
    return cl


def test_default_controls_keep_candidate_order(catalog):
    """With every control at its default the reference's order is the existing candidate_order (pod count, then name),
    on a 120-node config-4 cluster and on three random clusters. random_cluster leaves 5% of its nodes uninitialized,
    which the rule excludes (NOT_INITIALIZED) and candidate_order does not know of: the comparison is made with them
    initialized, and as generated against candidate_order without them."""
    from kpamd import disruption, synth
    from kpamd.model import DisruptionControls
    clusters = [synth.config4(catalog, n_nodes=120, seed=4)] + [synth.random_cluster(catalog, seed) for seed in (1, 2, 3)]
    for cl in clusters:
        _, order = ref.candidates(cl, DisruptionControls.default(cl), S, NOW)
        assert order == [c for c in disruption.candidate_order(cl) if cl.nodes[c].node.initialized], cl.name
        cl = _initialized(copy.deepcopy(cl))
        _, order = ref.candidates(cl, DisruptionControls.default(cl), M, NOW)
        assert order == disruption.candidate_order(cl) and len(order) == len(cl.nodes), cl.name


def test_randomized_builder_reaches_the_rule(catalog):
    """add_disruption_controls spreads a 120-node cluster over most reasons, and leaves candidates under every method."""
    from kpamd import synth
    cl = synth.config4(catalog, n_nodes=120, seed=4)
    synth.add_disruption_controls(cl, 0)
    reasons = set()
    for m in ref.METHODS:
        recs, order = ref.candidates(cl, cl.controls, m, NOW)
        reasons |= {r[0] for r in recs}
        assert order or m == E
    assert len(reasons) >= 7 and {ref.POD_DO_NOT_DISRUPT, ref.PDB_BLOCKED} <= reasons


@pytest.fixture(scope="module")
def controller_case(catalog):
    """The 12-node controller cluster with the three commands the oracle computes: from the reference's candidate
    lists, and with controls=None."""
    from e2e import OraclePlan
    from kpamd import disruption
    cl, fewest, nxt = cases.controller_cluster(catalog)
    with_controls = disruption.Controller().compute_command(cl, ref.RefPlan(cl, OraclePlan(cl)), now=NOW)
    bare = copy.copy(cl)
    bare.controls = None
    without = disruption.Controller().compute_command(bare, OraclePlan(bare), now=NOW)
    return cl, fewest, nxt, with_controls, without


def test_controller_oracle(controller_case):
    """The controls change the command: the node with the fewest pods is PDB-blocked and the next one costs more than
    its pod count says, so the oracle fed with the reference's lists picks another command than controls=None."""
    from kpamd import disruption
    cl, fewest, nxt, with_controls, without = controller_case
    recs, order = ref.candidates(cl, cl.controls, S, NOW)
    assert recs[fewest][:2] == (ref.PDB_BLOCKED, 0) and fewest not in order
    assert order.index(nxt) > 0 and disruption.candidate_order(cl)[:2] == [fewest, nxt]
    assert with_controls is not None and without is not None
    assert (with_controls.method, with_controls.candidates, with_controls.decision) != \
        (without.method, without.candidates, without.decision)
    assert fewest in without.candidates and fewest not in with_controls.candidates


# ---- GPU: device == reference ---------------------------------------------------------------------------------------
def check(plan, cl, controls=None, methods=ref.METHODS, now=NOW):
    """plan.candidates against the reference: every field of every record and the order list, with ==."""
    controls = cl.controls if controls is None else controls
    out = {}
    for m in methods:
        want_recs, want_order = ref.candidates(cl, controls, m, now)
        recs, order, _ = plan.candidates(m, now, controls=controls)
        assert len(recs) == len(want_recs)
        for i, w in enumerate(want_recs):
            g = recs[i]
            got = (int(g["reason"]), int(g["detail"]), int(g["rescheduling_cost_fx"]), float(g["disruption_cost"]))
            assert got == w and math.copysign(1.0, got[3]) == math.copysign(1.0, w[3]), (cl.name, m, cl.nodes[i].node.name, got, w)
        assert order == want_order, (cl.name, m)
        out[m] = (recs, order)
    return out


@pytest.fixture(scope="module")
def shared_catalog(ctx, catalog):
    import kpamd
    c = kpamd.Catalog(ctx, cases.tiny_catalog(catalog))
    yield c
    c.close()


@pytest.fixture(scope="module")
def planned(ctx, shared_catalog):
    """ClusterPlan of a crafted cluster (they share the three-type catalogue), closed at the end of the module."""
    import kpamd
    made = []

    def make(cl):
        made.append(kpamd.ClusterPlan(ctx, cl, catalogs=[shared_catalog]))
        return made[-1]
    yield make
    for p in made:
        p.close()


@pytest.mark.gpu
def test_gpu_docs_example(catalog, planned):
    for pdb2_only in (False, True):
        cl, _ = cases.docs_example(catalog, pdb2_only)
        check(planned(cl), cl)


@pytest.mark.gpu
def test_gpu_edges(edges, planned):
    """Pods per node at the chunk edges, the cost clamp and sums, lifetime, PDB forms, the ladder under each method."""
    cl, want, _ = edges
    got = check(planned(cl), cl)
    recs, order = got[D]
    assert names_of(cl, order) == cases.EDGES_DRIFT_ORDER
    i = next(i for i, n in enumerate(cl.nodes) if n.node.name == "tgp-blocked")
    assert int(got[D][0][i]["reason"]) == ref.CANDIDATE and int(got[S][0][i]["reason"]) == ref.PDB_BLOCKED


@pytest.mark.gpu
def test_gpu_order_counts(catalog, planned):
    """1 .. 4,200 candidates out of 4,200 nodes, the LDS tile's capacity - 1, + 0, + 1 among them; twice, for the same
    answer."""
    cl = cases.order_cluster(catalog)
    plan = planned(cl)
    for k in cases.ORDER_COUNTS:
        ctl, keep = cases.order_controls(cl, k)
        got = check(plan, cl, ctl, methods=(S,))
        assert len(got[S][1]) == k
        again = plan.candidates(S, NOW, controls=ctl)
        assert again[1] == got[S][1] and (again[0] == got[S][0]).all()


@pytest.mark.gpu
def test_gpu_equal_costs(catalog, planned):
    cl = cases.equal_costs(catalog)
    got = check(planned(cl), cl, methods=(S, E))
    assert len(got[S][1]) == 257


@pytest.mark.gpu
def test_gpu_pdb_counts(catalog, planned):
    cl = cases.pdb_cluster(catalog)
    plan = planned(cl)
    for n, blocking, _ in cases.PDB_CASES:
        check(plan, cl, cases.pdb_controls(cl, n, blocking), methods=(S, D))


@pytest.fixture(scope="module")
def full_catalog(ctx, catalog):
    import kpamd
    c = kpamd.Catalog(ctx, catalog)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_gpu_randomized(ctx, catalog, full_catalog, seed):
    import kpamd
    from kpamd import synth
    cl = synth.config4(catalog, n_nodes=120, seed=20 + seed)
    synth.add_disruption_controls(cl, seed)
    plan = kpamd.ClusterPlan(ctx, cl, catalogs=[full_catalog])
    try:
        check(plan, cl)
    finally:
        plan.close()


@pytest.mark.gpu
def test_gpu_randomized_2000(ctx, catalog, full_catalog):
    import kpamd
    from kpamd import synth
    cl = synth.config4(catalog, n_nodes=2000, seed=31)
    synth.add_disruption_controls(cl, 31, n_pdbs=40)
    plan = kpamd.ClusterPlan(ctx, cl, catalogs=[full_catalog])
    try:
        check(plan, cl)
    finally:
        plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["batched", "general"])
def test_gpu_both_plan_kinds(ctx, catalog, full_catalog, kind):
    """A plan of the batched simulation kernel and a general-path (spread) plan: the candidates equal the reference,
    and kp_cluster_simulate on the same plan answers after the call what it answered before it."""
    import kpamd
    from kpamd import synth
    cl = synth.config4(catalog, n_nodes=60, seed=5) if kind == "batched" else synth.spread_cluster(catalog, 40, seed=5)
    synth.add_disruption_controls(cl, 9)
    plan = kpamd.ClusterPlan(ctx, cl, catalogs=[full_catalog])
    try:
        subsets = [cl.candidates[:k] for k in (1, 2, 5)] + [[c] for c in cl.candidates[5:9]]
        before, _ = plan.simulate(subsets, multi_node=True)
        check(plan, cl)
        after, _ = plan.simulate(subsets, multi_node=True)
        assert after == before
        check(plan, cl, methods=(S,))
    finally:
        plan.close()


def _raw(plan, cl, ci, out=True, order=True, count=True):
    from kpamd import abi
    n = len(cl.nodes)
    o = np.zeros(n, dtype=abi.candidate_dtype())
    od = np.zeros(n, dtype=np.uint32)
    cnt = C.c_uint32(7)
    rc = plan.ctx.lib.kp_cluster_candidates(plan.h, C.byref(ci), o.ctypes.data if out else None,
                                            od.ctypes.data_as(C.POINTER(C.c_uint32)) if order else None,
                                            C.byref(cnt) if count else None, None)
    return rc, cnt.value


@pytest.mark.gpu
def test_gpu_errors(ctx, catalog, planned):
    """Each KP_E_INVAL: a count that differs from the snapshot, a NULL required array, an unknown method and selector
    operator; then the stale plan."""
    import kpamd
    from kpamd import abi
    cl, _ = cases.docs_example(catalog)
    plan = planned(cl)

    def fresh(**kw):
        arena = abi.Arena()
        ci = abi.build_candidates_in(arena, cl.controls, kw.pop("method", S), NOW)
        for k, v in kw.items():
            setattr(ci, k, v)
        return arena, ci

    assert _raw(plan, cl, fresh()[1]) == (abi.KP_OK, 0)
    for kw in (dict(n_pools=2), dict(n_nodes=2), dict(n_nodes=0), dict(n_pods=2), dict(pools=None), dict(nodes=None),
               dict(pods=None), dict(pdbs=None), dict(method=4), dict(method=-1)):
        keep, ci = fresh(**kw)
        assert _raw(plan, cl, ci) == (abi.KP_E_INVAL, 0), kw
    keep, ci = fresh()
    for kw in (dict(out=False), dict(order=False), dict(count=False)):
        assert _raw(plan, cl, ci, **kw)[0] == abi.KP_E_INVAL, kw
    assert plan.ctx.lib.kp_cluster_candidates(plan.h, None, None, None, None, None) == abi.KP_E_INVAL
    keep, ci = fresh()
    ci.pdbs[0].selector.match_expressions = keep.arr(abi.SelectorRequirement, [abi.SelectorRequirement(b"app", 9, 0, None)])
    ci.pdbs[0].selector.n_match_expressions = 1
    assert _raw(plan, cl, ci) == (abi.KP_E_INVAL, 0)
    assert _raw(plan, cl, fresh()[1]) == (abi.KP_OK, 0)  # the plan serves on after every refusal
    # a stale plan: the catalogue's seqnum moved since kp_cluster_prepare; kp_cluster_refresh brings it back
    its = copy.deepcopy(cl.catalogs[0])
    cat = kpamd.Catalog(ctx, its, seqnum=1)
    p = kpamd.ClusterPlan(ctx, cl, catalogs=[cat])
    try:
        check(p, cl, methods=(S,))
        o = next(o for o in its[0].offerings if o.available)
        cat.update_offerings([(0, o.capacity_type, o.zone, False)], seqnum=2)
        with pytest.raises(kpamd.KPError, match="stale plan") as e:
            p.candidates(S, NOW)
        assert e.value.code == abi.KP_E_INVAL
        p.refresh()
        check(p, cl, methods=(S,))
    finally:
        p.close()
        cat.close()


@pytest.mark.gpu
def test_gpu_controller(ctx, catalog, full_catalog, controller_case):
    """Controller.compute_command with the device's candidate lists picks the command the oracle picks from the
    reference's lists."""
    import kpamd
    from kpamd import disruption
    cl, fewest, nxt, want, _ = controller_case
    plan = kpamd.ClusterPlan(ctx, cl, catalogs=[full_catalog])
    try:
        got = disruption.Controller().compute_command(cl, plan, now=NOW)
        recs, order = disruption.candidates(cl, plan, "single", NOW)
        assert int(recs[fewest]["reason"]) == ref.PDB_BLOCKED and fewest not in order
    finally:
        plan.close()
    assert got is not None
    assert (got.method, got.candidates, got.decision) == (want.method, want.candidates, want.decision)
