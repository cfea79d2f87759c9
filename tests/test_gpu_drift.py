"""kp_cluster_drift on the device against the oracle of a drift simulation (tests/drift_ref.py: pyoracle.solve on the
Problem SimulateScheduling builds): every kp_drift_result field of every subset, and for the winner every pod placement
and every NodeClaim (NodePool, pods in add order, options, remaining count, final requirements). The simulations run as
whole Solves inside the general path's shared-arena launches - past two NodeClaims, which no consolidation simulation
reaches - so the launch regimes (kp_overrides.general_launch) are pinned bit for bit against the single launch."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

K = "karpenter.k8s.aws/"
UNLIMITED = 0xFFFFFFFF
HOSTNAME = "kubernetes.io/hostname"


def _val(it, key):
    for r in it.requirements:
        if r[0] == key and r[1] == "In" and len(r[2]) == 1:
            return r[2][0]
    return None


def small_catalog(catalog):
    """The amd64 c/m/r types of up to 16 vCPU (about 200 of the 919): every type config 4 launches nodes of, and a
    catalogue the oracle converts in a fifth of the time."""
    return [it for it in catalog if _val(it, K + "instance-category") in ("c", "m", "r")
            and _val(it, "kubernetes.io/arch") == "amd64" and int(_val(it, K + "instance-cpu") or 0) <= 16]


def split_cluster(catalog, topology=False):
    """Config 4, 120 nodes in two pools, after requirements drift: both NodePools now ask for instance-cpu < 5, so the
    largest type left (4 vCPU) is smaller than most nodes (2-16 vCPU) and a drifted node's pods split over several
    NodeClaims. Three nodes in four have no cpu left, so most pods go to new NodeClaims; every fourth keeps its slack,
    which takes some small nodes whole (0 NodeClaims). topology: synth.spread_cluster's zone spread on every even shape,
    and a hostname spread (maxSkew 1, DoNotSchedule, over the shape's app) on every shape with i % 4 == 1, so that
    each new NodeClaim is a hostname domain of its own."""
    from kpamd import synth
    from kpamd.model import LabelSelector, TopologySpread
    from test_gpu_budget_sweep import _two_pools
    cat = small_catalog(catalog)
    cl = _two_pools((synth.spread_cluster if topology else synth.config4)(cat, 120, seed=4))
    if topology:
        for i, sh in enumerate(cl.shapes):
            if i % 4 == 1:
                sh.topology_spread = [TopologySpread(HOSTNAME, 1, LabelSelector({"app": sh.labels["app"]}), "DoNotSchedule")]
    for p in cl.nodepools:
        p.requirements = list(p.requirements) + [(K + "instance-cpu", "Lt", ["5"])]
    for i, n in enumerate(cl.nodes):
        if i % 4:
            n.node.available = dict(n.node.available, cpu=0)
    return cl


def _check(got, want):
    """A ClusterPlan.drift(read_all=True) return against drift_ref.drift's."""
    import drift_ref
    assert len(got["results"]) == len(want["results"])
    bad = [i for i, (g, w) in enumerate(zip(got["results"], want["results"])) if g != w]
    assert not bad, \
        f"{len(bad)} subsets differ; first {bad[0]}: device {got['results'][bad[0]]} oracle {want['results'][bad[0]]}"
    assert got["first"] == want["first"] and got["blocked"] == want["blocked"]
    if want["first"] < 0:
        assert got["replacements"] is None
        return
    g, w = got["replacements"], want["replacements"]
    assert (g["placement"] == w["placement"]).all()
    assert drift_ref.nodeclaims(g) == drift_ref.nodeclaims(w)


def _same(a, b):
    """Two device returns equal bit for bit (but for the stats)."""
    import drift_ref
    assert a["results"] == b["results"] and a["first"] == b["first"] and a["blocked"] == b["blocked"]
    assert (a["replacements"] is None) == (b["replacements"] is None)
    if a["replacements"] is not None:
        assert (a["replacements"]["placement"] == b["replacements"]["placement"]).all()
        assert drift_ref.nodeclaims(a["replacements"]) == drift_ref.nodeclaims(b["replacements"])


@pytest.fixture(scope="module")
def split(catalog):
    """The split cluster, its 120 singletons and the oracle's answer (once). Oracle counts at seed 4: 37 simulations
    make >= 2 NodeClaims, 17 make >= 4 (up to 6), 9 make none; all 120 are feasible."""
    import drift_ref
    cl = split_cluster(catalog)
    subs = [[c] for c in range(len(cl.nodes))]
    want = drift_ref.drift(cl, subs)
    ncs = [r["n_nodeclaims"] for r in want["results"]]
    assert sum(n >= 2 for n in ncs) >= 30 and sum(n >= 4 for n in ncs) >= 5 and sum(n == 0 for n in ncs) >= 1
    return cl, subs, want


@pytest.fixture(scope="module")
def split_plan(ctx, split):
    import kpamd
    p = kpamd.ClusterPlan(ctx, split[0])
    yield p
    p.close()


@pytest.fixture(scope="module")
def split_prod(ctx, split, split_plan):
    """The production run: one launch."""
    ctx.set_overrides()
    got = split_plan.drift(split[1], read_all=True)
    return got


def test_split(split, split_prod):
    """1. Whole Solves past two NodeClaims: every verdict and the winner's NodeClaims equal the oracle's."""
    _, subs, want = split
    assert split_prod["stats"]["phase_cycles"][:3] == [len(subs), 0, 1]
    _check(split_prod, want)


def test_split_winner_with_many_nodeclaims(split, split_plan, ov):
    """The winner's result is read from its arena for every NodeClaim: the subsets making >= 4 NodeClaims alone, so one
    of them is first."""
    import drift_ref
    cl, subs, want = split
    many = [i for i, r in enumerate(want["results"]) if r["n_nodeclaims"] >= 4]
    got = split_plan.drift([subs[i] for i in many], read_all=True)
    assert got["first"] == 0 and got["results"] == [want["results"][i] for i in many]
    _, solve = drift_ref.simulate(cl, subs[many[0]])
    assert len(solve["nodeclaims"]) >= 4
    assert (got["replacements"]["placement"] == solve["placement"]).all()
    assert drift_ref.nodeclaims(got["replacements"]) == drift_ref.nodeclaims(solve)


def blocked_first_cluster(catalog):
    """2. The split cluster with pending pods, deleting nodes and a binding cpu limit, some nodes uninitialized, and the
    drift order chosen from the oracle's verdicts: three infeasible candidates are the oldest."""
    from kpamd import synth
    cl = synth.with_disruption_state(split_cluster(catalog), seed=9, n_deleting=2, n_pending=4, cpu_limit_m=12_000)
    return cl


@pytest.fixture(scope="module")
def blocked_first(catalog):
    import drift_ref
    cl = blocked_first_cluster(catalog)
    cands = [i for i, n in enumerate(cl.nodes) if not n.deleting and i % 3 == 0]  # (40 drifted nodes: the oracle's time)
    # a candidate pod landing on an uninitialized node counts as unscheduled: flip `initialized` on the nodes the oracle
    # shows the first feasible candidates' pods using
    probe = drift_ref.drift(cl, [[c] for c in cands])
    flipped = set()
    for i, r in enumerate(probe["results"]):
        if not r["feasible"] or len(flipped) >= 3:
            continue
        prob, kind, _, ex_nodes = drift_ref.simulation_problem(cl, [cands[i]])
        _, solve = drift_ref.simulate(cl, [cands[i]])
        used = [ex_nodes[-2 - int(t)] for p, t in enumerate(solve["placement"]) if kind[p] == 0 and t <= -2]
        if used:
            flipped.add(used[0])
    for i in flipped:
        cl.nodes[i].node.initialized = False
    want_all = drift_ref.drift(cl, [[c] for c in cands])
    feas = [bool(r["feasible"]) for r in want_all["results"]]
    bad, good = [c for c, f in zip(cands, feas) if not f], [c for c, f in zip(cands, feas) if f]
    assert len(bad) >= 3 and good, (len(bad), len(good))
    # the uninitialized-node rule decides verdicts here: with every node initialized (the probe) they differ
    assert flipped and any(a["feasible"] != b["feasible"] for a, b in zip(probe["results"], want_all["results"]))
    # drift order: three infeasible candidates oldest, then the rest by node index
    order = bad[:3] + [c for c in cands if c not in bad[:3]]
    for t, c in enumerate(order):
        cl.nodes[c].drifted = 1000.0 + t
    return cl, flipped


def test_blocked_first(ctx, blocked_first):
    import drift_ref
    import kpamd
    from kpamd import disruption
    cl, flipped = blocked_first
    order = disruption.drift_order(cl)
    subs = [[c] for c in order]
    want = drift_ref.drift(cl, subs)
    assert want["first"] >= 3 and not any(r["feasible"] for r in want["results"][:3])
    assert flipped and all(not cl.nodes[i].node.initialized for i in flipped)
    p = kpamd.ClusterPlan(ctx, cl)
    try:
        got = p.drift(subs, read_all=True)
        _check(got, want)
        cmd = disruption.Drift().compute_command(cl, p)
    finally:
        p.close()
    ref = disruption.Drift().compute_command(cl, drift_ref.OracleDriftPlan(cl))
    assert (cmd.method, cmd.candidates, cmd.decision, cmd.result["blocked"]) == \
        ("drift", [order[want["first"]]], ref.decision, order[:want["first"]])
    assert drift_ref.nodeclaims({"nodeclaims": cmd.result["replacements"]}) == \
        drift_ref.nodeclaims({"nodeclaims": ref.result["replacements"]})


@pytest.fixture(scope="module")
def topo(catalog):
    """3. The split cluster with zone and hostname spread (a general-path plan), its singletons plus 20 subsets of 2-6
    nodes. Condition on the oracle: some simulation that queues a hostname-spread pod makes >= 2 NodeClaims (at seed 4:
    131 such simulations, 92 make >= 2 NodeClaims, 43 make >= 4, one makes 25), so the per-NodeClaim hostname counts of a shared-arena launch are exercised past two
    NodeClaims."""
    import drift_ref
    cl = split_cluster(catalog, topology=True)
    spreads = [[t.topology_key for t in sh.topology_spread] for sh in cl.shapes]
    assert any(HOSTNAME in k for k in spreads) and any("topology.kubernetes.io/zone" in k for k in spreads)
    rng = np.random.default_rng(3)
    subs = [[c] for c in range(len(cl.nodes))]
    for _ in range(20):
        subs.append([int(c) for c in rng.choice(len(cl.nodes), size=int(rng.integers(2, 7)), replace=False)])
    want = drift_ref.drift(cl, subs)
    hosted = [i for i, s in enumerate(subs)
              if any(HOSTNAME in spreads[int(cl.pod_shape[p])] for c in s for p in cl.nodes[c].pods)]
    n2 = sum(want["results"][i]["n_nodeclaims"] >= 2 for i in hosted)
    n4 = sum(want["results"][i]["n_nodeclaims"] >= 4 for i in hosted)
    print(f"topo: {len(hosted)} simulations queue a hostname-spread pod; {n2} make >= 2 NodeClaims, {n4} make >= 4")
    assert n2 >= 10 and n4 >= 1
    return cl, subs, want


def test_topology(ctx, topo, ov):
    """Batched on the superset compile, and again with every subset compiled on its own: equal, and the oracle's."""
    import kpamd
    cl, subs, want = topo
    p = kpamd.ClusterPlan(ctx, cl)
    try:
        got = p.drift(subs, read_all=True)
        assert got["stats"]["phase_cycles"][:2] == [len(subs), 0]
        _check(got, want)
        ov(general_batch=1)
        one = p.drift(subs, read_all=True)
        assert one["stats"]["phase_cycles"][:3] == [0, len(subs), 0]
        _same(one, got)
    finally:
        p.close()


def test_launch_regimes(ctx, split, split_prod, ov):
    """4. general_launch = 7: 18 launches on reused dirty arenas with the winner in neither the first nor the last;
    three calls on one plan with different subset lists (the manner of test_warm_dirty_arenas), each equal bit for bit
    to the single-launch results, which equal the oracle's (test_split)."""
    import kpamd
    cl, subs, want = split
    by_len = sorted(range(len(subs)), key=lambda i: -len(cl.nodes[i].pods))  # (stable: the launches' longest-first order)
    w = by_len[60]  # (a middling length: caller index 0 of the first list lands in a middle launch, asserted below)
    perms = [[w] + [i for i in range(len(subs)) if i != w], list(range(len(subs)))[::-1], by_len[::-1][:50]]
    p = kpamd.ClusterPlan(ctx, cl)
    try:
        for k, perm in enumerate(perms):
            lst = [subs[i] for i in perm]
            # the winner (caller index 0: every simulation is feasible) in neither the first nor the last launch: its
            # position in the launches' stable longest-first order
            pos = sorted(range(len(lst)), key=lambda j: -len(cl.nodes[lst[j][0]].pods)).index(0)
            assert 0 < pos // 7 < (len(lst) + 6) // 7 - 1, (k, pos)
            ov()
            ref = p.drift(lst, read_all=True)
            assert ref["stats"]["phase_cycles"][:3] == [len(lst), 0, 1]
            assert ref["results"] == [split_prod["results"][i] for i in perm] and ref["first"] == 0
            ov(general_launch=7)
            got = p.drift(lst, read_all=True)
            assert got["stats"]["phase_cycles"][:3] == [len(lst), 0, (len(lst) + 6) // 7]
            if k == 0:
                assert got["stats"]["phase_cycles"][2] >= 18
            _same(got, ref)
    finally:
        p.close()


def test_lazy_superset_on_a_batched_kernel_plan(ctx, catalog, ov):
    """5. A plain config-4 plan is a plan of the batched simulation kernel; a drift call builds its superset Solve and
    keeps it, and simulate() stays on sim_kernel with identical output (stats: wave slots, not launches)."""
    import kpamd
    from kpamd import synth
    from oracle import pyoracle
    import drift_ref
    cl = synth.config4(small_catalog(catalog), n_nodes=60, seed=4, loose=0.1)
    subs = [[c] for c in cl.candidates[:24]] + synth.consolidation_subsets(cl, 8, seed=5, max_size=6, prefixes=False)
    p = kpamd.ClusterPlan(ctx, cl)
    try:
        before, st0 = p.simulate(subs)
        got = p.drift([[c] for c in cl.candidates[:24]], read_all=True)
        after, st1 = p.simulate(subs)
        again = p.drift([[c] for c in cl.candidates[:24]], read_all=True)
    finally:
        p.close()
    assert before == after
    # sim_kernel's stats: phase_cycles[1] wave slots launched (a multiple of the 4 waves of a workgroup), [2] the most
    # subsets any wave ran; the general path would report [len(subs), 0, launches]
    for st in (st0, st1):
        assert st["phase_cycles"][1] >= 4 and st["phase_cycles"][1] % 4 == 0 and st["phase_cycles"][2] >= 1
        assert st["phase_cycles"][1] != 0 and st["phase_cycles"][:3] != [len(subs), 0, 1]
    assert st0["phase_cycles"][:3] == st1["phase_cycles"][:3]
    want = drift_ref.drift(cl, [[c] for c in cl.candidates[:24]])
    _check(got, want)
    _same(got, again)
    # the helper against the existing oracle: DELETE exactly when every non-pending pod schedules with 0 NodeClaims
    sims, _ = pyoracle.simulate_batch(cl, [[c] for c in cl.candidates[:24]], multi_node=False)
    for s, r in zip(sims, want["results"]):
        assert (s["decision"] == 1) == (r["feasible"] == 1 and r["n_nodeclaims"] == 0) and s["n_pods"] == r["n_pods"]


def test_budgets_errors_cancel(ctx, split, split_plan, split_prod, ov):
    """6. The budget rule, the errors and cancellation of kp_cluster_simulate_budgeted."""
    import drift_ref
    import kpamd
    from kpamd import abi, disruption
    from test_gpu_budget_sweep import _csr
    cl, subs, want = split
    allowed = [0, UNLIMITED]
    adm = disruption.admissible(cl, *_csr(subs), allowed)
    pools = disruption.node_pools(cl)
    assert [bool(a) for a in adm] == [int(pools[s[0]]) != 0 for s in subs]
    got = split_plan.drift(subs, allowed=allowed, read_all=True)
    exp = [w if a else dict(drift_ref.BLOCKED) for w, a in zip(want["results"], adm)]
    assert got["results"] == exp and got["blocked"] == int((~adm).sum()) > 0
    first = next(i for i, r in enumerate(exp) if r["feasible"])
    assert got["first"] == first and adm[first]
    assert got["stats"]["phase_cycles"][0] == int(adm.sum())
    _, solve = drift_ref.simulate(cl, subs[first])
    assert drift_ref.nodeclaims(got["replacements"]) == drift_ref.nodeclaims(solve)
    with pytest.raises(kpamd.KPError) as e:
        split_plan.drift(subs, allowed=[0])
    assert e.value.code == abi.KP_E_INVAL
    cl2 = copy.deepcopy(cl)
    cl2.nodes[5].deleting = True
    p2 = kpamd.ClusterPlan(ctx, cl2)
    try:
        with pytest.raises(kpamd.KPError) as e:
            p2.drift([[4], [5]])
        assert e.value.code == abi.KP_E_INVAL
    finally:
        p2.close()
    tok = kpamd.Cancel(ctx)
    try:
        tok.set()
        with pytest.raises(kpamd.KPError) as e:
            split_plan.drift(subs, cancel=tok)
        assert e.value.code == abi.KP_E_CANCELED
    finally:
        tok.close()
    _same(split_plan.drift(subs, read_all=True), split_prod)
    # every subset infeasible: no cpu limit left on either pool, nothing fits the existing nodes
    cl3 = copy.deepcopy(cl)
    for pl in cl3.nodepools:
        pl.limits = {"cpu": 0}
    full = [[c] for c in range(len(cl3.nodes)) if c % 4 and want["results"][c]["n_nodeclaims"] > 0][:12]
    want3 = drift_ref.drift(cl3, full)
    assert want3["first"] == -1 and len(full) == 12
    p3 = kpamd.ClusterPlan(ctx, cl3)
    try:
        got3 = p3.drift(full, read_all=True)
    finally:
        p3.close()
    assert got3["first"] == -1 and got3["replacements"] is None
    _check(got3, want3)


def test_reservations(ctx, lib, catalog):
    """7. The reservation cluster of test_gpu_general_launches.test_reservations: a drifted on-demand node is replaced
    into a reservation under strict mode; the held reservation id is in the winner's final requirements."""
    import drift_ref
    import kpamd
    from test_reserved_consolidation import _reserve_nodes, reservation_cluster
    cl, crs = reservation_cluster(catalog, 70)
    cl = _reserve_nodes(lib, cl, crs, launch_into=True)
    od = [i for i, n in enumerate(cl.nodes) if n.node.labels.get("karpenter.sh/capacity-type") == "on-demand" and n.pods]
    subs = [[c] for c in od]
    want = drift_ref.drift(cl, subs)
    rid = "karpenter.k8s.aws/capacity-reservation-id"
    held = [i for i, s in enumerate(subs) if want["results"][i]["feasible"] and
            any(r[0] == rid and r[1] == "In" for n in drift_ref.simulate(cl, s)[1]["nodeclaims"] for r in n["requirements"])]
    assert held, "no drifted on-demand node is replaced into a reservation"
    p = kpamd.ClusterPlan(ctx, cl)
    try:
        got = p.drift(subs, read_all=True)
        _check(got, want)
        one = p.drift([subs[held[0]]], read_all=True)
    finally:
        p.close()
    _, solve = drift_ref.simulate(cl, subs[held[0]])
    assert one["first"] == 0 and drift_ref.nodeclaims(one["replacements"]) == drift_ref.nodeclaims(solve)
    assert any(r[0] == rid and r[1] == "In" and r[2] for n in one["replacements"]["nodeclaims"] for r in n["requirements"])


def test_min_values_route_to_the_per_subset_compile(ctx, catalog):
    """A NodePool with minValues: Truncate's minValues check runs on the host over the truncated options and can fail a
    NodeClaim's pods, so a superset compile carrying minValues sends every drift subset to the per-subset compile
    (stats phase_cycles[:3] == [0, n, 0]) and the verdict is taken from that Solve's result. instance-family minValues
    60 over the whole catalogue: the NodeClaim is created (more than 60 families fit) but its 100 cheapest options hold
    fewer, so its pods fail - asserted on the oracle (a NodeClaim left without options, its pods unscheduled) - and
    minValues 40, which the truncated options keep."""
    import drift_ref
    import kpamd
    from kpamd import synth
    for min_values, broken in ((60, True), (40, False)):
        cl = synth.config4(catalog, n_nodes=30, seed=4)
        for n in cl.nodes:
            n.node.available = dict(n.node.available, cpu=0)
        for p in cl.nodepools:
            p.requirements = list(p.requirements) + [(K + "instance-family", "Exists", [], min_values)]
        subs = [[c] for c in range(6)]
        want = drift_ref.drift(cl, subs)
        solves = [drift_ref.simulate(cl, s)[1] for s in subs]
        failed = [i for i, r in enumerate(solves) if any(not n["options"] for n in r["nodeclaims"])]
        if broken:
            assert failed and all(want["results"][i]["n_unscheduled"] > 0 and want["results"][i]["n_nodeclaims"] >= 1
                                  for i in failed)
        else:
            assert not failed and want["first"] == 0 and want["results"][0]["n_nodeclaims"] >= 1
        p = kpamd.ClusterPlan(ctx, cl)
        try:
            got = p.drift(subs, read_all=True)
        finally:
            p.close()
        assert got["stats"]["phase_cycles"][:3] == [0, len(subs), 0]
        _check(got, want)
