"""Drift on the CPU: the candidate order, the empty candidates under budgets, the zero-allowance skip, the method's
place in the controller, and Drift.compute_command against a plan stand-in that answers drift() from the oracle helper
(tests/drift_ref.py). The helper itself is pinned against the existing oracle first: pyoracle.simulate_batch says DELETE
exactly when the helper's Solve schedules every non-pending pod with no NodeClaim."""
import copy
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

K = "karpenter.k8s.aws/"


def _small(catalog):
    from test_gpu_drift import small_catalog
    return small_catalog(catalog)


@pytest.fixture(scope="module")
def cluster(catalog):
    """Config 4, 24 nodes in two pools (every third node in burst), a tenth of the nodes loose."""
    from kpamd import synth
    from test_gpu_budget_sweep import _two_pools
    return _two_pools(synth.config4(_small(catalog), n_nodes=24, seed=4, loose=0.1))


def _budget(cl, default=None, burst=None):
    from kpamd.model import Budget
    cl = copy.deepcopy(cl)
    for p, b in zip(cl.nodepools, (default, burst)):
        p.budgets = [Budget(b)] if b is not None else []
    return cl


def test_helper_against_the_existing_oracle(catalog, cluster):
    """simulate_batch's DELETE <=> the helper's Solve is feasible with 0 NodeClaims; n_pods equal. Also with pending
    pods, deleting nodes and a cpu limit."""
    import drift_ref
    from kpamd import synth
    from oracle import pyoracle
    for cl in (cluster, synth.with_disruption_state(cluster, seed=3, n_deleting=2, n_pending=4, cpu_limit_m=8000)):
        subs = [[c] for c in range(len(cl.nodes)) if not cl.nodes[c].deleting]
        sims, _ = pyoracle.simulate_batch(cl, subs, multi_node=False)
        ref = drift_ref.drift(cl, subs)
        assert any(s["decision"] == 1 for s in sims) or cl is not cluster
        for s, r in zip(sims, ref["results"]):
            assert (s["decision"] == 1) == (r["feasible"] == 1 and r["n_nodeclaims"] == 0), (s, r)
            assert s["n_pods"] == r["n_pods"]
            if s["decision"] != 0:
                assert r["feasible"] == 1


def test_candidate_order(cluster):
    from kpamd import disruption
    cl = copy.deepcopy(cluster)
    assert disruption.drift_order(cl) == []
    cl.nodes[5].drifted, cl.nodes[2].drifted, cl.nodes[9].drifted, cl.nodes[7].drifted = 50.0, 10.0, 10.0, 5.0
    cl.nodes[11].drifted, cl.nodes[11].deleting = 1.0, True
    assert cl.nodes[2].node.name < cl.nodes[9].node.name
    assert disruption.drift_order(cl) == [7, 2, 9, 5]


def test_empty_candidates_under_budgets(cluster):
    """Empty drifted nodes: one DELETE command, as many as Drifted allows per pool, without touching the plan."""
    import drift_ref
    from kpamd import disruption
    base = copy.deepcopy(cluster)
    pools = disruption.node_pools(base)
    d = [i for i in range(len(base.nodes)) if pools[i] == 0][:3]
    b = [i for i in range(len(base.nodes)) if pools[i] == 1][:2]
    for t, i in enumerate(d + b):
        base.nodes[i].pods = []
        base.nodes[i].drifted = float(t)
    base.nodes[d[2] + 1 if pools[d[2] + 1] == 0 else d[2] + 2].drifted = 0.5  # a drifted node with pods: not in the command
    for (bd, bb), want in ((("0", "1"), b[:1]), (("1", None), d[:1] + b), ((None, None), d + b), (("0", "0"), None)):
        cl = _budget(base, bd, bb) if (bd, bb) != (None, None) else base
        plan = drift_ref.OracleDriftPlan(cl)
        cmd = disruption.Drift().compute_command(cl, plan)
        if want is None:  # nothing kept: the candidates with pods are tried, every pool at 0: no command
            assert cmd is None and plan.calls == []
            continue
        assert (cmd.method, cmd.candidates, cmd.decision, cmd.result["replacements"]) == ("drift", want, disruption.DELETE, [])
        assert plan.calls == []


def test_budget_reason_is_drifted(cluster):
    from kpamd import disruption
    from kpamd.model import Budget
    cl = copy.deepcopy(cluster)
    cl.nodepools[0].budgets = [Budget("0", reasons=["Drifted"]), Budget("5", reasons=["Underutilized"])]
    cl.nodepools[1].budgets = [Budget("0", reasons=["Empty"])]
    assert disruption.allowed_disruptions(cl, disruption.DRIFTED) == [0, disruption.UNLIMITED]


def test_zero_allowance_pool_is_skipped(cluster):
    """The oldest candidate's pool allows nothing: a younger candidate of the other pool wins, and the skipped one is
    not even simulated."""
    import drift_ref
    from kpamd import disruption
    cl = _budget(cluster, "0", "2")
    pools = disruption.node_pools(cl)
    old = next(i for i in range(len(cl.nodes)) if pools[i] == 0 and cl.nodes[i].pods)
    young = [i for i in range(len(cl.nodes)) if pools[i] == 1 and cl.nodes[i].pods][:2]
    cl.nodes[old].drifted, cl.nodes[young[0]].drifted, cl.nodes[young[1]].drifted = 1.0, 2.0, 3.0
    plan = drift_ref.OracleDriftPlan(cl)
    cmd = disruption.Drift().compute_command(cl, plan)
    ref = drift_ref.drift(cl, [[c] for c in young], allowed=[0, 2])
    assert ref["first"] >= 0 and plan.calls == ["drift"]
    assert cmd.candidates == [young[ref["first"]]] and cmd.result["blocked"] == young[:ref["first"]]
    assert old not in cmd.candidates + cmd.result["blocked"]


def test_compute_command_against_the_helper(cluster):
    """The command is (first feasible candidate in drift order, every NodeClaim of its Solve); tight NodePools make the
    replacement split."""
    import drift_ref
    from kpamd import disruption
    cl = copy.deepcopy(cluster)
    for p in cl.nodepools:
        p.requirements = list(p.requirements) + [(K + "instance-cpu", "Lt", ["5"])]
    for i, n in enumerate(cl.nodes):
        n.node.available = dict(n.node.available, cpu=0)
    big = sorted((i for i in range(len(cl.nodes))), key=lambda i: -len(cl.nodes[i].pods))[:4]
    for t, i in enumerate(big):
        cl.nodes[i].drifted = float(t)
    plan = drift_ref.OracleDriftPlan(cl)
    cmd = disruption.Drift().compute_command(cl, plan)
    verdict, solve = drift_ref.simulate(cl, [big[0]])
    assert verdict["feasible"] and verdict["n_nodeclaims"] >= 2
    assert (cmd.method, cmd.candidates, cmd.decision, cmd.result["blocked"]) == ("drift", [big[0]], disruption.REPLACE, [])
    assert drift_ref.nodeclaims({"nodeclaims": cmd.result["replacements"]}) == drift_ref.nodeclaims(solve)
    assert all(len(n["options"]) <= 100 and n["options"] for n in cmd.result["replacements"])
    # no cpu limit left: every candidate is blocked, no command
    for p in cl.nodepools:
        p.limits = {"cpu": 0}
    plan = drift_ref.OracleDriftPlan(cl)
    assert disruption.Drift().compute_command(cl, plan) is None and plan.calls == ["drift"]


def test_controller_order_and_no_drift_is_unchanged(cluster):
    """Emptiness, then Drift, then the consolidation methods; without a drifted node the plan sees no drift() call and
    the command is the one the consolidation methods alone give."""
    import drift_ref
    from kpamd import disruption
    cl = copy.deepcopy(cluster)
    plan = drift_ref.OracleDriftPlan(cl)
    base = disruption.Controller().compute_command(cl, plan)
    assert "drift" not in plan.calls and plan.calls and base is not None and base.method in ("multi", "single")
    cl.nodes[3].drifted = 1.0
    plan = drift_ref.OracleDriftPlan(cl)
    cmd = disruption.Controller().compute_command(cl, plan)
    assert cmd.method == "drift" and cmd.candidates == [3] and plan.calls == ["drift"]  # before MultiNode
    cl.nodes[8].pods = []
    plan = drift_ref.OracleDriftPlan(cl)
    cmd = disruption.Controller().compute_command(cl, plan)
    assert cmd.method == "emptiness" and plan.calls == []  # Emptiness first


def test_no_drifted_node_same_commands_on_an_e2e_cluster(lib):
    """One consolidation trajectory over the e2e cluster model (tests/e2e.py: 12 pods provisioned, scaled to 5 at random,
    consolidated to the fixed point) with no drifted node: at every pass the controller never calls drift() and gives
    the command a controller without the Drift method gives. The scenarios of tests/test_e2e_suites.py themselves run
    unchanged through the same Controller, oracle and device, and pin the rest."""
    import drift_ref
    from kpamd import disruption

    class NoDrift(disruption.Controller):
        def compute_command(self, cluster, plan, now=None, not_ready=(), extra_deleting=None):
            saved, disruption.Drift.compute_command = disruption.Drift.compute_command, lambda *a, **k: None
            try:
                return super().compute_command(cluster, plan, now, not_ready, extra_deleting)
            finally:
                disruption.Drift.compute_command = saved

    import e2e
    from kpamd import synth
    env = e2e.Env("oracle", lib)
    env.pools.append(e2e.default_nodepool())
    env.deploy("web", synth.PodShape(synth.req_res(1000, 1024)), 12)
    env.provision()
    env.scale("web", 5, seed=1)
    for _ in range(6):
        cl, names = env.cluster()
        plan = drift_ref.OracleDriftPlan(cl)
        cmd = disruption.Controller().compute_command(cl, plan)
        ref = NoDrift().compute_command(cl, drift_ref.OracleDriftPlan(cl))
        assert "drift" not in plan.calls
        assert (cmd is None) == (ref is None)
        if cmd is None:
            break
        assert (cmd.method, cmd.candidates, cmd.decision) == (ref.method, ref.candidates, ref.decision)
        env._apply(cl, names, cmd)
