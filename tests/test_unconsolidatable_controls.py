"""disruption.unconsolidatable on a cluster with DisruptionControls and a NodePool budget: the nodes that are no
candidates carry their kp_candidate reason (the blocking PDB renders the documented "pdb <ns>/<name> prevents pod
evictions", R:website/content/en/preview/concepts/disruption.md:105-113), the candidates the budget walk skips carry the
BUDGET record without a simulation, and the rest their singleton's exit. Expectations are written by hand; the CPU half
runs on the reference plans (candidate_ref.RefPlan over why_ref.OracleWhyPlan), the gpu half on the device."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import candidate_ref  # noqa: E402
import option_order_cases as oc  # noqa: E402
import why_cases  # noqa: E402
import why_ref  # noqa: E402

NOW = 1_750_100_000
BACKENDS = ["reference", pytest.param("device", marks=pytest.mark.gpu)]
# kp_candidate_reason values (kp_abi.h)
NODE_DO_NOT_DISRUPT, NOT_INITIALIZED, PDB_BLOCKED = 2, 3, 7


def build(lib):
    """Seven one-pod nodes of one NodePool whose budget allows two disruptions. In node order: a node that can be
    replaced; one whose pod the second PDB blocks; a do-not-disrupt node; a node at the cheapest option's price; a
    candidate the walk skips; an uninitialized node; another candidate the walk skips. Every candidate has the same
    disruption cost, so the walk goes by name: node order."""
    from kpamd.model import Budget, DisruptionControls, LabelSelector, PodDisruptionBudget
    its = oc.fresh(lib)
    ts = oc.shuffled_usable(its, 30, 45)
    cand, cheap = [t for t in oc.usable(its) if t not in set(ts)][:2]
    oc.price_everywhere(its, ts, [0.25 + j / 4096 for j in range(len(ts))])
    oc.price_on_demand(its[cand], 1.0)
    oc.price_on_demand(its[cheap], 0.25)
    shapes = [why_cases._pod(labels={"app": "web"}), why_cases._pod(labels={"app": "inflate"})]
    nodes = [{"type": cand, "pods": [0]}, {"type": cand, "pods": [1]}, {"type": cand, "pods": [0]},
             {"type": cheap, "pods": [0]}, {"type": cand, "pods": [0]}, {"type": cand, "pods": [0], "initialized": False},
             {"type": cand, "pods": [0]}]
    pool = why_cases._pool([(oc.CT, "In", ["on-demand"]), (oc.IT, "In", [its[t].name for t in ts])], budgets=[Budget("2")])
    cl = why_cases._cluster(its, nodes, shapes, [pool], "why-controls")
    cl.controls = DisruptionControls.default(cl)
    cl.controls.nodes[2].do_not_disrupt = True
    cl.controls.pdbs = [PodDisruptionBudget("default", "other-pdb", LabelSelector({"app": "absent"}), 0),
                        PodDisruptionBudget("default", "inflate-pdb", LabelSelector({"app": "inflate"}), 0)]
    return cl


@pytest.mark.parametrize("backend", BACKENDS)
def test_entries_and_messages(request, lib, backend):
    from kpamd import disruption
    cl = build(lib)
    if backend == "device":
        import kpamd
        plan = kpamd.ClusterPlan(request.getfixturevalue("ctx"), cl)
    else:
        plan = candidate_ref.RefPlan(cl, why_ref.OracleWhyPlan(cl))
    try:
        entries = disruption.unconsolidatable(cl, plan, now=NOW)
    finally:
        plan.close()
    assert [e["node"] for e in entries] == list(range(7))
    msg = [disruption.unconsolidatable_message(e) for e in entries]
    # the nodes that are no candidates: DESIGN 14's reason and detail, no simulation
    assert [(e["candidate_reason"], e["detail"], e["pdb"]) for e in entries] == [
        (0, 0, None), (PDB_BLOCKED, 1, ("default", "inflate-pdb")), (NODE_DO_NOT_DISRUPT, 0, None), (0, 0, None),
        (0, 0, None), (NOT_INITIALIZED, 0, None), (0, 0, None)]
    assert all(entries[i]["why"] is None and entries[i]["sim"] is None for i in (1, 2, 5))
    assert msg[1] == "pdb default/inflate-pdb prevents pod evictions"
    assert msg[2] and msg[5] and msg[2] != msg[5]
    # the two candidates the budget of 2 admits were simulated: a REPLACE and the pinned text
    one = dict(n_nodeclaims=1, n_truncated=30, cheapest_launch=0.25)
    assert why_ref.bits(entries[0]["why"]) == why_ref.bits(why_ref.record(why_ref.NONE, n_cheaper=30, n_same_type=30, **one))
    assert entries[0]["sim"]["decision"] == 2 and msg[0] is None
    assert why_ref.bits(entries[3]["why"]) == why_ref.bits(why_ref.record(why_ref.NOT_CHEAPER, **one))
    assert entries[3]["sim"]["decision"] == 0 and msg[3] == "can't replace with a lower-priced node"
    # the walk skipped the other two: BUDGET, not simulated
    for i in (4, 6):
        assert why_ref.bits(entries[i]["why"]) == why_ref.bits(why_ref.record(why_ref.BUDGET)) and entries[i]["sim"] is None
        assert msg[i]
