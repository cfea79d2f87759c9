"""A spot-reclaim storm end to end: a few dozen spot nodes over three zones carrying pods, a dozen spot
interruption messages. kpamd.interruption.Controller.reconcile parses them and resolves them on the device; its marks
go into the resident catalogue, the hit nodes are marked deleting and their pods become pending; the Solve of those pods
on the device equals pyoracle's on the same inputs, and every marked offering is unavailable to both. The message bodies
are tests/golden/interruption_messages.json's."""
import copy
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import interruption_cases as cases  # noqa: E402
import interruption_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interruption_messages.json")
N_NODES, N_MESSAGES = 36, 12


def storm_cluster(types):
    """36 nearly full spot nodes (kpamd.synth.config4's shapes and fill), each with a provider id"""
    from kpamd import synth
    cl = synth.config4(types, n_nodes=N_NODES, seed=17, pods_min=4, pods_max=12)
    for i, n in enumerate(cl.nodes):
        n.node.labels[cases.CT] = "spot"
        n.provider_id = cases.provider_id(cases.iid(0xe2e00 + i), n.node.labels[ref.ZONE])
    assert {n.node.labels[ref.ZONE] for n in cl.nodes} == set(cases.ZONES)
    return cl


def resolve_problem(cl, types, gone):
    """The Solve after the storm: the pods of the nodes in `gone` pending, the other nodes existing"""
    from kpamd.model import Problem
    pods = [p for n in sorted(gone) for p in cl.nodes[n].pods]
    return Problem([types], cl.nodepools, cl.shapes, cl.pod_shape[pods], cl.pod_creation[pods], cl.pod_uid[pods],
                   existing=[n.node for i, n in enumerate(cl.nodes) if i not in gone], name="after-the-storm")


def solved(res):
    return res["placement"].tolist(), [(n["nodepool"], n["pods"], n["options"]) for n in res["nodeclaims"]]


def test_a_spot_storm_end_to_end(ctx, catalog):
    import kpamd
    from kpamd import interruption
    from oracle import pyoracle
    with open(GOLDEN) as f:
        g = json.load(f)
    spot_body = next(m["body"] for m in g["messages"] if m["name"] == "spot_interruption")
    types = copy.deepcopy(catalog)
    cl = storm_cluster(types)
    node_ids = [interruption.instance_id(n.provider_id) for n in cl.nodes]
    hit = [int(x) for x in np.random.default_rng(5).permutation(N_NODES)[:N_MESSAGES]]
    bodies = [spot_body.replace(g["placeholder_instance_id"], node_ids[n]) for n in hit]
    bodies.insert(4, next(m["body"] for m in g["messages"] if m["name"] == "malformed_json"))
    before = pyoracle.solve(resolve_problem(cl, copy.deepcopy(types), set(hit)))   # the Solve had nothing been marked

    cat = kpamd.Catalog(ctx, types, seqnum=1)
    plan = kpamd.ClusterPlan(ctx, cl, catalogs=[cat])
    try:
        out = interruption.Controller().reconcile(bodies, cl, plan, [cat], seqnum=2)
        # the device's answer is the reference's, and it is the storm: twelve deletes, a mark per (type, zone) hit
        msgs = [(ref.SPOT, [node_ids[n]]) for n in hit]
        want = ref.resolve(cl, msgs, node_ids)
        assert out.nodes == want["nodes"] and out.matches == want["matches"] == [1] * N_MESSAGES
        assert out.parse_errors == 1 and out.received["spot_interrupted"] == N_MESSAGES
        assert sorted(d[0] for d in out.deletes) == sorted(hit)
        assert out.disrupted == {("spot_interrupted", "default", "spot"): N_MESSAGES}
        pairs = {(cl.nodes[n].node.labels[ref.ITYPE], cl.nodes[n].node.labels[ref.ZONE]) for n in hit}
        assert {m[:2] for m in out.marks} == pairs and sum(m[2] for m in out.marks) == N_MESSAGES
        # the marks are in the catalogue: behind the ABI (the seqnum moved, the plan is stale until refreshed) and in
        # the model the oracle reads
        assert cat.seqnum() == 2 and len(out.updates[0]) == len(pairs)
        with pytest.raises(kpamd.KPError, match="stale plan"):
            plan.interruptions(msgs, node_ids)
        plan.refresh()
        by_name = {it.name: it for it in types}
        for name, zone in pairs:
            offs = [o for o in by_name[name].offerings if o.capacity_type == "spot" and o.zone == zone]
            assert offs and not any(o.available for o in offs)
        # the API deletes: the hit nodes are deleting, their pods pending; a second delivery of the batch finds them so
        for n, _, _ in out.deletes:
            cl.nodes[n].deleting = True
        again = kpamd.ClusterPlan(ctx, cl, catalogs=[cat])
        try:
            redelivered = again.interruptions(msgs, node_ids)
        finally:
            again.close()
        assert redelivered["deletes"] == [] and len(redelivered["marks"]) == len(pairs)
        assert all(redelivered["nodes"][n]["flags"] == ref.ALREADY_DELETING | ref.ICE for n in hit)
        # the re-Solve
        prob = resolve_problem(cl, types, set(hit))
        assert prob.n_pods >= 3 * N_MESSAGES
        got = kpamd.Scheduler(ctx, prob, catalogs=[cat]).solve()
        oracle = pyoracle.solve(prob)
        assert solved(got) == solved(oracle)
        assert len(got["nodeclaims"]) > 0
        assert solved(oracle) != solved(before)          # the marks changed what the Solve may launch
    finally:
        plan.close()
        cat.close()
