"""Drift detection (kp_cluster_detect_drift), the CPU half: every builder of tests/driftdet_cases.py against
its hand-written expectation through the plain-Python reference (tests/driftdet_ref.py), so that each case is shown to
be the edge it claims; the generator's helper against the oracle; the spread of the randomized clusters; and the life
of the Drifted condition (disruption.detect_drift) over a plan that answers from the reference. The device is held to
the same reference in tests/test_gpu_driftdet.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import driftdet_cases as cases  # noqa: E402
import driftdet_ref as ref  # noqa: E402
from kpamd import abi, disruption, synth  # noqa: E402


def check(built):
    cl, want = built
    assert set(want) == {n.node.name for n in cl.nodes} and len(want) == len(cl.nodes)
    records, counts = ref.detect(cl)
    for node, rec in zip(cl.nodes, records):
        assert rec == want[node.node.name], node.node.name
    assert counts == [sum(1 for w in want.values() if w[0] == r) for r in range(ref.REASON_COUNT)]
    return records


def test_abi_names_agree():
    assert [getattr(abi, "DRIFT_" + n) for n in abi.DRIFT_STATUS_NAMES] == list(range(8))
    assert (abi.DRIFT_AMI, abi.DRIFT_CAPACITY_RESERVATION, abi.DRIFT_ERR_NO_SUBNETS) == (ref.AMI, ref.CAPACITY_RESERVATION,
                                                                                      ref.ERR_NO_SUBNETS)
    assert abi.DRIFT_REASON_COUNT == ref.REASON_COUNT and abi.DRIFT_NO_AMI == ref.NO_AMI


def test_reference_suite(lib, catalog):
    records = check(cases.reference_suite(lib, catalog))
    assert {r[1] for r in records} == set(range(8))       # every status
    assert {r[0] for r in records} == set(range(8)) - {ref.NODEPOOL}   # every reason of the provider (tests/precedence: the core's)


def test_precedence(catalog):
    check(cases.precedence(catalog))


def test_requirement_edges(catalog):
    check(cases.requirement_edges(catalog))


@pytest.mark.parametrize("n", [0, 1, 65])
def test_node_counts(catalog, n):
    check(cases.node_counts(catalog, n))


def test_ami_lists(catalog):
    check(cases.ami_lists(catalog))


def test_value_dictionaries(catalog):
    check(cases.value_dictionaries(catalog))


def test_id_sets(catalog):
    check(cases.id_sets(catalog))


@pytest.mark.parametrize("n_pools,n_classes", [(1, 1), (2, 2), (300, 7)])
def test_pools_and_classes(catalog, n_pools, n_classes):
    check(cases.pools_and_classes(catalog, n_pools, n_classes))


def test_generator_ami_map_is_the_oracles(catalog):
    """synth.ami_for_type (what launches the generator's and the end-to-end model's nodes) against the oracle's
    Compatible, over every type of the catalogue and the generator's AMI lists"""
    cl = cases.random_cluster(catalog, 3)
    for nc in cl.drift_inputs.nodeclasses:
        for it in catalog[::7]:
            assert synth.ami_for_type(it, nc.amis) == ref.ami_for_type(it, nc.amis), (it.name, [a.id for a in nc.amis])


def test_random_clusters_reach_everything(catalog):
    """A condition, not a measurement: the randomized clusters of the GPU half reach every reason and every status,
    and at least a quarter of their nodes are judged and not drifted."""
    reasons, statuses, clean, total = set(), set(), 0, 0
    for seed in range(6):
        cl = cases.random_cluster(catalog, seed)
        records, counts = ref.detect(cl)
        assert sum(counts) == len(cl.nodes) == 120
        reasons |= {r[0] for r in records}
        statuses |= {r[1] for r in records}
        clean += sum(1 for r in records if r[:2] == (ref.NONE, ref.OK))
        total += len(records)
    assert reasons == set(range(8)) and statuses == set(range(8))
    assert 4 * clean >= total, (clean, total)


class RefPlan:
    """A plan that answers detect_drift from the reference, in the device's record format"""

    def __init__(self, cluster):
        self.cluster = cluster

    def detect_drift(self, inputs=None, records=True):
        recs, counts = ref.detect(self.cluster, inputs)
        out = np.zeros(len(recs), dtype=abi.node_drift_dtype())
        for i, (reason, status, detail) in enumerate(recs):
            out[i] = (reason, status, detail, 0)
        return (out if records else None), counts, {}


def test_drifted_condition_life(catalog):
    """disruption.md:162-164: newly drifted gets now, still drifted keeps its time, no longer drifted loses it, an
    error leaves what was there"""
    cl, _ = cases.node_counts(catalog, 6)           # nodes 2 and 5 AMI-drifted, node 4 subnet-drifted
    plan = RefPlan(cl)
    cl.nodes[0].drifted = 50.0                      # not drifted any more
    cl.nodes[2].drifted = 70.0                      # still drifted
    disruption.detect_drift(cl, plan, 100)
    assert [n.drifted for n in cl.nodes] == [None, None, 70.0, None, 100, 100]
    cl.drift_inputs.nodes[5].instance = None        # an error: the condition is not touched
    cl.drift_inputs.nodes[3].instance = None
    cl.drift_inputs.nodes[4].instance.subnet_id = "subnet-1"
    disruption.detect_drift(cl, plan, 200)
    assert [n.drifted for n in cl.nodes] == [None, None, 70.0, None, None, 100]
    controls = synth.add_disruption_controls(cl, 1)
    controls.nodes[0].drifted, controls.nodes[2].drifted, controls.nodes[5].drifted = 5, None, 100
    disruption.detect_drift(cl, plan, 300)
    assert [c.drifted for c in controls.nodes] == [None, None, 70, None, None, 100]


def test_controller_detects_first(catalog):
    """Controller.compute_command runs detection when the cluster carries DriftInputs, and not otherwise"""
    cl, _ = cases.node_counts(catalog, 3)

    class Plan(RefPlan):
        calls = 0

        def detect_drift(self, *a, **k):
            Plan.calls += 1
            return super().detect_drift(*a, **k)

        def drift(self, subsets, allowed=None):
            raise AssertionError("the drifted node is empty: no simulation")

    cmd = disruption.Controller().compute_command(cl, Plan(cl), now=100)
    assert Plan.calls == 1 and cl.nodes[2].drifted == 100
    assert cmd.method == "emptiness"                # every node of the builder is empty: Emptiness wins first
    inputs, cl.drift_inputs = cl.drift_inputs, None
    disruption.Controller().compute_command(cl, Plan(cl), now=100)
    assert Plan.calls == 1
    cl.drift_inputs = inputs
