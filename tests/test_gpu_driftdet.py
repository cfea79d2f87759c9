"""Drift detection on the device (kp_cluster_detect_drift) against the plain-Python reference
(tests/driftdet_ref.py) with == on every field of every record and on the histogram, at the smallest shapes where the
kernels can go wrong (tests/driftdet_cases.py; tests/test_driftdet.py holds the reference to the same cases on the
CPU)."""
import copy
import ctypes as C
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import driftdet_cases as cases  # noqa: E402
import driftdet_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


@contextmanager
def planned(ctx, cl):
    """ClusterPlan of cl with catalogues of its own, all closed at the end"""
    import kpamd
    plan = kpamd.ClusterPlan(ctx, cl)
    try:
        yield plan
    finally:
        plan.close()
        for c in plan.catalogs:
            c.close()


def compare(plan, cl, inputs=None):
    want, want_counts = ref.detect(cl, inputs)
    got, counts, stats = plan.detect_drift(inputs)
    assert len(got) == len(want) == len(cl.nodes)
    for i, w in enumerate(want):
        g = (int(got[i]["reason"]), int(got[i]["status"]), int(got[i]["detail"]))
        assert g == w and int(got[i]["r"]) == 0, (cl.name, cl.nodes[i].node.name, g, w)
    assert counts == want_counts, cl.name
    none, only_counts, _ = plan.detect_drift(inputs, records=False)   # out = NULL: the histogram alone
    assert none is None and only_counts == want_counts
    assert stats["device_ms"] >= 0 and stats["host_ms"] > 0
    return want


def run(ctx, built):
    cl, want = built
    with planned(ctx, cl) as plan:
        records = compare(plan, cl)
    assert records == [want[n.node.name] for n in cl.nodes]   # the hand-written expectations, as on the CPU


def test_reference_suite(ctx, lib, catalog):
    run(ctx, cases.reference_suite(lib, catalog))


def test_precedence(ctx, catalog):
    run(ctx, cases.precedence(catalog))


def test_requirement_edges(ctx, catalog):
    run(ctx, cases.requirement_edges(catalog))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_node_counts(ctx, catalog, n):
    run(ctx, cases.node_counts(catalog, n))


def test_ami_lists(ctx, catalog):
    run(ctx, cases.ami_lists(catalog))


def test_value_dictionaries(ctx, catalog):
    run(ctx, cases.value_dictionaries(catalog))


def test_id_sets(ctx, catalog):
    run(ctx, cases.id_sets(catalog))


@pytest.mark.parametrize("n_pools,n_classes", [(1, 1), (2, 2), (300, 7)])
def test_pools_and_classes(ctx, catalog, n_pools, n_classes):
    run(ctx, cases.pools_and_classes(catalog, n_pools, n_classes))


@pytest.mark.parametrize("seed", range(6))
def test_randomized(ctx, catalog, seed):
    """120 nodes over 12 pools; a pool on a second catalogue, so that nodes are looked up by name and some not found"""
    cl = cases.random_cluster(catalog, seed)
    with planned(ctx, cl) as plan:
        compare(plan, cl)


def test_randomized_2000(ctx, catalog):
    cl = cases.random_cluster(catalog, 11, n_nodes=2000)
    with planned(ctx, cl) as plan:
        compare(plan, cl)


@pytest.mark.parametrize("kind", ["batched", "general"])
def test_both_plan_kinds(ctx, catalog, kind):
    """A plan of the batched simulation kernel and a general-path (spread) plan: detection equals the reference, and
    kp_cluster_simulate on the same plan answers after the call what it answered before it."""
    from kpamd import synth
    cl = synth.config4(catalog, n_nodes=60, seed=5) if kind == "batched" else synth.spread_cluster(catalog, 40, seed=5)
    synth.add_drift_inputs(cl, 9)
    with planned(ctx, cl) as plan:
        subsets = [cl.candidates[:k] for k in (1, 2, 5)] + [[c] for c in cl.candidates[5:9]]
        before, _ = plan.simulate(subsets, multi_node=True)
        compare(plan, cl)
        after, _ = plan.simulate(subsets, multi_node=True)
        assert after == before
        compare(plan, cl)


def test_new_ami_published(ctx, catalog):
    """Two calls on one plan with different nodeclass statuses: the second call's answers follow the new status"""
    from kpamd.model import AMI
    cl, want = cases.node_counts(catalog, 70)
    with planned(ctx, cl) as plan:
        first = compare(plan, cl)
        assert first == [want[n.node.name] for n in cl.nodes]
        inputs = copy.deepcopy(cl.drift_inputs)
        inputs.nodeclasses[0].amis.insert(0, AMI("ami-new", [(cases.ARCH, "In", ["amd64"])]))
        inputs.nodes[0].instance.image_id = "ami-new"
        second = compare(plan, cl, inputs)
        assert first[0] == second[0] == cases.NOT_DRIFTED
        assert second[1:] == [(ref.AMI, ref.OK, 0)] * 69  # every other node now runs an image that is not its type's
        assert compare(plan, cl) == first                 # and back


def _raw(plan, di, n, out=True, counts=True):
    from kpamd import abi
    o = np.zeros(max(n, 1), dtype=abi.node_drift_dtype())
    c = (C.c_uint64 * abi.DRIFT_REASON_COUNT)()
    return plan.ctx.lib.kp_cluster_detect_drift(plan.h, C.byref(di) if di is not None else None,
                                                o.ctypes.data if out else None, c if counts else None, None)


def test_errors(ctx, lib, catalog):
    """Each KP_E_INVAL: counts that differ from the snapshot, NULL arrays with non-zero counts, a nodeclass index out of
    range, an unknown operator, a NULL key or id, out and counts both NULL; then the stale plan."""
    import kpamd
    from kpamd import abi
    cl, _ = cases.precedence(catalog)
    n = len(cl.nodes)

    def fresh(edit=None, **kw):
        arena = abi.Arena()
        di = abi.build_drift_in(arena, cl.drift_inputs)
        for k, v in kw.items():
            setattr(di, k, v)
        if edit:
            edit(arena, di)
        return arena, di

    def bad_op(arena, di):
        di.nodeclasses[0].amis[0].requirements.items[0].op = 6

    def null_key(arena, di):
        di.nodeclasses[0].amis[0].requirements.items[0].key = None

    def null_ami_id(arena, di):
        di.nodeclasses[0].amis[0].id = None

    def null_subnet(arena, di):
        di.nodeclasses[0].subnets[0] = None

    def null_sg(arena, di):
        di.nodeclasses[0].security_groups[0] = None

    def null_image(arena, di):
        di.nodes[0].image_id = None

    def class_high(arena, di):
        di.pools[0].nodeclass = di.n_nodeclasses

    def class_low(arena, di):
        di.pools[0].nodeclass = -2

    with planned(ctx, cl) as plan:
        assert _raw(plan, fresh()[1], n) == abi.KP_OK
        for kw in (dict(n_pools=1), dict(n_nodes=n - 1), dict(n_nodes=0), dict(pools=None), dict(nodes=None),
                   dict(nodeclasses=None)):
            keep, di = fresh(**kw)
            assert _raw(plan, di, n) == abi.KP_E_INVAL, kw
        for edit in (bad_op, null_key, null_ami_id, null_subnet, null_sg, null_image, class_high, class_low):
            keep, di = fresh(edit)
            assert _raw(plan, di, n) == abi.KP_E_INVAL, edit.__name__
        keep, di = fresh()
        assert _raw(plan, di, n, out=False, counts=False) == abi.KP_E_INVAL
        assert _raw(plan, None, n) == abi.KP_E_INVAL
        assert _raw(plan, di, n, out=False) == abi.KP_OK and _raw(plan, di, n, counts=False) == abi.KP_OK
        compare(plan, cl)                                   # the plan serves on after every refusal
    # a stale plan: the catalogue's seqnum moved since kp_cluster_prepare; kp_cluster_refresh brings it back
    cl, _ = cases.node_counts(catalog, 5)
    its = copy.deepcopy(cl.catalogs[0])
    cat = kpamd.Catalog(ctx, its, seqnum=1)
    p = kpamd.ClusterPlan(ctx, cl, catalogs=[cat])
    try:
        compare(p, cl)
        o = next(o for o in its[0].offerings if o.available)
        cat.update_offerings([(0, o.capacity_type, o.zone, False)], seqnum=2)
        with pytest.raises(kpamd.KPError, match="stale plan") as e:
            p.detect_drift()
        assert e.value.code == abi.KP_E_INVAL
        p.refresh()
        compare(p, cl)
    finally:
        p.close()
        cat.close()
