"""kp_cluster_interruptions on the device against the plain-Python reference (tests/interruption_ref.py)
with == on every field of every output, at the smallest shapes where the kernels can go wrong
(tests/interruption_cases.py; tests/test_interruption_ref.py holds the reference to the same cases on the CPU): block
and wave edges of the node and entry counts, shared ids, forced tables whose probe runs are long or wrap the table end,
and both compactions with all, none and every other node emitting."""
import copy
import ctypes as C
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import interruption_cases as cases  # noqa: E402
import interruption_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


@contextmanager
def planned(ctx, cl, catalogs=None):
    """ClusterPlan of cl; the plan and the catalogues it made itself are closed at the end"""
    import kpamd
    plan = kpamd.ClusterPlan(ctx, cl, catalogs=catalogs)
    try:
        yield plan
    finally:
        plan.close()
        if catalogs is None:
            for c in plan.catalogs:
                c.close()


def compare(plan, built, want=None):
    """One call: every output field equals the reference's. Returns (the reference's dict, the raw arrays' bytes)."""
    cl, ids, msgs, log2 = built
    want = ref.resolve(cl, msgs, ids) if want is None else want
    got = plan.interruptions(msgs, ids, table_log2=log2)
    for key in ("nodes", "matches", "deletes", "marks", "counts"):
        assert got[key] == want[key], (cl.name, key)
    assert got["stats"]["device_ms"] >= 0 and got["stats"]["host_ms"] > 0
    raw = plan.interruptions(msgs, ids, table_log2=log2, raw=True)
    assert all(int(r["reserved"]) == 0 for r in raw["deletes"])
    return want, b"".join(raw[k].tobytes() for k in ("nodes", "matches", "deletes", "marks"))


def run(ctx, built):
    """The first call, a second call on the same plan, and a call after refresh: equal to the reference, equal bytes"""
    with planned(ctx, built[0]) as plan:
        want, first = compare(plan, built)
        _, second = compare(plan, built, want)
        plan.refresh()
        _, third = compare(plan, built, want)
    assert first == second == third, built[0].name
    return want


@pytest.mark.parametrize("n_nodes", [0, 1, 63, 64, 65, 257, 1025])
def test_node_counts(ctx, catalog, n_nodes):
    run(ctx, cases.sized(catalog, n_nodes, 65))


@pytest.mark.parametrize("n_messages", [0, 1, 64, 65, 257])
def test_message_counts(ctx, catalog, n_messages):
    run(ctx, cases.sized(catalog, 65, n_messages))


@pytest.mark.parametrize("copies", [2, 3])
def test_nodes_sharing_one_id(ctx, catalog, copies):
    want = run(ctx, cases.shared_id(catalog, copies))
    assert want["matches"][0] == want["matches"][1] == copies


@pytest.mark.parametrize("copies,home", [(2, 3), (3, 3), (3, 2), (3, 0), (1, 1)])
def test_the_smallest_forced_table_and_a_run_that_wraps(ctx, catalog, copies, home):
    """copies nodes of one id alone in a table of the least legal size, the run starting at slot home: from the last
    slot it wraps the table end, and the one empty slot is all that ends a probe"""
    built = cases.smallest_table(catalog, copies, home)
    assert (1 << built[3]) > copies >= (1 << built[3]) // 2
    want = run(ctx, built)
    assert want["matches"] == [copies, 0, copies, copies]


@pytest.mark.parametrize("copies", [2, 3])
def test_shared_ids_in_a_forced_table_among_other_nodes(ctx, catalog, copies):
    run(ctx, cases.shared_id(catalog, copies, home=7, slots_log2=3))


@pytest.mark.parametrize("n_nodes,quarter", [(255, False), (255, True), (1023, False)])
def test_forced_tables_full_and_at_a_quarter_load(ctx, catalog, n_nodes, quarter):
    """Every slot but one taken (probe runs as long as the table allows) and a table at a quarter load"""
    run(ctx, cases.forced_load(catalog, n_nodes, quarter))


def test_scheduled_changes(ctx, catalog):
    run(ctx, cases.scheduled_changes(catalog))


def test_long_and_close_ids(ctx, catalog):
    want = run(ctx, cases.long_and_close_ids(catalog))
    assert want["matches"] == [1, 1, 1, 1, 0, 1, 1]


def test_kind_orders(ctx, catalog):
    want = run(ctx, cases.kind_orders(catalog))
    assert all(cases.kind_orders(catalog)[2][n["first_message"]][0] != ref.REBALANCE for n in want["nodes"][:6])


def test_only_notifications(ctx, catalog):
    want = run(ctx, cases.only_notifications(catalog))
    assert want["deletes"] == []


def test_ice_marks(ctx, catalog):
    want = run(ctx, cases.ice_marks(catalog))
    assert [m["n_nodes"] for m in want["marks"]] == [2, 1, 70, 1, 1]


@pytest.mark.parametrize("n_nodes", [255, 256, 257])
@pytest.mark.parametrize("pattern", ["all", "none", "alternate"])
def test_compaction(ctx, catalog, n_nodes, pattern):
    want = run(ctx, cases.compaction(catalog, n_nodes, pattern))
    assert len(want["deletes"]) == {"all": n_nodes, "none": 0, "alternate": (n_nodes + 1) // 2}[pattern]


def test_the_storm_mix(ctx, catalog):
    run(ctx, cases.storm(catalog, 300))


def test_a_general_path_plan(ctx, catalog):
    """A general-path (spread) plan serves the call as a plan of the batched kernel does, and simulates on as before"""
    from kpamd import synth
    cl = synth.spread_cluster(catalog, 40, seed=5)
    ids = [cases.iid(0x700 + i) for i in range(len(cl.nodes))]
    msgs = [(ref.SPOT, [ids[3]]), (ref.SCHEDULED_CHANGE, [ids[5], ids[3], cases.iid(1)]), (ref.STOPPED, [ids[39]])]
    with planned(ctx, cl) as plan:
        subsets = [[c] for c in cl.candidates[:4]]
        before, _ = plan.simulate(subsets, multi_node=True)
        compare(plan, (cl, ids, msgs, 0))
        after, _ = plan.simulate(subsets, multi_node=True)
        assert after == before


def test_two_batches_on_one_plan(ctx, catalog):
    """A second batch on the plan, smaller and with other ids: nothing of the first call is left in the answer"""
    big = cases.sized(catalog, 257, 257)
    cl, ids, _, _ = big
    with planned(ctx, cl) as plan:
        compare(plan, big)
        compare(plan, (cl, ids, [(ref.TERMINATED, [ids[200]])], 0))
        compare(plan, (cl, [None] * len(ids), big[2], 0))
        compare(plan, big)


def _raw(plan, ii, n, **null):
    from kpamd import abi
    nodes = np.zeros(max(n, 1), dtype=abi.interrupt_node_dtype())
    matches = np.zeros(max(int(ii.n_ids), 1) if ii is not None else 1, dtype=np.uint32)
    deletes = np.zeros(max(n, 1), dtype=abi.interrupt_delete_dtype())
    marks = np.zeros(max(n, 1), dtype=abi.interrupt_mark_dtype())
    nd, nm = C.c_uint32(7), C.c_uint32(7)
    rc = plan.ctx.lib.kp_cluster_interruptions(
        plan.h, C.byref(ii) if ii is not None else None, None if null.get("nodes") else nodes.ctypes.data,
        None if null.get("matches") else matches.ctypes.data, None if null.get("deletes") else deletes.ctypes.data,
        None if null.get("n_deletes") else C.byref(nd), None if null.get("marks") else marks.ctypes.data,
        None if null.get("n_marks") else C.byref(nm), None, None)
    return rc, nd.value, nm.value


def test_errors(ctx, catalog):
    """What needs the plan: a node count that differs from the snapshot's, NULL counts, then every refusal of the
    validate entry through the call, and the stale plan. The plan serves on after every refusal."""
    import kpamd
    from kpamd import abi
    built = cases.shared_id(catalog, 3)
    cl, ids, msgs, _ = built
    n = len(ids)

    def fresh(**kw):
        arena = abi.Arena()
        ii = abi.build_interrupt_in(arena, msgs, ids, kw.pop("table_log2", 0))
        for k, v in kw.items():
            setattr(ii, k, v)
        return arena, ii

    with planned(ctx, cl) as plan:
        keep, ii = fresh()
        assert _raw(plan, ii, n) == (abi.KP_OK, 3, 3)
        assert _raw(plan, ii, n, nodes=True, matches=True, deletes=True, marks=True) == (abi.KP_OK, 3, 3)
        assert _raw(plan, ii, n, n_deletes=True)[0] == abi.KP_E_INVAL
        assert _raw(plan, ii, n, n_marks=True)[0] == abi.KP_E_INVAL
        assert _raw(plan, None, n) == (abi.KP_E_INVAL, 0, 0)
        for kw in (dict(n_nodes=n - 1), dict(n_nodes=0), dict(kinds=None), dict(ids=None), dict(node_ids=None),
                   dict(id_offsets=None), dict(n_ids=int(ii.n_ids) - 1), dict(table_log2=2), dict(table_log2=31)):
            keep, bad = fresh(**kw)
            assert _raw(plan, bad, n) == (abi.KP_E_INVAL, 0, 0), kw
        keep, bad = fresh()
        bad.kinds[0] = 6
        assert _raw(plan, bad, n)[0] == abi.KP_E_INVAL
        keep, bad = fresh()
        bad.ids[0] = None
        assert _raw(plan, bad, n)[0] == abi.KP_E_INVAL
        keep, bad = fresh(n_messages=1 << 31)
        assert _raw(plan, bad, n)[0] == abi.KP_E_UNSUPPORTED
        with pytest.raises(kpamd.KPError) as e:
            plan.interruptions([(ref.SPOT, ["i-" + "0" * 30])], ids)
        assert e.value.code == abi.KP_E_UNSUPPORTED
        compare(plan, built)
    # a stale plan: the catalogue's seqnum moved since kp_cluster_prepare; kp_cluster_refresh brings it back
    its = copy.deepcopy(cl.catalogs[0])
    cat = kpamd.Catalog(ctx, its, seqnum=1)
    with planned(ctx, cl, catalogs=[cat]) as p:
        try:
            compare(p, built)
            o = next(o for o in its[0].offerings if o.available)
            cat.update_offerings([(0, o.capacity_type, o.zone, False)], seqnum=2)
            with pytest.raises(kpamd.KPError, match="stale plan") as e:
                p.interruptions(msgs, ids)
            assert e.value.code == abi.KP_E_INVAL
            p.refresh()
            compare(p, built)
        finally:
            p.close()
            cat.close()
