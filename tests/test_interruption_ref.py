"""Interruption handling (kp_cluster_interruptions), the CPU half: the plain-Python reference
(tests/interruption_ref.py) and kpamd.interruption.parse held to the reference suite's cases
(R:pkg/controllers/interruption/suite_test.go:129-258) and to the parsers' edges, through kpamd.interruption.Controller
on the reference plan. The message bodies are data (tests/golden/interruption_messages.json, written to the EventBridge
schemas); the device is held to the same reference in tests/test_gpu_interruption.py."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import interruption_cases as cases  # noqa: E402
import interruption_ref as ref  # noqa: E402
from kpamd import abi, interruption  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interruption_messages.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    return g["placeholder_instance_id"], {m["name"]: m for m in g["messages"]}


class FakeCatalog:
    """Catalog.update_offerings without a device: the records it was handed, applied to the instance types"""

    def __init__(self, instance_types):
        import copy
        self.instance_types = copy.deepcopy(instance_types)
        self.calls = []

    def update_offerings(self, updates, seqnum):
        self.calls.append((list(updates), seqnum))
        for t, ct, zone, avail in updates:
            for o in self.instance_types[t].offerings:
                if o.capacity_type == ct and o.zone == zone:
                    o.available = avail


def body(golden, name, instance_id):
    placeholder, msgs = golden
    return msgs[name]["body"].replace(placeholder, instance_id)


def reconcile(built, bodies, catalogs=None):
    cl = built[0]
    cats = [FakeCatalog(c) for c in cl.catalogs] if catalogs is None else catalogs
    out = interruption.Controller().reconcile(bodies, cl, ref.RefPlan(cl), cats, seqnum=2)
    return out, cats


def test_the_kind_values_are_the_abi_s():
    assert tuple(abi.MESSAGE_KIND_NAMES) == ref.KIND_NAMES
    assert (abi.MSG_NO_OP, abi.MSG_REBALANCE_RECOMMENDATION, abi.MSG_SCHEDULED_CHANGE, abi.MSG_SPOT_INTERRUPTED,
            abi.MSG_INSTANCE_STOPPED, abi.MSG_INSTANCE_TERMINATED) == (ref.NO_OP, ref.REBALANCE, ref.SCHEDULED_CHANGE,
                                                                       ref.SPOT, ref.STOPPED, ref.TERMINATED)
    assert (abi.INTERRUPT_DELETE, abi.INTERRUPT_ALREADY_DELETING, abi.INTERRUPT_ICE) == (ref.DELETE, ref.ALREADY_DELETING, ref.ICE)


def test_every_golden_body_parses_as_recorded(golden):
    _, msgs = golden
    assert len(msgs) >= 30
    for name, m in msgs.items():
        if m.get("error"):
            with pytest.raises(interruption.ParseError):
                interruption.parse(m["body"])
        else:
            kind, ids = interruption.parse(m["body"])
            assert (abi.MESSAGE_KIND_NAMES[kind], ids) == (m["kind"], m["ids"]), name


def test_parser_edges(golden):
    _, msgs = golden
    kind = lambda name: abi.MESSAGE_KIND_NAMES[interruption.parse(msgs[name]["body"])[0]]
    assert kind("empty_body") == "no_op"                                   # parser.go:75-77
    assert kind("unknown_detail_type") == kind("unknown_source") == kind("unknown_version") == "no_op"   # :92
    assert kind("state_change_creating") == "no_op"                        # statechange/parser.go:38
    assert kind("state_change_STOPPED_upper_case") == "instance_terminated"  # accepted lower-cased, Kind() as written
    assert kind("state_change_stopped") == "instance_stopped"
    assert kind("scheduled_change_other_service") == kind("scheduled_change_other_category") == "no_op"
    assert kind("scheduled_change_service_lower_case") == "no_op"          # the filter compares as written
    assert interruption.parse(msgs["scheduled_change_same_entity_twice"]["body"])[1] == [golden[0]] * 2
    assert kind("unknown_fields_only") == "no_op"                          # valid JSON of no known key (suite :218-232)


def test_instance_id_is_the_last_path_segment():
    assert interruption.instance_id("aws:///test-zone-1a/i-0123456789abcdef0") == "i-0123456789abcdef0"
    assert interruption.instance_id("aws:///a/b/i-1") == "i-1"
    assert interruption.instance_id("aws:///zone/") == ""
    assert interruption.instance_id("i-0123456789abcdef0") is None
    assert interruption.instance_id("") is None and interruption.instance_id(None) is None


# ---- R:pkg/controllers/interruption/suite_test.go:129-258 ----------------------------------------------------------
def test_a_spot_interruption_deletes_the_nodeclaim(catalog, golden):
    built = cases.reference_suite_node(catalog).build("suite-129", None)
    out, _ = reconcile(built, [body(golden, "spot_interruption", built[1][0])])
    assert out.deletes == [(0, 0, ref.SPOT)]
    assert out.disrupted == {("spot_interrupted", "default", "spot"): 1}
    assert out.received["spot_interrupted"] == 1 and out.parse_errors == 0


def test_a_scheduled_change_deletes_the_nodeclaim(catalog, golden):
    built = cases.reference_suite_node(catalog).build("suite-142", None)
    out, _ = reconcile(built, [body(golden, "scheduled_change", built[1][0])])
    assert out.deletes == [(0, 0, ref.SCHEDULED_CHANGE)]
    assert out.disrupted == {("scheduled_change", "default", "spot"): 1}
    assert out.marks == []                                                 # only a spot interruption marks


def test_the_four_state_changes_delete_their_nodeclaims(catalog, golden):
    b = cases.Build([cases.types_named(catalog)])
    states = ["terminated", "stopped", "stopping", "shutting-down"]
    for i, _ in enumerate(states):
        b.node(cases.iid(0x50 + i))
    built = b.build("suite-155", None)
    out, _ = reconcile(built, [body(golden, "state_change_" + s, built[1][i]) for i, s in enumerate(states)])
    assert [d[0] for d in out.deletes] == [0, 1, 2, 3]
    assert out.disrupted == {("instance_terminated", "default", "spot"): 2, ("instance_stopped", "default", "spot"): 2}


def test_a_hundred_spot_messages_delete_a_hundred_nodeclaims(catalog, golden):
    b = cases.Build([cases.types_named(catalog)])
    for i in range(100):
        b.node(cases.iid(0x1000 + i))
    built = b.build("suite-188", None)
    out, _ = reconcile(built, [body(golden, "spot_interruption", x) for x in built[1]])
    assert [d[0] for d in out.deletes] == list(range(100)) and [d[1] for d in out.deletes] == list(range(100))
    assert out.received["spot_interrupted"] == 100


def test_a_body_that_cannot_be_parsed_deletes_no_nodeclaim(catalog, golden):
    built = cases.reference_suite_node(catalog).build("suite-218", None)
    _, msgs = golden
    out, _ = reconcile(built, [msgs["unknown_fields_only"]["body"], msgs["malformed_json"]["body"], None,
                               msgs["not_json"]["body"]])
    assert out.deletes == [] and out.marks == [] and out.updates == {}
    assert out.parse_errors == 3 and out.received["no_op"] == 1          # every one of the four is deleted from the queue
    assert out.nodes == [{"first_message": -1, "kinds": 0, "n_messages": 0, "flags": 0}]


def test_a_state_outside_the_accepted_states_is_a_no_op(catalog, golden):
    built = cases.reference_suite_node(catalog).build("suite-233", None)
    out, _ = reconcile(built, [body(golden, "state_change_creating", built[1][0])])
    assert out.deletes == [] and out.received == dict({n: 0 for n in ref.KIND_NAMES}, no_op=1)


def test_a_spot_interruption_marks_the_offering(catalog, golden):
    built = cases.reference_suite_node(catalog, labels={ref.ZONE: "coretest-zone-1a"}).build("suite-242", None)
    out, cats = reconcile(built, [body(golden, "spot_interruption", built[1][0])])
    assert out.marks == [("t3.large", "coretest-zone-1a", 1)]              # exactly that mark
    assert out.deletes == [(0, 0, ref.SPOT)]
    assert out.updates == {} and cats[0].calls == []                       # no catalogue has an offering in that zone


# ---- the marks as offering updates -----------------------------------------------------------------------------------
def test_marks_become_updates_where_the_catalogue_has_the_spot_offering(catalog):
    cl, ids, msgs, _ = cases.ice_marks(catalog)
    want = ref.resolve(cl, msgs, ids)
    plan = ref.RefPlan(cl)
    cats = [FakeCatalog(c) for c in cl.catalogs]
    got = plan.interruptions(msgs, ids)
    assert got == want
    labels = lambda n: cl.nodes[n].node.labels
    marks = [(labels(m["node"])[ref.ITYPE], labels(m["node"])[ref.ZONE], m["n_nodes"]) for m in want["marks"]]
    z = cases.ZONES
    assert marks == [("m5.large", z[0], 2), ("m5.2xlarge", z[1], 1), ("t3.large", z[1], 70), ("c5.large", z[0], 1),
                     ("m5.large ", z[0], 1)]
    # the deleting node 0 carries its mark and is not deleted; the on-demand node 1 is both marked and deleted
    assert want["nodes"][0]["flags"] == ref.ALREADY_DELETING | ref.ICE
    assert want["nodes"][1]["flags"] == ref.DELETE | ref.ICE
    assert [want["nodes"][n]["flags"] for n in (2, 3, 4, 5)] == [ref.DELETE] * 4   # a label missing or empty: no mark
    assert want["nodes"][6] == {"first_message": -1, "kinds": 0, "n_messages": 0, "flags": 0}   # no id
    ups0 = interruption.mark_updates(cats[0].instance_types, [m[:2] for m in marks])
    ups1 = interruption.mark_updates(cats[1].instance_types, [m[:2] for m in marks])
    name = lambda cat, ups: [(cat.instance_types[t].name, ct, zone, a) for t, ct, zone, a in ups]
    assert name(cats[0], ups0) == [("m5.large", "spot", z[0], False), ("m5.2xlarge", "spot", z[1], False),
                                   ("t3.large", "spot", z[1], False), ("c5.large", "spot", z[0], False)]
    assert name(cats[1], ups1) == [("m5.large", "spot", z[0], False), ("c5.large", "spot", z[0], False)]


def test_reconcile_updates_every_catalogue_once(catalog, golden):
    cl, ids, msgs, _ = cases.ice_marks(catalog)
    bodies = [body(golden, "spot_interruption" if k == ref.SPOT else "state_change_stopped", i[0]) for k, i in msgs]
    out, cats = reconcile((cl, ids, msgs, 0), bodies)
    want = ref.resolve(cl, msgs, ids)
    assert out.nodes == want["nodes"] and out.matches == want["matches"]
    assert [len(c.calls) for c in cats] == [1, 1] and {c.calls[0][1] for c in cats} == {2}
    for c, cat in enumerate(cats):
        for t, ct, zone, _ in out.updates[c]:
            assert not any(o.available for o in cat.instance_types[t].offerings if o.capacity_type == ct and o.zone == zone)
    assert sum(out.disrupted.values()) == len(out.deletes) == len(want["deletes"])


# ---- the reference against hand-written expectations at the rule's edges ------------------------------------------
def test_first_message_skips_the_rebalance_message(catalog):
    cl, ids, msgs, _ = cases.kind_orders(catalog)
    got = ref.resolve(cl, msgs, ids)
    bits = (1 << ref.REBALANCE) | (1 << ref.SPOT) | (1 << ref.TERMINATED)
    for o in range(6):
        acting = [m for m in range(3 * o, 3 * o + 3) if msgs[m][0] != ref.REBALANCE]
        assert got["nodes"][o] == {"first_message": acting[0], "kinds": bits, "n_messages": 3, "flags": ref.DELETE | ref.ICE}
    assert got["nodes"][6] == {"first_message": -1, "kinds": 1 << ref.REBALANCE, "n_messages": 2, "flags": 0}
    assert got["nodes"][7] == {"first_message": -1, "kinds": 0, "n_messages": 0, "flags": 0}   # named by a no_op only
    assert got["matches"][18:] == [1, 0, 0, 1]
    assert [d["node"] for d in got["deletes"]] == list(range(6))


def test_shared_ids_and_repeated_ids(catalog):
    cl, ids, msgs, _ = cases.shared_id(catalog, 3)
    got = ref.resolve(cl, msgs, ids)
    assert got["matches"] == [3, 3, 1, 0, 3, 1]
    assert [got["nodes"][n]["first_message"] for n in range(6)] == [-1, 1, 1, 1, 2, 3]
    assert [got["nodes"][n]["flags"] & 3 for n in range(6)] == [0, ref.DELETE, ref.ALREADY_DELETING, ref.DELETE,
                                                               ref.DELETE, ref.ALREADY_DELETING]
    assert got["counts"] == [0, 0, 0, 2, 0, 1]
    cl, ids, msgs, _ = cases.scheduled_changes(catalog)
    got = ref.resolve(cl, msgs, ids)
    assert got["matches"] == [1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 0]
    assert got["nodes"][4] == {"first_message": 3, "kinds": 1 << ref.SCHEDULED_CHANGE, "n_messages": 3, "flags": ref.DELETE}


def test_only_notifications_delete_nothing(catalog):
    cl, ids, msgs, _ = cases.only_notifications(catalog)
    got = ref.resolve(cl, msgs, ids)
    assert got["deletes"] == [] and got["marks"] == [] and got["counts"] == [0] * 6
    assert got["matches"] == [1, 0, 1]


@pytest.mark.parametrize("pattern,deletes,marks", [("all", 257, 241), ("none", 0, 0), ("alternate", 129, 15)])
def test_compaction_cases(catalog, pattern, deletes, marks):
    cl, ids, msgs, _ = cases.compaction(catalog, 257, pattern)
    got = ref.resolve(cl, msgs, ids)
    assert (len(got["deletes"]), len(got["marks"])) == (deletes, marks)
    # all: the first 17 nodes share a pair, each of the other 240 has its own; alternate: 5 types x 3 zones
    assert [m["node"] for m in got["marks"]] == sorted(m["node"] for m in got["marks"])
    if pattern == "all":
        assert got["marks"][0] == {"node": 0, "n_nodes": 17} and got["marks"][-1] == {"node": 256, "n_nodes": 1}


def test_the_storm_mix(catalog):
    cl, ids, msgs, _ = cases.storm(catalog, 100)
    got = ref.resolve(cl, msgs, ids)
    assert len(got["deletes"]) == 100 and got["counts"] == [0, 0, 34, 33, 16, 17]
    assert sum(m["n_nodes"] for m in got["marks"]) == 33
