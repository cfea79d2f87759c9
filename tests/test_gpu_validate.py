"""kp_cluster_validate on plans of the batched simulation kernel: the record the checking sim_kernel instantiation leaves
for every (subset, check) equals the expected record of tests/validate_ref.py (the oracle's simulation plus the rule of
include/kp/kp_abi.h), field for field, with no tolerance."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import command_ref  # noqa: E402
import validate_ref as vr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plans(ctx):
    import kpamd
    made = {}

    def get(name):
        if name not in made:
            made[name] = kpamd.ClusterPlan(ctx, vr.cluster_of(name)[0])
        return made[name]
    yield get
    for p in made.values():
        p.close()


def _check(plan, name, order=None):
    """plan.validate on a named input (optionally permuted) against its recorded records."""
    doc = vr.expected(name)
    idx = list(range(len(doc["records"]))) if order is None else [int(i) for i in order]
    got, st = plan.validate([doc["subsets"][i] for i in idx], [doc["checks"][i] for i in idx], allowed=vr.cluster_of(name)[1])
    for g, i in zip(got, idx):
        assert g == doc["records"][i], f"{name} input {i} ({doc['labels'][i]}) subset {doc['subsets'][i]}"
    return got, st, doc


def test_self_validation(plans):
    """Every recorded command of config4 (399 subsets, both multi_node values) is KP_VALID on the plan it came from."""
    got, _, doc = _check(plans("config4"), "config4")
    own = [g for g, lab in zip(got, doc["labels"]) if lab == "self"]
    assert len(own) > 50 and all(g["verdict"] == vr.VALID for g in own)


def test_crafted(plans):
    """The crafted checks on the same plan: a DELETE claimed where the simulation makes a NodeClaim, a REPLACE where it
    makes none, checks on multi-NodeClaim subsets, the truncated list plus one type outside it, the whole truncated
    list (more than 64 options; filterByPrice dropped some of them), a name in no catalogue, duplicate names."""
    got, _, doc = _check(plans("config4"), "config4")
    by = {}
    for g, lab, c in zip(got, doc["labels"], doc["checks"]):
        by.setdefault(lab, []).append((g, c))
    assert all(g["verdict"] == vr.NEEDS_REPLACEMENT for g, _ in by["delete-claimed"])
    assert all(g["verdict"] == vr.NO_REPLACEMENT_NEEDED for g, _ in by["none-replace"])
    assert all(g["verdict"] == vr.MULTIPLE and g["n_nodeclaims"] == 2 for g, _ in by["multi-delete"] + by["multi-replace"])
    assert all(g["verdict"] == vr.VALID for g, _ in by["whole-truncated-list"])
    assert max(len(c["options"]) for _, c in by["whole-truncated-list"]) > 64
    assert all(g["verdict"] == vr.NOT_SUBSET and g["n_missing"] == 1 for g, _ in by["one-outside"] + by["unknown-name"] + by["duplicates"])
    assert all(g["verdict"] == vr.VALID for g, _ in by["last-of-the-list"])


def test_infeasible(plans):
    """Any check on an infeasible subset. With config4's NodePools unlimited no subset of its nodes is infeasible (a
    pod that fits no existing node gets a NodeClaim), so the same nodes and subsets run under remaining cpu limits:
    the one NodeClaim the limits admit takes what it can and the other pods stay unplaced - a non-pending pod with no
    placement next to a NodeClaim: UNSCHEDULED, whatever the check claims."""
    got, _, doc = _check(plans("config4-limits"), "config4-limits")
    bad = [g for g, lab in zip(got, doc["labels"]) if lab in ("infeasible-one-delete", "infeasible-one-replace")]
    assert len(bad) >= 6 and all(g["verdict"] == vr.UNSCHEDULED and g["n_nodeclaims"] == 1 and g["n_unscheduled"] > 0 for g in bad)
    assert {g["verdict"] for g in got} >= {vr.VALID, vr.UNSCHEDULED, vr.NO_REPLACEMENT_NEEDED, vr.MULTIPLE,
                                           vr.NEEDS_REPLACEMENT, vr.NOT_SUBSET}
    # tighter limits: pods that no type is left for fail without a NodeClaim being tried (the kernel's own count of
    # unplaced pods; no second NodeClaim is in sight, so nothing is settled on the host)
    got, _, doc = _check(plans("config4-tight-limits"), "config4-tight-limits")
    bad = [g for g, lab in zip(got, doc["labels"]) if lab in ("infeasible-delete", "infeasible-replace")]
    assert len(bad) >= 6 and all(g["verdict"] == vr.UNSCHEDULED and g["n_nodeclaims"] == 0 and g["n_unscheduled"] > 0 for g in bad)


@pytest.mark.parametrize("name", ["config4", "config4-limits", "config4-tight-limits"])
@pytest.mark.parametrize("slots", [4, 28])
def test_wave_slots(plans, ov, slots, name):
    """sim_slots 4 and 28: one wave checks many commands in a row in its reused state (config4-limits: simulations
    that leave pods unplaced among them); the records of the production grid."""
    ov(sim_slots=slots)
    got, st, _ = _check(plans(name), name)
    n_slots = min(slots, (len(got) + 3) // 4 * 4)
    assert st["phase_cycles"][1] == n_slots and st["phase_cycles"][2] == -(-len(got) // n_slots)
    assert slots != 4 or st["phase_cycles"][2] > 1


def test_order(plans, ov):
    """The batch reversed and shuffled (other waves, other predecessors in a wave's slot)."""
    for name, slots in (("config4", 28), ("config4-limits", 4), ("config4-tight-limits", 4)):
        ov(sim_slots=slots)
        n = len(vr.expected(name)["records"])
        for order in (list(range(n))[::-1], list(np.random.default_rng(9).permutation(n))):
            _check(plans(name), name, order=order)


@pytest.mark.parametrize("kind", ["pods-removed", "pending-added", "node-removed"])
def test_changed_snapshot(plans, kind):
    """Snapshot A's recorded commands on a changed snapshot B (candidates and options carried by name)."""
    got, _, _ = _check(plans(f"config4-{kind}"), f"config4-{kind}")
    assert len(got) >= 40


def test_iced_and_refreshed(ctx):
    """A's own plan after ICE marks on some commands' cheapest options: refused as stale, then kp_cluster_refresh, then
    the records of the oracle on the marked catalogue (NOT_SUBSET where the cheapest option left the list)."""
    import kpamd
    a = command_ref.case("config4")[0]
    cat = kpamd.Catalog(ctx, copy.deepcopy(a.catalogs[0]), seqnum=1)
    plan = kpamd.ClusterPlan(ctx, a, catalogs=[cat])
    try:
        doc = vr.expected("config4-iced")
        before, _ = plan.validate(doc["subsets"], doc["checks"])
        assert all(r["verdict"] == vr.VALID for r in before)
        cat.update_offerings([(t, ct, z, False) for t, ct, z in vr.iced_marks()], seqnum=2)
        with pytest.raises(kpamd.KPError, match="stale plan"):
            plan.validate(doc["subsets"], doc["checks"])
        plan.refresh()
        got, _ = plan.validate(doc["subsets"], doc["checks"])
        assert got == doc["records"]
        assert any(r["verdict"] == vr.NOT_SUBSET for r in got)
    finally:
        plan.close()
        cat.close()


@pytest.mark.parametrize("name", ["disruption-state", "min-values", "min-values-broken", "host-ports"])
def test_cases(plans, name):
    """Pending and deleting-node pods with binding limits, a NodePool with instance-family minValues 40, one whose
    instance-type minValues 101 cannot survive Truncate(100) (the NodeClaim's pods fail: UNSCHEDULED), host ports."""
    got, _, _ = _check(plans(name), name)
    if name == "min-values-broken":
        assert any(r["verdict"] == vr.UNSCHEDULED and r["n_nodeclaims"] == 1 for r in got)


def test_spot_to_spot_gate(ctx, plans):
    """The SpotToSpotConsolidation gate on and off: it must not change a validation verdict."""
    import kpamd
    on, _, _ = _check(plans("spot-to-spot"), "spot-to-spot")
    cl = copy.copy(vr.cluster_of("spot-to-spot")[0])
    assert cl.spot_to_spot
    cl.spot_to_spot = False
    plan = kpamd.ClusterPlan(ctx, cl)
    try:
        off, _, _ = _check(plan, "spot-to-spot")
    finally:
        plan.close()
    assert on == off


def test_budgets(plans):
    """Budgets on the two-pool relabelling: a blocked command is KP_INVALID_BUDGET with blocked 1 and is not
    simulated; n_blocked is their count; unlimited allowances and no budgets give the same records."""
    from kpamd.disruption import UNLIMITED
    got, st, doc = _check(plans("budgets"), "budgets")
    blocked = [g for g in got if g["blocked"]]
    assert 0 < len(blocked) < len(got) and st["budget_blocked"] == len(blocked)
    assert all(g == vr.BLOCKED for g in blocked)
    a = plans("budgets").validate(doc["subsets"], doc["checks"], allowed=[UNLIMITED, UNLIMITED])
    b = plans("budgets").validate(doc["subsets"], doc["checks"])
    assert a[0] == b[0] and a[1]["budget_blocked"] == 0 and not any(g["blocked"] for g in a[0])
    for g, w in zip(b[0], doc["records"]):
        assert w["blocked"] or g == w


def test_errors_and_lifecycle(ctx, plans):
    """The KP_E_INVAL cases, no subsets, a set cancel token with the plan left usable, a subset naming a deleting node,
    a wrong n_allowed."""
    import kpamd
    from kpamd import abi
    plan = plans("config4")
    doc = vr.expected("config4")
    sub = doc["subsets"][0]
    for bad, word in (({"decision": 0}, "decision"), ({"decision": 7}, "decision"),
                      ({"decision": vr.REPLACE, "options": []}, "without options"),
                      ({"decision": vr.REPLACE, "options": ["m5.large", None]}, "null name")):
        with pytest.raises(kpamd.KPError) as e:
            plan.validate([sub, sub], [{"decision": vr.DELETE}, bad])
        assert e.value.code == abi.KP_E_INVAL and word in str(e.value) and "check 1" in str(e.value)
    assert plan.validate([], [])[0] == []
    tok = kpamd.Cancel(ctx)
    try:
        tok.set()
        with pytest.raises(kpamd.KPError) as e:
            plan.validate(doc["subsets"][:40], doc["checks"][:40], cancel=tok)
        assert e.value.code == abi.KP_E_CANCELED
        tok.reset()
        got, _ = plan.validate(doc["subsets"][:40], doc["checks"][:40], cancel=tok)  # the plan stays usable
    finally:
        tok.close()
    assert got == doc["records"][:40]
    ds = vr.cluster_of("disruption-state")[0]
    dsub = vr.expected("disruption-state")["subsets"]
    deleting = next(i for i, n in enumerate(ds.nodes) if n.deleting)
    with pytest.raises(kpamd.KPError) as e:
        plans("disruption-state").validate([dsub[0], [dsub[1][0], deleting]], [{"decision": vr.DELETE}] * 2)
    assert e.value.code == abi.KP_E_INVAL and "subset 1" in str(e.value) and "deleted" in str(e.value)
    with pytest.raises(kpamd.KPError) as e:
        plans("budgets").validate([vr.expected("budgets")["subsets"][0]], [{"decision": vr.DELETE}], allowed=[1])
    assert e.value.code == abi.KP_E_INVAL
