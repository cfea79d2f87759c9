"""tests/validate_ref.py held to itself on the CPU: every recorded file under tests/golden/validate_*.json.gz equals the
recomputation (inputs and expected records, from the oracle), and the inputs reach what the GPU tests lean on."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import command_ref  # noqa: E402
import validate_ref as vr  # noqa: E402


@pytest.mark.parametrize("name", vr.ALL)
def test_recorded_equals_recomputed(name):
    assert vr._doc(name) == vr.expected(name)


def _all():
    for name in vr.ALL:
        doc = vr.expected(name)
        for i, rec in enumerate(doc["records"]):
            yield name, doc["subsets"][i], doc["checks"][i], doc["labels"][i], rec


def test_inputs_reach_every_verdict():
    seen = {rec["verdict"] for *_, rec in _all()}
    assert seen == set(range(7)), seen
    # on plans of the batched kernel and on general-path plans alike (BUDGET is the host's on both: batched only)
    for group in (vr.BATCHED + tuple(f"config4-{k}" for k in vr.CHANGED), vr.GENERAL):
        seen = {rec["verdict"] for name, *_, rec in _all() if name in group}
        assert seen >= {vr.VALID, vr.UNSCHEDULED, vr.NO_REPLACEMENT_NEEDED, vr.MULTIPLE, vr.NEEDS_REPLACEMENT, vr.NOT_SUBSET}, (group, seen)


def test_inputs_reach_the_edges():
    """A NOT_SUBSET with one missing type of index >= 64; a check with more than 64 options; a check with exactly the
    truncated list, longer than what the price filters kept of it; a NodeClaim whose truncated options break minValues."""
    cl = vr.cluster_of("config4")[0]
    index = {it.name: t for t, it in enumerate(cl.catalogs[0])}
    doc = vr.expected("config4")
    rows = list(zip(doc["subsets"], doc["checks"], doc["labels"], doc["records"]))
    one = [(c, r) for _, c, lab, r in rows if lab == "one-outside"]
    assert one and all(r["verdict"] == vr.NOT_SUBSET and r["n_missing"] == 1 and index[c["options"][-1]] >= 64 for c, r in one)
    whole = [(s, c, r) for s, c, lab, r in rows if lab == "whole-truncated-list"]
    assert whole and all(r["verdict"] == vr.VALID for _, _, r in whole)
    assert any(len(c["options"]) > 64 for _, c, _ in whole)
    kept = {}
    for mn in (False, True):
        _, cmds, _ = command_ref.expected("config4", mn)
        for s, c in zip(command_ref.case("config4")[1], cmds):
            if c and c["nodeclaims"]:
                kept.setdefault(tuple(s), []).append(len(c["nodeclaims"][0]["options"]))
    dropped = [(s, c) for s, c, _ in whole if tuple(s) in kept and min(kept[tuple(s)]) < len(c["options"])]
    assert dropped, "no whole-list check on a subset whose command lost options to filterByPrice"
    broken = [r for r in vr.expected("min-values-broken")["records"] if r["verdict"] == vr.UNSCHEDULED]
    assert broken and all(r["n_nodeclaims"] == 1 and r["n_unscheduled"] > 0 for r in broken)
    # the same subsets without the minValues 101 requirement make that NodeClaim and schedule everything
    plain = {tuple(s): r for s, r in zip(vr.expected("min-values")["subsets"], vr.expected("min-values")["records"])}
    subs = vr.expected("min-values-broken")["subsets"]
    both = [plain[tuple(s)] for s, r in zip(subs, vr.expected("min-values-broken")["records"])
            if r["verdict"] == vr.UNSCHEDULED and tuple(s) in plain]
    assert both and all(r["n_unscheduled"] == 0 and r["n_nodeclaims"] == 1 for r in both)


def test_inputs_reach_an_unplaced_pod():
    """An infeasible subset on config4's nodes: a non-pending pod with placement -1 (not the uninitialized-node rule,
    not minValues), next to the one NodeClaim the NodePools' limits admit. config4 itself, with unlimited NodePools,
    has no such subset: a pod that fits no existing node always gets a NodeClaim."""
    from drift_ref import PENDING
    import drift_ref
    doc = vr.expected("config4-limits")
    cl = vr.cluster_of("config4-limits")[0]
    rows = [(s, r) for s, lab, r in zip(doc["subsets"], doc["labels"], doc["records"]) if lab.startswith("infeasible-one")]
    assert len(rows) >= 6
    for s, r in rows:
        assert r["verdict"] == vr.UNSCHEDULED and r["n_nodeclaims"] == 1 and r["n_unscheduled"] > 0
        verdict, solve = vr._simulate(cl, s, vr._SOLVES.setdefault("config4-limits", {}))
        _, kind, _, _ = drift_ref.simulation_problem(cl, s)
        unplaced = [p for p, pl in enumerate(solve["placement"]) if int(pl) == -1 and kind[p] != PENDING]
        assert len(unplaced) == r["n_unscheduled"] and len(solve["nodeclaims"]) == 1 and solve["nodeclaims"][0]["options"]
    assert not any(r["verdict"] == vr.UNSCHEDULED for r in vr.expected("config4")["records"])
    # and without any NodeClaim, under limits that leave no type for the pod
    tight = vr.expected("config4-tight-limits")
    none = [r for lab, r in zip(tight["labels"], tight["records"]) if lab in ("infeasible-delete", "infeasible-replace")]
    assert len(none) >= 6 and all(r["verdict"] == vr.UNSCHEDULED and r["n_nodeclaims"] == 0 and r["n_unscheduled"] > 0 for r in none)


def test_changed_snapshots_change_verdicts():
    """Every carried command is VALID on the snapshot it came from; each change but the index shift turns some of them
    invalid, and the index shift none."""
    for kind in vr.CHANGED:
        recs = vr.expected(f"config4-{kind}")["records"]
        bad = [r for r in recs if r["verdict"] != vr.VALID]
        assert (not bad) if kind == "node-removed" else bad, kind
    assert any(r["verdict"] == vr.NOT_SUBSET for r in vr.expected("config4-iced")["records"])


def test_oracle_plan_validates_its_own_commands():
    """OracleValidatePlan: every command it returns is KP_VALID on its own cluster."""
    cl, subs, _, _ = command_ref.case("reservations")
    plan = vr.OracleValidatePlan(cl)
    _, cmds, _ = plan.command(subs, multi_node=True)
    pairs = [(s, vr.check_of(cl, c)) for s, c in zip(subs, cmds) if c is not None]
    recs, _ = plan.validate([s for s, _ in pairs], [c for _, c in pairs])
    assert pairs and all(r["verdict"] == vr.VALID for r in recs)
