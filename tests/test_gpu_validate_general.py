"""kp_cluster_validate on general-path plans: validate_verdict_kernel behind the batched launches' solve_kernel and
finalize_kernel (and the host's verdict for subsets compiled on their own) against the expected records of
tests/validate_ref.py, field for field."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

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


def _check(plan, name, idx=None):
    doc = vr.expected(name)
    idx = list(range(len(doc["records"]))) if idx is None else idx
    got, st = plan.validate([doc["subsets"][i] for i in idx], [doc["checks"][i] for i in idx])
    for g, i in zip(got, idx):
        assert g == doc["records"][i], f"{name} input {i} ({doc['labels'][i]}) subset {doc['subsets'][i]}"
    return got, st


def test_one_launch(plans):
    """The 120-node spread cluster: every input batched, one launch."""
    got, st = _check(plans("spread"), "spread")
    assert st["phase_cycles"][:3] == [len(got), 0, 1]
    assert {g["verdict"] for g in got} >= {vr.VALID, vr.MULTIPLE, vr.NEEDS_REPLACEMENT, vr.NOT_SUBSET}


def test_nine_launches_on_reused_arenas(plans, ov):
    """63 inputs, 7 per launch: each of the two slots' arenas is reused four times; the list reversed gives every
    simulation another arena and other predecessors in it. The records of the single launch."""
    n = len(vr.expected("spread")["records"])
    idx = [i % n for i in range(63)]
    ov(general_launch=7)
    for order in (idx, idx[::-1]):
        _, st = _check(plans("spread"), "spread", order)
        assert st["phase_cycles"][:3] == [63, 0, 9]


def test_batched_next_to_compiled_alone(plans):
    """Anti-affinity: the subsets that remove every owner of an inverse anti-affinity term are compiled on their own
    and take the host's verdict, the others the device's, in one call."""
    got, st = _check(plans("anti-affinity"), "anti-affinity")
    assert st["phase_cycles"][0] > 0 and st["phase_cycles"][1] > 0
    assert st["phase_cycles"][0] + st["phase_cycles"][1] == len(got)


def test_every_subset_compiled_alone(plans, ov):
    """kp_overrides.general_batch = 1: the host's verdict for every input."""
    ov(general_batch=1)
    got, st = _check(plans("spread"), "spread")
    assert st["phase_cycles"][:2] == [0, len(got)]


def test_reservations(plans):
    _check(plans("reservations"), "reservations")


@pytest.mark.parametrize("name", ["spread-min-values", "spread-min-values-broken"])
def test_min_values(plans, name):
    """Truncate's minValues check on the device (minvalues_ok on the finalized requirements): holding, and broken by
    the cut to 100 types (the NodeClaim's pods fail: UNSCHEDULED)."""
    got, st = _check(plans(name), name)
    assert st["phase_cycles"][0] == len(got)
    if name.endswith("broken"):
        assert any(g["verdict"] == vr.UNSCHEDULED and g["n_nodeclaims"] == 1 for g in got)
    else:
        assert any(g["verdict"] == vr.VALID and g["n_nodeclaims"] == 1 for g in got)


def test_two_catalogues(plans):
    """Every NodePool reads a second catalogue holding the same types in reverse order: the new NodeClaim lands on
    catalogue 1, and the command's names resolve through that catalogue's table, not the one they came from."""
    got, _ = _check(plans("two-catalogues"), "two-catalogues")
    assert got == vr.expected("spread")["records"]  # the same names: the same verdicts


def test_budgets(plans):
    """Budgets on the two-pool spread cluster: the inputs kpamd.disruption.admissible rejects are KP_INVALID_BUDGET and
    are neither batched nor compiled; the others keep their records."""
    import numpy as np
    from kpamd import disruption
    doc = vr.expected("spread")
    cl = vr.cluster_of("spread")[0]
    allowed = [3, 0]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in doc["subsets"]])]).astype(np.uint32)
    adm = disruption.admissible(cl, offs, np.concatenate(doc["subsets"]).astype(np.uint32), allowed)
    got, st = plans("spread").validate(doc["subsets"], doc["checks"], allowed=allowed)
    assert 0 < int(adm.sum()) < len(adm) and st["budget_blocked"] == int((~adm).sum())
    assert st["phase_cycles"][0] + st["phase_cycles"][1] == int(adm.sum())
    assert got == [w if ok else vr.BLOCKED for w, ok in zip(doc["records"], adm)]


def test_errors_and_cancel(ctx, plans):
    import kpamd
    from kpamd import abi
    doc = vr.expected("spread")
    plan = plans("spread")
    with pytest.raises(kpamd.KPError) as e:
        plan.validate(doc["subsets"][:2], [{"decision": vr.DELETE}, {"decision": vr.REPLACE, "options": []}])
    assert e.value.code == abi.KP_E_INVAL and "check 1" in str(e.value)
    tok = kpamd.Cancel(ctx)
    try:
        tok.set()
        with pytest.raises(kpamd.KPError) as e:
            plan.validate(doc["subsets"], doc["checks"], cancel=tok)
        assert e.value.code == abi.KP_E_CANCELED
        tok.reset()
        got, _ = plan.validate(doc["subsets"], doc["checks"], cancel=tok)  # the plan stays usable
    finally:
        tok.close()
    assert got == doc["records"]
