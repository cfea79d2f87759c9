"""kp_cluster_simulate_explained on the device: every field of every kp_sim_why record equals the expectation with ==
(floats by bit pattern) - the hand-written records of tests/why_cases.py and, for the named clusters, the reference of
tests/why_ref.py as recorded under tests/golden/ - the histogram equals the records', and out[] is bit for bit what
kp_cluster_simulate_budgeted writes on the same plan before and after the call."""
import copy
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import command_ref  # noqa: E402
import why_cases  # noqa: E402
import why_ref  # noqa: E402
from why_ref import bits  # noqa: E402

pytestmark = pytest.mark.gpu


def _explain(plan, subs, multi_node, allowed, want):
    """simulate_explained against the expected records; out against simulate() before and after; counts against the
    records. Returns (sims, whys, counts, stats)."""
    before, _ = plan.simulate(subs, multi_node=multi_node, allowed=allowed)
    sims, whys, counts, st = plan.simulate_explained(subs, multi_node=multi_node, allowed=allowed)
    after, _ = plan.simulate(subs, multi_node=multi_node, allowed=allowed)
    assert [bits(d) for d in sims] == [bits(d) for d in before] == [bits(d) for d in after]
    for s, (g, w) in enumerate(zip(whys, want)):
        assert bits(g) == bits(w), f"subset {s} {subs[s]}: device {g}, expected {w}"
    assert len(whys) == len(want) and counts == why_ref.histogram(whys)
    for s, (sim, w) in enumerate(zip(sims, whys)):  # the record and the decision agree
        assert (w["reason"] == why_ref.NONE) == (sim["decision"] != command_ref.NOOP), (s, sim, w)
    if allowed is not None:
        assert st["budget_blocked"] == counts[why_ref.BUDGET]
    return sims, whys, counts, st


@pytest.fixture(scope="module")
def plans(ctx):
    import kpamd
    made = {}

    def get(name):
        if name not in made:
            cl = why_cases.case(name)[0] if name in why_cases.BATCHED + why_cases.GENERAL else why_ref.case(name)[0]
            made[name] = kpamd.ClusterPlan(ctx, cl)
        return made[name]
    yield get
    for p in made.values():
        p.close()


@pytest.mark.parametrize("name", why_cases.BATCHED)
def test_crafted(plans, name):
    """The batched kernel on the crafted inputs: the price filter's counts across the lane halves and at the strict <,
    SAME_TYPE, unpriced candidates, the first unscheduled pod at queue positions 0, 63, 64 and 129, uninitialized nodes,
    a second NodeClaim, binding limits, the gate-off-and-minValues order, a failing pod next to a NodeClaim whose
    truncated options break minValues, and 14 against 15 cheaper spot options with the gate on and off."""
    cl, subs, want = why_cases.case(name)
    for m in (False, True):
        _, whys, _, st = _explain(plans(name), subs, m, None, want[m])
    if name == "limits":  # the record came from the subset's own Solve, and only that subset had one
        assert st["phase_cycles"][3] == 1 and whys[0]["reason"] == why_ref.UNSCHEDULABLE
    else:
        assert st["phase_cycles"][3] == 0


@pytest.mark.parametrize("name", why_cases.GENERAL)
def test_crafted_general(plans, name):
    """The same inputs with a hostname spread on every shape: general-path plans, the decision code's records."""
    cl, subs, want = why_cases.case(name)
    for m in (False, True):
        _, _, _, st = _explain(plans(name), subs, m, None, want[m])
    assert st["phase_cycles"][0] + st["phase_cycles"][1] == len(subs)  # every subset a Solve of the general path


@pytest.mark.parametrize("name", why_ref.BATCHED + why_ref.GENERAL)
def test_named(plans, name):
    cl, subs, multis, allowed = why_ref.case(name)
    for m in multis:
        want, want_counts, _ = why_ref.expected(name, m)
        _, whys, counts, st = _explain(plans(name), subs, m, allowed, want)
        assert counts == want_counts
    if name == "disruption-state":  # limits that bind without flipping a record: every re-run confirms MULTIPLE
        assert st["phase_cycles"][3] == counts[why_ref.MULTIPLE_NODECLAIMS] == 41
    if name == "anti-affinity":
        assert st["phase_cycles"][1] > 0  # some subsets were compiled alone


COUNT_SIZES = (0, 1, 300, 255, 256, 257, 64 * 256 - 1, 64 * 256, 64 * 256 + 1)


def test_counts(plans):
    """counts equals the histogram of why for 0, 1 and a few hundred subsets and for sizes one below, at and one above
    why_count_kernel's block (256 threads) and its first-stage grid (64 blocks); with budgets the blocked subsets are
    under BUDGET and carry the BUDGET record."""
    cl, subs, _, _ = why_ref.case("min-values")
    want, _, _ = why_ref.expected("min-values", True)
    plan = plans("min-values")
    for n in COUNT_SIZES:
        batch = [subs[i % len(subs)] for i in range(n)]
        sims, whys, counts, _ = plan.simulate_explained(batch, multi_node=True)
        assert counts == why_ref.histogram([want[i % len(subs)] for i in range(n)]), n
        assert all(bits(whys[i]) == bits(want[i % len(subs)]) for i in range(n)), n
    cl, subs, _, allowed = why_ref.case("budgets")
    want, _, _ = why_ref.expected("budgets", True)
    for n in (257, 64 * 256 + 1):
        batch = [subs[i % len(subs)] for i in range(n)]
        sims, whys, counts, st = plans("budgets").simulate_explained(batch, multi_node=True, allowed=allowed)
        assert counts == why_ref.histogram([want[i % len(subs)] for i in range(n)]), n
        assert all(bits(whys[i]) == bits(want[i % len(subs)]) for i in range(n)), n
        assert 0 < counts[why_ref.BUDGET] == st["budget_blocked"]


@pytest.mark.parametrize("name", ["min-values", "disruption-state", "spread"])
def test_histogram_alone(plans, name):
    """why = NULL: the same histogram and out[] without the records - on a batched plan, on one whose limits send
    records to their own Solve, and on a general-path plan."""
    cl, subs, multis, allowed = why_ref.case(name)
    m = multis[-1]
    sims, whys, counts, st = plans(name).simulate_explained(subs, multi_node=m, allowed=allowed)
    sims2, none, counts2, st2 = plans(name).simulate_explained(subs, multi_node=m, allowed=allowed, records=False)
    assert none is None and counts2 == counts == why_ref.expected(name, m)[1]
    assert [bits(d) for d in sims2] == [bits(d) for d in sims]
    assert st2["phase_cycles"][3] == st["phase_cycles"][3]


def test_slot_reuse(plans, ov):
    """sim_slots 4: each wave runs REPLACE, NOT_CHEAPER, UNSCHEDULABLE, DELETE, then (behind a budget-blocked
    neighbour, which no wave runs) REPLACE again in one reused slot; the records equal the production-size run's bit for
    bit, and the hand-written ones."""
    cl, subs, want = why_cases.case("solve-exits")
    at = {tuple(s): w for s, w in zip(subs, want[True])}
    seq = [[0], [18], [8], [6], [1, 0, 2], [0]]
    batch = [s for s in seq for _ in range(4)]
    plan = plans("solve-exits")
    wide = plan.simulate_explained(batch, multi_node=True, allowed=[1])
    assert wide[3]["phase_cycles"][2] == 1  # production size: no wave ran two subsets
    ov(sim_slots=4)
    sims, whys, counts, st = plan.simulate_explained(batch, multi_node=True, allowed=[1])
    assert st["phase_cycles"][1] == 4 and st["phase_cycles"][2] == 5  # four slots, five simulations each
    assert [bits(w) for w in whys] == [bits(w) for w in wide[1]] and [bits(d) for d in sims] == [bits(d) for d in wide[0]]
    assert counts == wide[2] and counts[why_ref.BUDGET] == 4
    for s, w in zip(batch, whys):
        assert bits(w) == bits(why_ref.record(why_ref.BUDGET) if len(s) > 1 else at[tuple(s)])


def test_other_paths(ctx, plans):
    """A cancelled call and a call after it, a stale plan, an n_allowed mismatch, a deleting node in a subset."""
    import kpamd
    from kpamd import abi
    cl, subs, _, _ = why_ref.case("min-values")
    want, want_counts, _ = why_ref.expected("min-values", True)
    plan = plans("min-values")
    tok = kpamd.Cancel(ctx)
    try:
        tok.set()
        with pytest.raises(kpamd.KPError) as e:
            plan.simulate_explained(subs, cancel=tok)
        assert e.value.code == abi.KP_E_CANCELED
        tok.reset()
        _, whys, counts, _ = plan.simulate_explained(subs, cancel=tok)  # the plan stays usable
    finally:
        tok.close()
    assert [bits(w) for w in whys] == [bits(w) for w in want] and counts == want_counts
    assert plan.simulate_explained([])[:3] == ([], [], [0] * why_ref.COUNT)
    with pytest.raises(kpamd.KPError) as e:
        plan.simulate_explained(subs, allowed=[1, 1, 1, 1, 1, 1, 1])
    assert e.value.code == abi.KP_E_INVAL
    ds, ds_subs, _, _ = why_ref.case("disruption-state")
    deleting = next(i for i, n in enumerate(ds.nodes) if n.deleting)
    with pytest.raises(kpamd.KPError) as e:
        plans("disruption-state").simulate_explained([ds_subs[0], [ds_subs[1][0], deleting]])
    assert e.value.code == abi.KP_E_INVAL and "subset 1" in str(e.value) and "deleted" in str(e.value)
    cat = kpamd.Catalog(ctx, copy.deepcopy(cl.catalogs[0]), seqnum=1)
    p = kpamd.ClusterPlan(ctx, cl, catalogs=[cat])
    try:
        p.simulate_explained([[0]])
        t = next(i for i, it in enumerate(cl.catalogs[0])
                 if any(o.capacity_type == "spot" and o.zone == "test-zone-1a" for o in it.offerings))
        cat.update_offerings([(t, "spot", "test-zone-1a", False)], seqnum=2)
        with pytest.raises(kpamd.KPError, match="stale plan"):
            p.simulate_explained([[0]])
    finally:
        p.close()
        cat.close()
