"""NodePool disruption budgets on the host (kpamd.disruption): allowed disruptions per NodePool and reason, budget
schedules (five-field cron and macros, UTC), the candidate walk and the sweep's per-subset admissibility
(R:website/content/en/preview/concepts/disruption.md:274-333, R:pkg/apis/crds/karpenter.sh_nodepools.yaml:95-135)."""
import calendar
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

POOL = "karpenter.sh/nodepool"


def _cluster(pool_nodes, budgets=None, deleting=()):
    """A bare cluster: pool_nodes = [(pool name, node count)], budgets = {pool name: [Budget]}; node i of the whole
    list is deleting when i is in `deleting`. Node names sort in index order."""
    from kpamd.model import Cluster, ClusterNode, ExistingNode, NodePool
    budgets = budgets or {}
    pools = [NodePool(name, budgets=budgets.get(name)) for name, _ in pool_nodes]
    nodes = []
    for name, n in pool_nodes:
        for _ in range(n):
            i = len(nodes)
            nodes.append(ClusterNode(ExistingNode(f"n{i:04d}", {POOL: name}, {}), 0, 0, [], deleting=i in deleting))
    z = np.zeros(0, dtype=np.uint32)
    return Cluster([[]], pools, nodes, [], z, z.astype(np.int64), z.astype(np.uint64))


def _utc(*t):
    return calendar.timegm(t)


def _doc_budgets():
    """The documentation's example NodePool (disruption.md:291-310)."""
    from kpamd.model import Budget
    return [Budget("20%", reasons=["Empty", "Drifted"]), Budget("5"),
            Budget("0", reasons=["Underutilized"], schedule="@daily", duration_s=600)]


# ---- arithmetic ------------------------------------------------------------------------------------------------------
def test_documentation_example():
    from kpamd.disruption import allowed_disruptions
    noon = _utc(2025, 3, 14, 12, 0, 0)
    cl = _cluster([("default", 19)], {"default": _doc_budgets()})
    assert allowed_disruptions(cl, "Empty", now=noon) == [4]        # roundup(19 * 0.2) = 4
    assert allowed_disruptions(cl, "Drifted", now=noon) == [4]
    assert allowed_disruptions(cl, "Underutilized", now=noon) == [5]
    cl30 = _cluster([("default", 30)], {"default": _doc_budgets()})
    assert allowed_disruptions(cl30, "Empty", now=noon) == [5]      # the "5" budget is the ceiling past 25 nodes
    assert allowed_disruptions(cl, "Underutilized", now=_utc(2025, 3, 14, 0, 5, 0)) == [0]
    assert allowed_disruptions(cl, "Empty", now=_utc(2025, 3, 14, 0, 5, 0)) == [4]
    assert allowed_disruptions(cl, "Underutilized", now=_utc(2025, 3, 14, 0, 9, 59)) == [0]
    assert allowed_disruptions(cl, "Underutilized", now=_utc(2025, 3, 14, 0, 10, 0)) == [5]


def test_deleting_and_not_ready_subtract():
    from kpamd.disruption import allowed_disruptions
    from kpamd.model import Budget
    cl = _cluster([("default", 10)], {"default": [Budget("50%")]}, deleting={0, 1})
    assert allowed_disruptions(cl, "Empty") == [3]                       # ceil(10 * .5) - 2 deleting
    assert allowed_disruptions(cl, "Empty", not_ready=[4]) == [2]
    assert allowed_disruptions(cl, "Empty", not_ready=[2, 3, 4, 5]) == [0]  # floor of 0
    # nodes still terminating but gone from the snapshot: total 12, deleting 4 -> 6 - 4
    assert allowed_disruptions(cl, "Empty", extra_deleting={"default": 2}) == [2]
    assert allowed_disruptions(cl, "Empty", extra_deleting={0: 2}) == [2]


def test_values_and_unmodelled():
    from kpamd.disruption import UNLIMITED, allowed_disruptions, budget_value
    from kpamd.model import Budget
    assert UNLIMITED == 2**32 - 1
    assert [budget_value(v, 7) for v in ("0%", "100%", "0", "10%", "99%", "12")] == [0, 7, 0, 1, 7, 12]
    for bad in ("101%", "-1", "5 %", "", "1.5", "abc"):
        with pytest.raises(ValueError):
            budget_value(bad, 7)
    cl = _cluster([("a", 7), ("b", 3), ("c", 2)], {"a": [Budget("0%")], "c": [Budget("100%"), Budget("1", ["Drifted"])]})
    assert allowed_disruptions(cl, "Empty") == [0, UNLIMITED, 2]
    assert allowed_disruptions(cl, "Drifted") == [0, UNLIMITED, 1]
    empty_list = _cluster([("a", 4)], {"a": []})
    assert allowed_disruptions(empty_list, "Empty") == [UNLIMITED]      # no active applicable budget


# ---- cron ------------------------------------------------------------------------------------------------------------
def test_window_as_the_suite_builds_it():
    """R:test/suites/consolidation/suite_test.go:455-460: the schedule fires at now - 15 min, duration 30 min."""
    import time
    from kpamd.disruption import budget_active
    from kpamd.model import Budget
    now = _utc(2025, 6, 30, 23, 50, 17)
    start = time.gmtime(now - 15 * 60)
    b = Budget("0", schedule=f"{start.tm_min} {start.tm_hour} * * *", duration_s=30 * 60)
    assert budget_active(b, now)
    assert budget_active(b, now + 14 * 60)
    assert not budget_active(b, now + 16 * 60)
    assert not budget_active(b, now - 16 * 60)


def test_lists_ranges_steps():
    from kpamd.disruption import parse_schedule, schedule_next
    mins, hours, doms, months, dows, dom_r, dow_r = parse_schedule("0,15,30-32 */6 1-3 2-12/5 *")
    assert mins == {0, 15, 30, 31, 32} and hours == {0, 6, 12, 18} and doms == {1, 2, 3} and months == {2, 7, 12}
    assert dows == set(range(7)) and dom_r and not dow_r
    assert parse_schedule("5/20 * * * *")[0] == {5, 25, 45}
    assert parse_schedule("* * * * 5-7")[4] == {5, 6, 0}              # 7 is also Sunday
    t = _utc(2025, 1, 1, 0, 0, 0)
    assert schedule_next("0,15,30-32 */6 1-3 2-12/5 *", t) == _utc(2025, 2, 1, 0, 0, 0)
    assert schedule_next("0,15,30-32 */6 1-3 2-12/5 *", _utc(2025, 2, 1, 0, 0, 0)) == _utc(2025, 2, 1, 0, 15, 0)
    assert schedule_next("0,15,30-32 */6 1-3 2-12/5 *", _utc(2025, 2, 3, 18, 32, 0)) == _utc(2025, 7, 1, 0, 0, 0)
    assert schedule_next("*/20 3 * * *", _utc(2025, 1, 1, 3, 40, 0)) == _utc(2025, 1, 2, 3, 0, 0)
    assert schedule_next("0 0 29 2 *", t) == _utc(2028, 2, 29, 0, 0, 0)
    for bad in ("* * * *", "60 * * * *", "* 24 * * *", "* * 0 * *", "* * * 13 *", "* * * * 8", "* * * jan *",
                "* * * * mon", "*/0 * * * *", "5-1 * * * *", "@fortnightly", "a b c d e"):
        with pytest.raises(ValueError):
            parse_schedule(bad)


def test_day_of_month_or_day_of_week():
    from kpamd.disruption import schedule_next
    t = _utc(2025, 1, 1, 0, 0, 0)  # a Wednesday
    # both restricted: either one matching suffices (the 13th, or any Friday)
    assert schedule_next("0 0 13 * 5", t) == _utc(2025, 1, 3, 0, 0, 0)            # Friday the 3rd
    assert schedule_next("0 0 13 * 5", _utc(2025, 1, 10, 0, 0, 0)) == _utc(2025, 1, 13, 0, 0, 0)  # Monday the 13th
    # only one restricted: both must match
    assert schedule_next("0 0 13 * *", t) == _utc(2025, 1, 13, 0, 0, 0)
    assert schedule_next("0 0 * * 5", t) == _utc(2025, 1, 3, 0, 0, 0)
    assert schedule_next("0 0 * * 0", t) == schedule_next("0 0 * * 7", t) == _utc(2025, 1, 5, 0, 0, 0)
    # a step over * leaves the field unrestricted: every second day AND a Friday
    assert schedule_next("0 0 */2 * 5", t) == _utc(2025, 1, 3, 0, 0, 0)
    assert schedule_next("0 0 */2 * 5", _utc(2025, 1, 3, 0, 0, 0)) == _utc(2025, 1, 17, 0, 0, 0)


@pytest.mark.parametrize("macro,want", [
    ("@yearly", (2026, 1, 1, 0, 0, 0)), ("@annually", (2026, 1, 1, 0, 0, 0)), ("@monthly", (2025, 6, 1, 0, 0, 0)),
    ("@weekly", (2025, 5, 18, 0, 0, 0)), ("@daily", (2025, 5, 15, 0, 0, 0)), ("@midnight", (2025, 5, 15, 0, 0, 0)),
    ("@hourly", (2025, 5, 14, 11, 0, 0))])
def test_macros(macro, want):
    from kpamd.disruption import schedule_next
    assert schedule_next(macro, _utc(2025, 5, 14, 10, 30, 0)) == _utc(*want)  # a Wednesday; the 18th is a Sunday


def test_schedule_and_duration_go_together():
    from kpamd.disruption import allowed_disruptions, budget_active
    from kpamd.model import Budget
    with pytest.raises(ValueError):
        budget_active(Budget("1", schedule="@daily"), 0)
    with pytest.raises(ValueError):
        budget_active(Budget("1", duration_s=60), 0)
    with pytest.raises(ValueError):
        allowed_disruptions(_cluster([("a", 2)], {"a": [Budget("1", duration_s=60)]}), "Empty", now=0)


# ---- walk and admissibility --------------------------------------------------------------------------------------------
def test_budget_walk_two_pools():
    from kpamd.disruption import UNLIMITED, budget_walk
    cl = _cluster([("a", 4), ("b", 4)])
    order = [4, 0, 5, 1, 6, 2, 7, 3]  # b a b a b a b a
    assert budget_walk(cl, order, [1, 2]) == [4, 0, 5]
    assert budget_walk(cl, order, [0, UNLIMITED]) == [4, 5, 6, 7]
    assert budget_walk(cl, order, [3, 0]) == [0, 1, 2]
    assert budget_walk(cl, order, [UNLIMITED, UNLIMITED]) == order
    assert budget_walk(cl, budget_walk(cl, order, [1, 2]), [1, 2]) == [4, 0, 5]  # idempotent
    cl.nodes[2].node.labels.pop(POOL)
    with pytest.raises(ValueError):
        budget_walk(cl, order, [4, 4])


def test_admissible_equals_a_plain_loop():
    from kpamd.disruption import UNLIMITED, admissible
    cl = _cluster([("a", 50), ("b", 30), ("c", 20)])
    rng = np.random.default_rng(3)
    subs = [sorted(rng.choice(100, int(rng.integers(0, 40)), replace=False).tolist()) for _ in range(300)]
    subs += [[], [7], list(range(100))]
    offs = np.zeros(len(subs) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(s) for s in subs])
    flat = np.array([c for s in subs for c in s], dtype=np.uint32)
    owner = [0] * 50 + [1] * 30 + [2] * 20
    seen = set()
    for allowed in ([8, 3, 2], [0, 0, 0], [UNLIMITED] * 3, [UNLIMITED, 0, 4], [50, 30, 20]):
        want = []
        for s in subs:
            cnt = [0, 0, 0]
            for c in s:
                cnt[owner[c]] += 1
            want.append(all(cnt[p] <= allowed[p] for p in range(3)))
        got = admissible(cl, offs, flat, allowed)
        assert got.dtype == bool and got.tolist() == want
        seen.update(want)
    assert seen == {True, False}
    with pytest.raises(ValueError):
        admissible(cl, offs, flat, [1, 2])


# ---- unchanged behaviour ---------------------------------------------------------------------------------------------
def test_controller_unchanged_without_and_with_full_budgets(catalog):
    """Controller.compute_command on config 4: budgets None, "100%" on every pool, and the parent's logic driven
    directly (Emptiness' rule, first_n_option, compute_command over the oracle's results) give the same command."""
    import copy
    from e2e import OraclePlan
    from kpamd import disruption, synth
    from kpamd.model import Budget
    from oracle import pyoracle
    cl = synth.config4(catalog, n_nodes=150, seed=12)
    assert all(p.budgets is None for p in cl.nodepools)
    plain = disruption.Controller().compute_command(cl, OraclePlan(cl))
    full = copy.copy(cl)
    full.nodepools = [copy.copy(p) for p in cl.nodepools]
    for p in full.nodepools:
        p.budgets = [Budget("100%")]
    budgeted = disruption.Controller().compute_command(full, OraclePlan(full), now=0)

    cands = disruption.candidate_order(cl)
    empty = [c for c in cands if not cl.nodes[c].pods]
    if empty:
        want = ("emptiness", empty, disruption.DELETE)
    else:
        mids = disruption.MultiNodeConsolidation.search_prefixes(len(cands))
        res, _ = pyoracle.simulate_batch(cl, [cands[:m + 1] for m in mids], multi_node=True)
        hit = disruption.MultiNodeConsolidation.replay(len(cands), dict(zip(mids, res)))
        if hit is not None:
            want = ("multi", cands[:hit[0] + 1], hit[1]["decision"])
        else:
            res1, _ = pyoracle.simulate_batch(cl, [[c] for c in cands], multi_node=False)
            first = next(((c, r) for c, r in zip(cands, res1) if r["decision"] != 0), None)
            want = None if first is None else ("single", [first[0]], first[1]["decision"])
    for cmd in (plain, budgeted):
        got = None if cmd is None else (cmd.method, cmd.candidates, cmd.decision)
        assert got == want
    assert want is not None
