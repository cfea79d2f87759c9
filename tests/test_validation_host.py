"""kpamd.disruption.Validation on the host: the candidate check (gone, marked for deletion, nominated, the budget walk),
emptiness, and what validate_command hands to plan.validate. No device: the plan is a stub that records its calls."""
import copy
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kpamd import disruption  # noqa: E402
from kpamd.disruption import DELETE, REPLACE, Command, Controller, Validation  # noqa: E402
from kpamd.model import Budget  # noqa: E402

POOL = disruption.POOL_LABEL


class StubPlan:
    def __init__(self, verdict=0):
        self.verdict, self.calls = verdict, []

    def validate(self, subsets, checks, allowed=None, cancel=None):
        self.calls.append((subsets, checks, allowed))
        return [{"verdict": self.verdict, "n_nodeclaims": 0, "n_pods": 0, "n_unscheduled": 0, "n_missing": 0,
                 "blocked": 0} for _ in subsets], {}


@pytest.fixture(scope="module")
def cluster(catalog):
    from kpamd import synth
    cl = synth.config4(catalog, n_nodes=12, seed=4, loose=0.05)
    for i, n in enumerate(cl.nodes):
        n.node.labels[POOL] = cl.nodepools[i % 2].name
    return cl


def _without(cluster, index):
    cl = copy.deepcopy(cluster)
    del cl.nodes[index]
    return cl


def test_candidates_map_by_name(cluster):
    """An earlier node is gone: the candidates keep their names and shift their indices."""
    cmd = Command("multi", [3, 5], DELETE, {"decision": DELETE, "replacements": []})
    new = _without(cluster, 1)
    mapped, why = Validation(new, StubPlan()).validate_candidates(cmd, cluster)
    assert (mapped, why) == ([2, 4], None)
    assert [new.nodes[i].node.name for i in mapped] == [cluster.nodes[c].node.name for c in cmd.candidates]


def test_candidate_gone_deleting_nominated(cluster):
    cmd = Command("single", [4], DELETE, {"decision": DELETE, "replacements": []})
    name = cluster.nodes[4].node.name
    plan = StubPlan()
    assert Validation(_without(cluster, 4), plan).validate_candidates(cmd, cluster) == (None, f"candidate {name} is gone")
    new = copy.deepcopy(cluster)
    new.nodes[4].deleting = True
    assert Validation(new, plan).validate_candidates(cmd, cluster) == (None, f"candidate {name} is marked for deletion")
    new = copy.deepcopy(cluster)
    new.nodes[4].nominated = True
    ok, why, rec = Validation(new, plan).validate_command(cmd, cluster)
    assert (ok, rec) == (False, None) and "nominated" in why
    assert plan.calls == []  # a failed candidate check asks the device nothing
    assert Controller().validate(cmd, cluster, new, plan) == (False, why)


def test_budget_walk(cluster):
    """With budgets modelled the walk over the mapped candidates must keep them all, for the command's reason."""
    new = copy.deepcopy(cluster)
    for p in new.nodepools:
        p.budgets = [Budget("1", reasons=["Underutilized"])]
    same_pool = [i for i, n in enumerate(new.nodes) if n.node.labels[POOL] == new.nodepools[0].name]
    other = next(i for i in range(len(new.nodes)) if i not in same_pool)
    plan = StubPlan()
    two = Command("multi", same_pool[:2], DELETE, {"decision": DELETE, "replacements": []})
    mapped, why = Validation(new, plan).validate_candidates(two, cluster)
    assert mapped is None and "Underutilized budget" in why
    one = Command("multi", [same_pool[0], other], DELETE, {"decision": DELETE, "replacements": []})
    assert Validation(new, plan).validate_candidates(one, cluster) == ([same_pool[0], other], None)
    ok, _, _ = Validation(new, plan).validate_command(one, cluster)
    assert ok and plan.calls[-1][2] == [1, 1]  # the device gate gets the same allowances
    # the allowance consumed meanwhile: another node of the pool is being deleted
    new.nodes[same_pool[1]].deleting = True
    mapped, why = Validation(new, plan).validate_candidates(one, cluster)
    assert mapped is None and "budget" in why
    # a budget for another reason does not bind; an emptiness command asks with Empty
    for p in new.nodepools:
        p.budgets = [Budget("0", reasons=["Empty"])]
    assert Validation(new, plan).validate_candidates(one, cluster)[0] is not None
    assert Validation(new, plan).validate_candidates(Command("emptiness", [other], DELETE), cluster)[0] is None


def test_emptiness(cluster):
    old = copy.deepcopy(cluster)
    moved = old.nodes[2].pods
    old.nodes[2].pods = []
    cmd = Command("emptiness", [2], DELETE, {"decision": DELETE})
    plan = StubPlan()
    assert Validation(old, plan).validate_command(cmd, old) == (True, None, None)
    new = copy.deepcopy(old)
    new.nodes[2].pods = list(moved[:1])
    ok, why, _ = Validation(new, plan).validate_command(cmd, old)
    assert not ok and "no longer empty" in why
    new = copy.deepcopy(old)
    new.nodes[2].deleting = True
    assert not Validation(new, plan).validate_command(cmd, old)[0]
    assert plan.calls == []  # emptiness never simulates


def test_validate_command_checks(cluster):
    """A DELETE asks without options, a REPLACE with its replacement's options by name through the OLD cluster's
    catalogue; the verdict decides; Drift is not validated."""
    plan = StubPlan()
    v = Validation(cluster, plan)
    assert v.validate_command(Command("multi", [1, 2], DELETE, {"decision": DELETE, "replacements": []}), cluster)[0]
    assert plan.calls[-1] == ([[1, 2]], [{"decision": DELETE}], None)
    repl = {"nodepool": 0, "options": [70, 3, 5]}
    cmd = Command("single", [1], REPLACE, {"decision": REPLACE, "replacements": [repl]})
    old = copy.deepcopy(cluster)
    old.catalogs = [list(reversed(cluster.catalogs[0]))]  # the old snapshot's indices are its own
    assert v.validate_command(cmd, old)[0]
    names = [old.catalogs[0][t].name for t in (70, 3, 5)]
    assert plan.calls[-1][1] == [{"decision": REPLACE, "options": names}]
    bad = StubPlan(verdict=5)
    ok, why, rec = Validation(cluster, bad).validate_command(cmd, old)
    assert (ok, why, rec["verdict"]) == (False, "not-subset", 5)
    with pytest.raises(ValueError, match="materialize"):
        v.validate_command(Command("single", [1], REPLACE, {"decision": REPLACE}), cluster)
    drift = Command("drift", [1], DELETE, {"decision": DELETE, "replacements": []})
    with pytest.raises(ValueError, match="not validated"):
        v.validate_command(drift, cluster)
    assert Controller().validate(drift, cluster, cluster, plan) == (True, None)
