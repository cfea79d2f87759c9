"""The reason reference (tests/why_ref.py) held to the oracle and to the hand-written records, on the CPU: for every
subset the GPU tests use, the decision the restated order arrives at is the oracle's own computeConsolidation's; every
crafted case of tests/why_cases.py yields its hand-written record; the inputs reach every exit at least as often as the
sweep that motivated the call found them; and what the GPU tests read from tests/golden/ is what the reference
computes."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import command_ref  # noqa: E402
import why_cases  # noqa: E402
import why_ref  # noqa: E402
from why_ref import (BUDGET, MIN_VALUES, MULTIPLE_NODECLAIMS, NONE, NOT_CHEAPER, SAME_TYPE, SPOT_FLEXIBILITY,  # noqa: E402
                     SPOT_TO_SPOT_DISABLED, UNPRICED, UNSCHEDULABLE, bits)

CRAFTED = why_cases.BATCHED + why_cases.GENERAL
NAMED = why_ref.BATCHED + why_ref.GENERAL


def _decisions_agree(cl, subs, multi_node, decisions, whys, allowed=None):
    from oracle import pyoracle
    want, _ = pyoracle.simulate_batch(cl, subs, multi_node=multi_node)
    for s, (d, w, o) in enumerate(zip(decisions, whys, want)):
        if w["reason"] == BUDGET:
            continue
        assert d == o["decision"], f"subset {s} {subs[s]}: the restated order decides {d}, the oracle {o['decision']} ({w})"
        assert (w["reason"] == NONE) == (d != command_ref.NOOP)


@pytest.mark.parametrize("name", CRAFTED)
def test_crafted_records(name):
    """Every crafted case yields its hand-written record, and the decision the oracle takes."""
    cl, subs, want = why_cases.case(name)
    solves = {}
    for m in (False, True):
        whys, counts, decisions = why_ref.reference(cl, subs, m, None, solves=solves)
        for s, (g, w) in enumerate(zip(whys, want[m])):
            assert bits(g) == bits(w), f"{name} subset {s} {subs[s]}: reference {g}, hand-written {w}"
        _decisions_agree(cl, subs, m, decisions, whys)


@pytest.mark.parametrize("name", NAMED)
def test_decisions_and_recorded_files(name):
    """The named cases as the GPU tests cut them: the reference decides as the oracle does, and tests/golden/ holds
    what it computes, field for field."""
    cl, subs, multis, allowed = why_ref.case(name)
    for m in multis:
        whys, counts, decisions = why_ref.computed(name, m)
        _decisions_agree(cl, subs, m, decisions, whys)
        got = why_ref.expected(name, m)
        assert [bits(w) for w in got[0]] == [bits(w) for w in whys] and got[1] == counts and got[2] == decisions


def _tally(name, multi_node):
    """(reason, stage, decision) counts over ALL subsets of a command_ref case (config4: the whole 399), no budgets."""
    cl, subs, _, _ = command_ref.case(name)
    whys, _, decisions = why_ref.reference(cl, subs, multi_node, None, solves=command_ref._SOLVES.setdefault(name, {}))
    out = {}
    for w, d in zip(whys, decisions):
        key = (w["reason"], w["stage"], d)
        out[key] = out.get(key, 0) + 1
    return out, whys


DEL, REP, NOOP = command_ref.DELETE, command_ref.REPLACE, command_ref.NOOP
# the exits found on the project's own inputs when the call was proposed: at least these many of each must occur
FLOOR = {
    ("config4", True): {(NONE, 0, DEL): 16, (NONE, 0, REP): 63, (MULTIPLE_NODECLAIMS, 0, NOOP): 319, (SAME_TYPE, 0, NOOP): 1},
    ("min-values", False): {(NONE, 0, REP): 26, (NONE, 0, DEL): 12, (MULTIPLE_NODECLAIMS, 0, NOOP): 11,
                            (NOT_CHEAPER, 0, NOOP): 2, (MIN_VALUES, 1, NOOP): 10},
    ("min-values", True): {(NONE, 0, REP): 25, (NONE, 0, DEL): 12, (MULTIPLE_NODECLAIMS, 0, NOOP): 11,
                           (NOT_CHEAPER, 0, NOOP): 2, (MIN_VALUES, 1, NOOP): 10, (MIN_VALUES, 2, NOOP): 1},
    ("spot-to-spot-config4", True): {(NONE, 0, REP): 10, (NONE, 0, DEL): 7, (SPOT_FLEXIBILITY, 0, NOOP): 1},
    ("host-ports", True): {(NONE, 0, DEL): 20, (NONE, 0, REP): 1, (MULTIPLE_NODECLAIMS, 0, NOOP): 47,
                           (UNSCHEDULABLE, 0, NOOP): 1},
    ("anti-affinity", True): {(NONE, 0, DEL): 10, (NONE, 0, REP): 1, (MULTIPLE_NODECLAIMS, 0, NOOP): 29,
                              (UNSCHEDULABLE, 0, NOOP): 1, (NOT_CHEAPER, 0, NOOP): 1},
    ("spread", True): {(NONE, 0, REP): 3, (MULTIPLE_NODECLAIMS, 0, NOOP): 55},
}


@pytest.mark.parametrize("name,multi_node", sorted(FLOOR))
def test_coverage_floor(name, multi_node):
    got, whys = _tally(name, multi_node)
    for key, n in FLOOR[(name, multi_node)].items():
        assert got.get(key, 0) >= n, f"{name}: {key} occurs {got.get(key, 0)} times, {n} expected at least ({got})"
    if name == "config4":  # the subset the GPU tests add to the first 120
        assert whys[why_ref.SAME_TYPE_SUBSET]["reason"] == SAME_TYPE


def test_every_code_and_stage_occurs():
    """Every one of the ten codes and both stage values occurs in some input of the GPU tests."""
    seen = set()
    for name in CRAFTED:
        for want in why_cases.case(name)[2].values():
            seen |= {(w["reason"], w["stage"]) for w in want}
    for name in NAMED:
        for m in why_ref.case(name)[2]:
            seen |= {(w["reason"], w["stage"]) for w in why_ref.expected(name, m)[0]}
    assert {r for r, _ in seen} == set(range(why_ref.COUNT)), seen
    assert {(MIN_VALUES, 1), (MIN_VALUES, 2)} <= seen
    assert {BUDGET, UNPRICED, SPOT_TO_SPOT_DISABLED, SPOT_FLEXIBILITY} <= {r for r, _ in seen}
