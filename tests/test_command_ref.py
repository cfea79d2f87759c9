"""The command reference (tests/command_ref.py) held to the oracle's own decision, on the CPU: for every subset of every
cluster tests/test_gpu_command.py and tests/test_gpu_command_general.py use, the Python restatement of the price
filters over the simulation's oracle Solve must arrive where the oracle's computeConsolidation arrives - no exceptions.
The chosen inputs must also reach the states the GPU tests are there for."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import command_ref  # noqa: E402
from command_ref import DELETE, NOOP, REPLACE  # noqa: E402

CASES = command_ref.BATCHED_CASES + command_ref.GENERAL_CASES


def _agree(name, multi_node):
    """reference() without budgets against pyoracle.simulate_batch; returns (sims, commands, infos)."""
    from oracle import pyoracle
    cl, subs, _, _ = command_ref.case(name)
    sims, cmds, infos = command_ref.reference(cl, subs, multi_node, None, solves=command_ref._SOLVES.setdefault(name, {}))
    want, _ = pyoracle.simulate_batch(cl, subs, multi_node=multi_node)
    for s, (g, w, c) in enumerate(zip(sims, want, cmds)):
        assert g == w, f"{name} subset {s} {subs[s]}: reference {g}, oracle {w}"  # (floats: == is bit for bit here)
        if w["decision"] == REPLACE:
            nc = c["nodeclaims"][0]
            assert len(c["nodeclaims"]) == 1 and len(nc["options"]) == w["n_options"]
            cat = cl.catalogs[cl.nodepools[nc["nodepool"]].catalog]
            s2s = infos[s]["s2s"]
            assert min(command_ref.e2e.worst_launch_price(cat[t], nc["requirements"], s2s) for t in nc["options"]) == \
                w["replacement_price"]
            assert sorted(nc["pods"]) == [p for p, t in enumerate(c["placement"]) if t == 0]
        elif w["decision"] == DELETE:
            # DELETE iff the Solve made no NodeClaim and every non-pending pod is placed
            n_pending = len(cl.pending)
            assert c["nodeclaims"] == [] and all(int(t) <= -2 for t in c["placement"][n_pending:])
        else:
            assert c is None
    return sims, cmds, infos


@pytest.mark.parametrize("name", CASES)
def test_reference_agrees_with_the_oracle(name):
    _, _, multis, _ = command_ref.case(name)
    for m in multis:
        _agree(name, m)


def test_inputs_reach_the_states_that_matter():
    """Over the batched-kernel cases: a REPLACE keeping more than 64 options (both lane halves), filterByPrice dropping
    options from the middle of the list, filterOutSameType dropping more, a spot-to-spot single cut to exactly 15, a
    DELETE, a NOOP, a subset with pods on existing nodes and on the NodeClaim."""
    seen = set()
    for name in command_ref.BATCHED_CASES:
        cl, subs, multis, _ = command_ref.case(name)
        for m in multis:
            sims, cmds, infos = command_ref.reference(cl, subs, m, None, solves=command_ref._SOLVES.setdefault(name, {}))
            for sub, sim, cmd, i in zip(subs, sims, cmds, infos):
                seen.add({NOOP: "noop", DELETE: "delete", REPLACE: "replace"}[sim["decision"]])
                if sim["decision"] != REPLACE:
                    continue
                if i["kept"] > 64:
                    seen.add("more than 64 kept")
                if i["price_hole"]:
                    seen.add("filterByPrice drops from the middle")
                if i["after_same_type"] < i["after_price"]:
                    seen.add("filterOutSameType drops more")
                if i["s2s"] and len(sub) == 1 and i["after_same_type"] > 15 and i["kept"] == 15:
                    seen.add("spot-to-spot single cut to 15")
                if i["on_existing"] and i["on_nodeclaim"]:
                    seen.add("pods on existing nodes and on the NodeClaim")
                if len(cl.pending) and any(int(t) == -1 for t in cmd["placement"][:len(cl.pending)]):
                    seen.add("an unschedulable pending pod")
    assert seen >= {"noop", "delete", "replace", "more than 64 kept", "filterByPrice drops from the middle",
                    "filterOutSameType drops more", "spot-to-spot single cut to 15",
                    "pods on existing nodes and on the NodeClaim"}, seen


@pytest.mark.parametrize("name", command_ref.ALL_CASES)
def test_recorded_commands_are_the_reference(name):
    """What the GPU tests read from tests/golden/ is what the reference computes, field for field."""
    for m in command_ref.case(name)[2]:
        want, got = command_ref.computed(name, m), command_ref.expected(name, m)
        assert got[0] == want[0]
        assert [command_ref.command_fields(c) for c in got[1]] == [command_ref.command_fields(c) for c in want[1]]


def test_budgets_block_some():
    cl, subs, _, allowed = command_ref.case("budgets")
    sims, cmds, _ = command_ref.expected("budgets", True)
    blocked = [s for s, x in enumerate(sims) if x["n_pods"] == 0]
    assert 0 < len(blocked) < len(subs) and all(cmds[s] is None for s in blocked)
    assert any(c is not None for c in cmds)
