"""kp_cluster_command on general-path plans (topology spread, pod anti-affinity, capacity reservations): the command is
read from the simulation's arena of the batched launch that decides (or from the Solve of a subset compiled on its own);
every field equals the reference of tests/command_ref.py, and the per-subset results are those of
kp_cluster_simulate_budgeted on the same plan, bit for bit."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import command_ref  # noqa: E402
from test_gpu_command import _bits  # noqa: E402

pytestmark = pytest.mark.gpu
RID = "karpenter.k8s.aws/capacity-reservation-id"


def _ceil(a, b):
    return (a + b - 1) // b


def _fields(cmds):
    return [command_ref.command_fields(c) for c in cmds]


def _check(plan, name, multi_node):
    """One command call on the plan against the reference and against simulate(); returns the call's results."""
    cl, subs, _, allowed = command_ref.case(name)
    sims_w, cmds_w, _ = command_ref.expected(name, multi_node)
    sims, cmds, st = plan.command(subs, multi_node=multi_node, allowed=allowed)
    plain, st2 = plan.simulate(subs, multi_node=multi_node, allowed=allowed)
    assert sims == sims_w
    for s, (g, w) in enumerate(zip(cmds, cmds_w)):
        assert command_ref.command_fields(g) == command_ref.command_fields(w), f"{name} subset {s} {subs[s]}"
    assert [_bits(d) for d in sims] == [_bits(d) for d in plain]
    assert st["phase_cycles"][:3] == st2["phase_cycles"][:3]  # batched, compiled alone, launches: as simulate runs them
    return sims, cmds, st


@pytest.fixture
def plan_of(ctx):
    import kpamd
    made = []

    def make(name):
        made.append(kpamd.ClusterPlan(ctx, command_ref.case(name)[0]))
        return made[-1]
    yield make
    for p in made:
        p.close()


def test_spread_one_launch_and_many(plan_of, ov):
    """The 120-node spread cluster: the commands of one launch, then of 9 launches of 7 simulations over the two slots
    (at least 4 launches per slot, every arena reused and dirty), then of the list reversed on those arenas: the
    command call's own stats count the launches, and the commands are identical."""
    _, subs, _, _ = command_ref.case("spread")
    plan = plan_of("spread")
    sims1, cmds1, st1 = _check(plan, "spread", True)
    assert st1["phase_cycles"][:3] == [len(subs), 0, 1]
    assert {s["decision"] for s in sims1} >= {0, 2}
    assert any(c and c["nodeclaims"] and (c["placement"] <= -2).any() for c in cmds1)
    ov(general_launch=7)
    sims7, cmds7, st7 = _check(plan, "spread", True)
    assert st7["phase_cycles"][:3] == [len(subs), 0, _ceil(len(subs), 7)] and st7["phase_cycles"][2] >= 8
    assert [_bits(d) for d in sims7] == [_bits(d) for d in sims1] and _fields(cmds7) == _fields(cmds1)
    simsr, cmdsr, str_ = plan.command(subs[::-1], multi_node=True)
    assert str_["phase_cycles"][2] >= 8
    assert [_bits(d) for d in simsr] == [_bits(d) for d in sims1[::-1]] and _fields(cmdsr) == _fields(cmds1[::-1])


@pytest.mark.parametrize("multi_node", [False, True])
def test_anti_affinity(plan_of, ov, multi_node):
    """Subsets that remove every owner of an inverse anti-affinity term are compiled on their own, the others batched
    (4 per launch): one command call takes commands from both."""
    ov(general_launch=4)
    sims, cmds, st = _check(plan_of("anti-affinity"), "anti-affinity", multi_node)
    batched, single, launches = st["phase_cycles"][:3]
    assert batched > 0 and single > 0 and batched + single == len(sims) and launches == _ceil(batched, 4) >= 4
    assert any(c is not None for c in cmds)


@pytest.mark.parametrize("multi_node", [False, True])
def test_reservations(plan_of, ov, multi_node):
    ov(general_launch=3)
    _, _, st = _check(plan_of("reservations"), "reservations", multi_node)
    assert st["phase_cycles"][2] >= 4


@pytest.mark.parametrize("general_batch", [0, 1])
def test_reserved_replacement(plan_of, ov, general_batch):
    """A replacement into a capacity reservation, batched and compiled on its own: the command's requirements carry the
    held reservation id."""
    ov(general_batch=general_batch)
    _, cmds, st = _check(plan_of("reserved-replacement"), "reserved-replacement", False)
    assert sum(st["phase_cycles"][:2]) == 1 and (general_batch == 0 or st["phase_cycles"][:2] == [0, 1])
    reqs = cmds[0]["nodeclaims"][0]["requirements"]
    assert [tuple(r) for r in reqs if r[0] == RID] == [(RID, "In", ["cr-m5.large-1a"], None)]


def test_budgets(plan_of):
    sims, cmds, st = _check(plan_of("spread-budgets"), "spread-budgets", True)
    blocked = [s for s in range(len(sims)) if sims[s]["n_pods"] == 0]
    assert 0 < len(blocked) < len(sims) and st["budget_blocked"] == len(blocked)
    assert all(cmds[s] is None for s in blocked) and any(c is not None for c in cmds)
    assert st["phase_cycles"][0] + st["phase_cycles"][1] == len(sims) - len(blocked)
