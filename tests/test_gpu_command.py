"""kp_cluster_command on plans of the batched simulation kernel: the command (replacement NodeClaim and placements) the
emitting sim_kernel instantiation leaves equals the reference of tests/command_ref.py in every field, with no
tolerance, and the per-subset results are those of kp_cluster_simulate_budgeted on the same plan, bit for bit."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import command_ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(d):
    """A kp_sim_result dict with its floats as their bit patterns."""
    return tuple(sorted((k, v.hex() if isinstance(v, float) else v) for k, v in d.items()))


def _check(plan, name, multi_node, subsets=None, want=None):
    """plan.command on a named case against the reference and against simulate() on the same plan."""
    cl, subs, _, allowed = command_ref.case(name)
    sims_w, cmds_w, _ = command_ref.expected(name, multi_node) if want is None else want
    subs = subs if subsets is None else subsets
    sims, cmds, st = plan.command(subs, multi_node=multi_node, allowed=allowed)
    assert sims == sims_w
    for s, (g, w) in enumerate(zip(cmds, cmds_w)):
        assert command_ref.command_fields(g) == command_ref.command_fields(w), f"{name} subset {s} {subs[s]}"
    plain, st2 = plan.simulate(subs, multi_node=multi_node, allowed=allowed)
    assert [_bits(d) for d in sims] == [_bits(d) for d in plain]  # out: bitwise kp_cluster_simulate_budgeted's
    if allowed is not None:
        assert st["budget_blocked"] == st2["budget_blocked"] == sum(c is None and s["n_pods"] == 0 for c, s in zip(cmds_w, sims_w))
    return sims, cmds, st


@pytest.fixture(scope="module")
def plans(ctx):
    import kpamd
    made = {}

    def get(name):
        if name not in made:
            made[name] = kpamd.ClusterPlan(ctx, command_ref.case(name)[0])
        return made[name]
    yield get
    for p in made.values():
        p.close()


@pytest.mark.parametrize("multi_node", [False, True])
def test_config4(plans, multi_node):
    """399 subsets at the production launch size: REPLACE commands keeping more than 64 options (both lane halves),
    options dropped from the middle of the price order, filterOutSameType dropping more, DELETEs, no-ops."""
    sims, cmds, st = _check(plans("config4"), "config4", multi_node)
    assert max(len(c["nodeclaims"][0]["options"]) for c in cmds if c and c["nodeclaims"]) > 64
    assert any(c is not None and not c["nodeclaims"] for c in cmds) and any(c is None for c in cmds)


@pytest.mark.parametrize("slots", [4, 28])
def test_config4_slot_reuse(plans, ov, slots):
    """sim_slots 4 and 28: one wave emits many commands in a row into its reused state."""
    ov(sim_slots=slots)
    _, _, st = _check(plans("config4"), "config4", True)
    assert st["phase_cycles"][1] == slots and st["phase_cycles"][2] > 1


def test_config4_order(plans, ov):
    """Reversed and shuffled subset orders (other waves, other predecessors in a wave's slot): the same command for
    every subset."""
    ov(sim_slots=28)
    cl, subs, _, _ = command_ref.case("config4")
    sims_w, cmds_w, infos = command_ref.expected("config4", True)
    for order in (list(range(len(subs)))[::-1], list(np.random.default_rng(9).permutation(len(subs)))):
        _check(plans("config4"), "config4", True, subsets=[subs[i] for i in order],
               want=([sims_w[i] for i in order], [cmds_w[i] for i in order], None))


@pytest.mark.parametrize("name", ["disruption-state", "spot-to-spot", "spot-to-spot-config4", "min-values"])
@pytest.mark.parametrize("multi_node", [False, True])
def test_cases(plans, name, multi_node):
    """Pending and deleting-node pods with binding limits (the placement index convention), the spot-to-spot gate with
    singletons (the cut to 15) and larger subsets, a NodePool with instance-family minValues 40."""
    _check(plans(name), name, multi_node)


def test_host_ports(plans):
    _check(plans("host-ports"), "host-ports", True)


def test_budgets(plans):
    """Budgets on the two-pool relabelling: a blocked subset has no command, n_blocked is the host's count."""
    sims, cmds, st = _check(plans("budgets"), "budgets", True)
    blocked = [s for s in range(len(sims)) if sims[s]["n_pods"] == 0]
    assert 0 < len(blocked) < len(sims) and st["budget_blocked"] == len(blocked)
    assert all(cmds[s] is None for s in blocked)
    # all unlimited, and no budgets at all: the same commands
    from kpamd.disruption import UNLIMITED
    cl, subs, _, _ = command_ref.case("budgets")
    a = plans("budgets").command(subs, allowed=[UNLIMITED, UNLIMITED])
    b = plans("budgets").command(subs)
    assert a[0] == b[0] and [command_ref.command_fields(c) for c in a[1]] == [command_ref.command_fields(c) for c in b[1]]
    assert a[2]["budget_blocked"] == 0 and any(c is not None for c in a[1])


def test_edges(ctx, plans):
    """One subset alone, no subsets, a call after a cancelled one, a stale plan, a subset naming a deleting node."""
    import kpamd
    from kpamd import abi
    cl, subs, _, _ = command_ref.case("config4")
    sims_w, cmds_w, _ = command_ref.expected("config4", True)
    plan = plans("config4")
    pick = next(s for s, c in enumerate(cmds_w) if c and c["nodeclaims"])
    sims, cmds, _ = plan.command([subs[pick]])
    assert sims == [sims_w[pick]] and command_ref.command_fields(cmds[0]) == command_ref.command_fields(cmds_w[pick])
    assert plan.command([])[:2] == ([], [])
    tok = kpamd.Cancel(ctx)
    try:
        tok.set()
        with pytest.raises(kpamd.KPError) as e:
            plan.command(subs[:40], cancel=tok)
        assert e.value.code == abi.KP_E_CANCELED
        tok.reset()
        sims, cmds, _ = plan.command(subs[:40], cancel=tok)  # the plan stays usable
    finally:
        tok.close()
    assert sims == sims_w[:40]
    assert [command_ref.command_fields(c) for c in cmds] == [command_ref.command_fields(c) for c in cmds_w[:40]]
    # a subset naming a node that is being deleted
    ds, ds_subs, _, _ = command_ref.case("disruption-state")
    deleting = next(i for i, n in enumerate(ds.nodes) if n.deleting)
    with pytest.raises(kpamd.KPError) as e:
        plans("disruption-state").command([ds_subs[0], [ds_subs[1][0], deleting]])
    assert e.value.code == abi.KP_E_INVAL and "subset 1" in str(e.value) and "deleted" in str(e.value)
    # a stale plan: the catalogue's seqnum moved since kp_cluster_prepare
    small = command_ref.case("min-values")[0]
    cat = kpamd.Catalog(ctx, copy.deepcopy(small.catalogs[0]), seqnum=1)
    p = kpamd.ClusterPlan(ctx, small, catalogs=[cat])
    try:
        p.command([[0]])
        t = next(i for i, it in enumerate(small.catalogs[0])
                 if any(o.capacity_type == "spot" and o.zone == "test-zone-1a" for o in it.offerings))
        cat.update_offerings([(t, "spot", "test-zone-1a", False)], seqnum=2)
        with pytest.raises(kpamd.KPError, match="stale plan"):
            p.command([[0]])
    finally:
        p.close()
        cat.close()
