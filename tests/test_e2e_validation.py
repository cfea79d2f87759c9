"""The e2e consolidation scenarios with every command validated against a fresh snapshot before it is applied
(tests/e2e_validation.py). Without churn a validated loop gives the trajectory the suites give today and every command
validates; with churn between compute and apply the command is rejected, not applied, and the next pass recomputes.
The device and the oracle must agree on every trajectory and every verdict."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import e2e  # noqa: E402
import test_e2e_suites as suites  # noqa: E402
from e2e import CT, NOT_BURSTABLE  # noqa: E402
from e2e_validation import ValidatingEnv  # noqa: E402
from test_e2e_commands import _trajectory  # noqa: E402
from test_e2e_suites import SIZE, _pod, _spread  # noqa: E402

BACKENDS = ["oracle", pytest.param("device", marks=pytest.mark.gpu)]


@pytest.fixture
def envs(request, lib):
    made = []

    def make(cls, backend, **kw):
        env = cls(backend, lib, ctx=request.getfixturevalue("ctx") if backend == "device" else None, **kw)
        made.append(env)
        return env
    yield make
    for env in made:
        env.close()


# ---- no churn --------------------------------------------------------------------------------------------------------
def _unchanged(envs, backend, test, *params):
    """One consolidation scenario of tests/test_e2e_suites.py over ValidatingEnv (its _twin: on the device also on the
    oracle), then over the plain e2e.Env on the oracle: equal trajectories, and every command validated."""
    made = {"val": [], "plain": []}

    def maker(kind, cls):
        def make(b, **kw):
            made[kind].append(envs(cls, b, **kw))
            return made[kind][-1]
        return make
    test(maker("val", ValidatingEnv), backend, *params)
    test(maker("plain", e2e.Env), "oracle", *params)
    want = _trajectory(made["plain"][0])
    assert want[1], "the scenario applied no command"
    for env in made["val"]:
        assert _trajectory(env) == want, env.backend
        assert len(env.validations) == len(env.commands) and all(v[3] for v in env.validations), env.validations
        assert not env.rejected
    assert len({tuple(map(repr, env.validations)) for env in made["val"]}) == 1
    assert any(c.method != "emptiness" for env in made["val"] for c in env.commands)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("capacity_type", ["on-demand", "spot"])
def test_delete(envs, backend, capacity_type):
    _unchanged(envs, backend, suites.test_consolidation_delete, capacity_type, 1)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("capacity_type", ["on-demand", "spot"])
def test_replace(envs, backend, capacity_type):
    _unchanged(envs, backend, suites.test_consolidation_replace, capacity_type)


@pytest.mark.parametrize("backend", BACKENDS)
def test_on_demand_to_spot(envs, backend):
    _unchanged(envs, backend, suites.test_consolidation_on_demand_to_spot)


@pytest.mark.parametrize("backend", BACKENDS)
def test_into_a_reservation(envs, backend):
    _unchanged(envs, backend, suites.test_consolidation_into_a_reservation)


@pytest.mark.parametrize("backend", BACKENDS)
def test_between_reservations(envs, backend):
    _unchanged(envs, backend, suites.test_consolidation_between_reservations)


# ---- churn between compute and apply ---------------------------------------------------------------------------------
def _delete_setup(env, replicas=40):
    """test_consolidation_delete's start: 100 one-CPU pods, scaled down at random (partly used nodes). At 40 replicas
    the multi-node command is a REPLACE, at 30 a DELETE."""
    from kpamd.model import NodePool
    env.pools = [NodePool("default", 0, 0, [(CT, "In", ["on-demand"]), (SIZE, "In", ["medium", "large", "xlarge"]), NOT_BURSTABLE])]
    env.deploy("large-app", _pod(1000, labels={"app": "large-app"}), 100)
    env.provision()
    env.scale("large-app", replicas, seed=1)


def _replace_setup(env, budgets=None):
    """test_consolidation_replace's start: three nodes left with one 1.8-CPU pod each (hostname spread)."""
    from kpamd.model import NodePool
    env.pools = [NodePool("default", 0, 0, [(CT, "In", ["on-demand"]), (SIZE, "In", ["large", "2xlarge"]), NOT_BURSTABLE,
                                            ("kubernetes.io/os", "In", ["linux"])], budgets=budgets)]
    env.deploy("large-app", _pod(4000, labels={"app": "large-app"}, topology_spread=[_spread("kubernetes.io/hostname", "large-app")]), 3)
    env.deploy("small-app", _pod(1800, labels={"app": "small-app"}, topology_spread=[_spread("kubernetes.io/hostname", "small-app")]), 3)
    env.provision()
    env.scale("large-app", 0)


def _churned(envs, backend, setup, churn, **setup_kw):
    """setup + consolidate(churn) on the backend (on the device also on the oracle: equal trajectories and verdicts).
    Returns the backend's env and what the churn noted."""
    runs = []
    for b in ([backend, "oracle"] if backend == "device" else [backend]):
        env = envs(ValidatingEnv, b)
        setup(env, **setup_kw)
        notes = {}
        env.consolidate(churn=lambda e, cl, names, cmd: churn(e, cl, names, cmd, notes))
        assert notes, "the churn never acted"
        assert len(env.rejected) >= 1 and env.rejected[0] is notes["cmd"]
        assert all(c is not notes["cmd"] for c in env.commands)  # the rejected command was not applied
        assert not env.pending() and not env.deleting
        runs.append((env, notes))
    if len(runs) == 2:
        assert _trajectory(runs[0][0]) == _trajectory(runs[1][0])
        assert runs[0][0].validations == runs[1][0].validations
    return runs[0]


@pytest.mark.parametrize("backend", BACKENDS)
def test_scale_up_invalidates_a_delete(envs, backend):
    """A multi-node DELETE is computed; the Deployment scales up before it is applied: the simulation on the new
    snapshot needs new capacity, the command is rejected and its nodes stay."""
    def churn(env, cl, names, cmd, notes):
        if cmd.method == "emptiness" or cmd.decision != 1:
            return None
        notes.update(cmd=cmd, cands=[names[c] for c in cmd.candidates], nodes=set(env.nodes))
        env.scale("large-app", 70)
        return lambda: None
    env, notes = _churned(envs, backend, _delete_setup, churn, replicas=30)
    k = next(i for i, v in enumerate(env.validations) if not v[3])
    assert env.validations[k][1] == notes["cands"]
    assert env.validations[k][4] == "multiple"  # the 40 new pods need more than one NodeClaim
    assert len([p for p in range(len(env.alive)) if env.alive[p]]) == 70


@pytest.mark.parametrize("backend", BACKENDS)
def test_ice_on_the_cheapest_option(envs, backend):
    """A single-node REPLACE is computed; its cheapest option goes ICE before the launch: NOT_SUBSET, and the next
    pass recomputes the replacement without that option."""
    def churn(env, cl, names, cmd, notes):
        if cmd.decision != 2:
            return None
        nc, = cmd.result["replacements"]
        it = env.types()[nc["options"][0]]
        notes.update(cmd=cmd, name=it.name, at=len(env.validations))
        env.ice |= {(it.name, o.capacity_type, o.zone) for o in it.offerings}
        return lambda: None
    env, notes = _churned(envs, backend, _replace_setup, churn)
    at = notes["at"]
    assert env.validations[at][3:] == (False, "not-subset")
    assert env.validations[at + 1][3] and env.validations[at + 1][1] == env.validations[at][1]  # recomputed, same candidate
    nxt = env.commands[[v[3] for v in env.validations[:at + 2]].count(True) - 1]
    names = [env.types()[t].name for t in nxt.result["replacements"][0]["options"]]
    assert names and notes["name"] not in names
    assert all(t != notes["name"] for _, t, *_ in env.launches[-3:])


@pytest.mark.parametrize("backend", BACKENDS)
def test_candidate_marked_for_deletion(envs, backend):
    """A candidate of a computed command is marked for deletion meanwhile: rejected before any simulation."""
    def churn(env, cl, names, cmd, notes):
        if cmd.method == "emptiness":
            return None
        victim = names[cmd.candidates[0]]
        notes.update(cmd=cmd, victim=victim)
        env.deleting.add(victim)
        return lambda: env.finish_deletion(victim)
    env, notes = _churned(envs, backend, _delete_setup, churn)
    bad = next(v for v in env.validations if not v[3])
    assert bad[4] == f"candidate {notes['victim']} is marked for deletion"
    assert notes["victim"] not in env.nodes


@pytest.mark.parametrize("backend", BACKENDS)
def test_budget_consumed_meanwhile(envs, backend):
    """The NodePool allows one disruption; another of its nodes starts terminating after the command was computed: the
    walk over the command's candidates finds the allowance used up."""
    from kpamd.model import Budget

    def churn(env, cl, names, cmd, notes):
        if cmd.decision != 2:
            return None
        other = next(n for n in names if n not in [names[c] for c in cmd.candidates])
        notes.update(cmd=cmd, other=other)
        env.deleting.add(other)
        return lambda: env.finish_deletion(other)
    env, notes = _churned(envs, backend, _replace_setup, churn, budgets=[Budget("1")])
    bad = next(v for v in env.validations if not v[3])
    assert "budget" in bad[4]
