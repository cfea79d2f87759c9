"""The consolidation scenarios of tests/test_e2e_suites.py with commands applied straight from what the plan returns:
an Env whose _apply launches the replacement from Command.result["replacements"] and binds the pods from
Command.result["placement"] (disruption.Controller(materialize=True), ClusterPlan.command), with no second Solve and
no Python restatement of the price filters. On both backends every launch and every command must equal the trajectory
the re-deriving e2e.Env._apply produces; on the device each command is served by one command call."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import command_ref  # noqa: E402
import e2e  # noqa: E402
import test_e2e_suites as suites  # noqa: E402

BACKENDS = ["oracle", pytest.param("device", marks=pytest.mark.gpu)]


class _Counting:
    """A plan that counts the calls made on it."""

    def __init__(self, plan, calls):
        self.plan, self.calls = plan, calls

    def simulate(self, *a, **kw):
        self.calls.append("simulate")
        return self.plan.simulate(*a, **kw)

    def command(self, subsets, **kw):
        self.calls.append(("command", len(subsets)))
        return self.plan.command(subsets, **kw)

    def close(self):
        self.plan.close()


class CommandEnv(e2e.Env):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.consolidating = False
        self.plan_calls = []  # per compute_command pass: the calls made on its plan

    def _plan(self, cl):
        calls = []
        self.plan_calls.append(calls)
        return _Counting(super()._plan(cl) if self.backend == "device" else command_ref.OracleCommandPlan(cl), calls)

    def _solve(self, pods, names):
        assert not self.consolidating, "a command was applied through a second Solve"
        return super()._solve(pods, names)

    def consolidate(self, max_commands=64):
        from kpamd import disruption
        done = []
        self.consolidating = True
        try:
            for _ in range(max_commands):
                cl, names = self.cluster()
                plan = self._plan(cl)
                try:
                    cmd = disruption.Controller(materialize=True).compute_command(cl, plan)
                finally:
                    plan.close()
                if cmd is None:
                    return done
                if cmd.method != "emptiness":  # one command call, of the winner alone
                    assert [c for c in self.plan_calls[-1] if c != "simulate"] == [("command", 1)], self.plan_calls[-1]
                self._apply(cl, names, cmd)
                done.append(cmd)
                self.commands.append(cmd)
        finally:
            self.consolidating = False
        raise AssertionError(f"consolidation did not settle after {max_commands} commands: {done[-4:]}")

    def _apply(self, cl, names, cmd):
        from kpamd import disruption
        cands = [names[c] for c in cmd.candidates]
        if cmd.method == "emptiness":
            for n in cands:
                del self.nodes[n]
            return
        alive = [p for p in range(len(self.pod_shape)) if self.alive[p]]  # cluster pod index -> pod (Env.cluster)
        moving = [alive[p] for p in cl.pending] + [alive[p] for c in cmd.candidates for p in cl.nodes[c].pods]
        others = [n for n in names if n not in cands]
        placement = cmd.result["placement"]
        assert len(placement) == len(moving)
        new = None
        if cmd.decision == disruption.REPLACE:
            nc, = cmd.result["replacements"]
            assert len(nc["options"]) == cmd.result["n_options"] > 0
            new = self._create(nc["requirements"], nc["requests"], nc["options"], nc["nodepool"])
            assert new is not None, "replacement launch failed"
        else:
            assert cmd.result["replacements"] == []
        for p, pl in zip(moving, placement):
            pl = int(pl)
            self.pod_node[p] = others[-2 - pl] if pl <= -2 else new if pl >= 0 else None
        for n in cands:
            del self.nodes[n]


def _trajectory(env):
    """Every launch (requirements as a sorted set of (key, op, values, minValues), whatever tuple form they came in),
    every command, and the nodes that remain."""
    launches = [(name, t, z, ct, sorted((r[0], r[1], tuple(r[2]), r[3] if len(r) > 3 else None) for r in reqs))
                for name, t, z, ct, reqs in env.launches]
    return launches, [(c.method, c.candidates, c.decision) for c in env.commands], env.summary()


def _run(request, lib, backend, test, *params):
    """Run one scenario of tests/test_e2e_suites.py (its _twin: on the device also on the oracle, equal trajectories)
    over CommandEnv, then over the re-deriving e2e.Env on the oracle; all trajectories must be equal."""
    made = {"cmd": [], "plain": []}

    def maker(kind, cls):
        def make(b, **kw):
            env = cls(b, lib, ctx=request.getfixturevalue("ctx") if b == "device" else None, **kw)
            made[kind].append(env)
            return env
        return make
    try:
        test(maker("cmd", CommandEnv), backend, *params)
        test(maker("plain", e2e.Env), "oracle", *params)
        want = _trajectory(made["plain"][0])
        assert want[1], "the scenario applied no command"
        for env in made["cmd"]:
            assert _trajectory(env) == want, env.backend
        assert any(c.method != "emptiness" for env in made["cmd"] for c in env.commands)
    finally:
        for envs in made.values():
            for env in envs:
                env.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("capacity_type", ["on-demand", "spot"])
def test_delete(request, lib, backend, capacity_type):
    """A random scale-down leaves partly used nodes: multi-node DELETE commands, pods bound from the placements."""
    _run(request, lib, backend, suites.test_consolidation_delete, capacity_type, 1)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("capacity_type", ["on-demand", "spot"])
def test_replace(request, lib, backend, capacity_type):
    """Single-node REPLACE commands (spot: spot-to-spot, 15 options, capacity-type narrowed to spot)."""
    _run(request, lib, backend, suites.test_consolidation_replace, capacity_type)


@pytest.mark.parametrize("backend", BACKENDS)
def test_on_demand_to_spot(request, lib, backend):
    _run(request, lib, backend, suites.test_consolidation_on_demand_to_spot)


@pytest.mark.parametrize("backend", BACKENDS)
def test_into_a_reservation(request, lib, backend):
    _run(request, lib, backend, suites.test_consolidation_into_a_reservation)


@pytest.mark.parametrize("backend", BACKENDS)
def test_between_reservations(request, lib, backend):
    _run(request, lib, backend, suites.test_consolidation_between_reservations)
