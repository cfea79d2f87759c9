"""Drift end to end over the cluster model of tests/e2e.py, extended here (DriftEnv) with a Drifted condition per node
and a Drift command's application: every replacement NodeClaim of the command is launched, the old node goes, its pods
move where the command's Solve put them. Every scenario runs on the oracle (CPU) and on the device (-m gpu); on the
device the whole trajectory (every node launched, every command) must equal the oracle's.

R:test/suites/drift/suite_test.go:93-113 is the reference's statement: one pod on one node, the node drifts, one
replacement NodeClaim is launched, the old node goes and the pod is healthy on the new node. Budgets:
R:website/content/en/preview/concepts/disruption.md:274-333."""
import pytest

import e2e
from e2e import CT, NOT_BURSTABLE

BACKENDS = ["oracle", pytest.param("device", marks=pytest.mark.gpu)]


class DriftEnv(e2e.Env):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.drifted = {}  # node name -> transition time of its Drifted condition

    def drift(self, name):
        self.drifted[name] = float(self.clock)
        self.clock += 1

    def cluster(self):
        cl, names = super().cluster()
        for node, name in zip(cl.nodes, names):
            node.drifted = self.drifted.get(name)
        return cl, names

    def _plan(self, cl):
        if self.backend == "device":
            return super()._plan(cl)
        import drift_ref
        return drift_ref.OracleDriftPlan(cl)

    def _apply(self, cl, names, cmd):
        if cmd.method != "drift":
            return super()._apply(cl, names, cmd)
        cands = [names[c] for c in cmd.candidates]
        # the command's simulation queued the pending pods, then the candidates' pods (no node is being deleted here)
        moving = self.pending() + [p for n in cands for p in self.pods_on(n)]
        others = [n for n in names if n not in cands]
        placement = cmd.result.get("placement")
        new = []
        for nc in cmd.result["replacements"]:
            name = self._create(nc["requirements"], nc["requests"], nc["options"], nc["nodepool"])
            assert name is not None, "replacement launch failed"
            new.append(name)
        if placement is not None:
            assert len(placement) == len(moving)
            for i, pl in enumerate(placement):
                pl = int(pl)
                self.pod_node[moving[i]] = others[-2 - pl] if pl <= -2 else (new[pl] if pl >= 0 else None)
        for n in cands:
            del self.nodes[n]
            self.drifted.pop(n, None)


@pytest.fixture
def mk(request, lib):
    envs = []

    def make(backend, **kw):
        ctx = request.getfixturevalue("ctx") if backend == "device" else None
        env = DriftEnv(backend, lib, ctx=ctx, **kw)
        envs.append(env)
        return env
    yield make
    for env in envs:
        env.close()


def _twin(mk, backend, scenario):
    env = mk(backend)
    out = scenario(env)
    if backend == "device":
        ref = mk("oracle")
        want = scenario(ref)
        assert env.launches == ref.launches, (env.launches, ref.launches)
        assert [(c.method, c.candidates, c.decision) for c in env.commands] == \
            [(c.method, c.candidates, c.decision) for c in ref.commands]
        assert env.summary() == ref.summary()
        assert out == want
    return env


def _pool(budget=None):
    from kpamd.model import Budget, NodePool
    p = NodePool("default", 0, 0, [(CT, "In", ["on-demand"]), NOT_BURSTABLE])
    if budget is not None:
        p.budgets = [Budget(budget)]
    return p


def _pod(cpu_m, **kw):
    from kpamd.model import PodShape
    return PodShape({"pods": 1000, "cpu": cpu_m}, **kw)


def _passes(env, max_passes=8):
    """One command per pass until the controller finds nothing; the commands."""
    from kpamd import disruption
    done = []
    for _ in range(max_passes):
        cl, names = env.cluster()
        plan = env._plan(cl)
        try:
            cmd = disruption.Controller().compute_command(cl, plan)
        finally:
            plan.close()
        if cmd is None:
            return done
        env._apply(cl, names, cmd)
        env.commands.append(cmd)
        done.append((cmd.method, [names[c] for c in cmd.candidates], cmd.decision, len(cmd.result.get("replacements", []))))
    raise AssertionError(f"no fixed point after {max_passes} passes: {done}")


@pytest.mark.parametrize("backend", BACKENDS)
def test_drifted_node_is_replaced(mk, backend):
    """:93-113: one pod on one node; the node drifts; one replacement NodeClaim is launched, the old node goes, the pod
    is healthy on the new node."""
    from kpamd import disruption

    def scenario(env):
        env.pools = [_pool()]
        env.deploy("app", _pod(1000, labels={"app": "app"}), 1)
        env.provision()
        (old,) = list(env.nodes)
        env.drift(old)
        done = _passes(env)
        assert done == [("drift", [old], disruption.REPLACE, 1)]
        (new,) = list(env.nodes)
        assert new != old and len(env.launches) == 2 and not env.pending()
        assert [env.pod_node[p] for p in range(len(env.pod_shape)) if env.alive[p]] == [new]
        return done, env.summary()
    _twin(mk, backend, scenario)


@pytest.mark.parametrize("backend", BACKENDS)
def test_three_drifted_nodes_under_a_budget_of_one(mk, backend):
    """Budget("1"): one node is replaced per pass, oldest first; the fixed point after three passes."""
    from kpamd import disruption
    from kpamd.model import LabelSelector, TopologySpread

    def scenario(env):
        env.pools = [_pool("1")]
        host = TopologySpread("kubernetes.io/hostname", 1, LabelSelector({"app": "app"}), "DoNotSchedule")
        env.deploy("app", _pod(1000, labels={"app": "app"}, topology_spread=[host]), 3)
        env.provision()
        old = list(env.nodes)
        assert len(old) == 3
        for n in (old[2], old[0], old[1]):  # drift order is the conditions' age, not the node order
            env.drift(n)
        done = _passes(env)
        assert [(m, c, d) for m, c, d, _ in done] == [("drift", [n], disruption.REPLACE) for n in (old[2], old[0], old[1])]
        assert all(r == 1 for *_, r in done)
        assert len(env.nodes) == 3 and not set(old) & set(env.nodes) and not env.pending()
        return done, env.summary()
    _twin(mk, backend, scenario)


@pytest.mark.parametrize("backend", BACKENDS)
def test_empty_drifted_node_is_deleted(mk, backend):
    """An empty drifted node goes by one command with no launch. The controller's Emptiness comes first and takes an
    empty node whether it drifted or not; Drift's own empty-candidate command is the same command (checked directly)."""
    from kpamd import disruption

    def scenario(env):
        env.pools = [_pool()]
        env.deploy("app", _pod(1000, labels={"app": "app"}), 1)
        env.provision()
        (old,) = list(env.nodes)
        env.scale("app", 0)
        env.drift(old)
        cl, names = env.cluster()
        plan = env._plan(cl)
        try:
            own = disruption.Drift().compute_command(cl, plan)
        finally:
            plan.close()
        assert (own.method, [names[c] for c in own.candidates], own.decision, own.result["replacements"]) == \
            ("drift", [old], disruption.DELETE, [])
        n_launch = len(env.launches)
        done = _passes(env)
        assert len(done) == 1 and done[0][1] == [old] and done[0][2] == disruption.DELETE
        assert not env.nodes and len(env.launches) == n_launch
        return done, env.summary()
    _twin(mk, backend, scenario)
