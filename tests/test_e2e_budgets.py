"""The reference's disruption-budget scenarios (R:test/suites/consolidation/suite_test.go:184-486, Context "Budgets"),
transcribed over the cluster model of tests/e2e.py with the finalizer model of tests/e2e_budgets.py. Every scenario runs
on the oracle (CPU) and on the device (-m gpu); on the device the whole trajectory (launches, commands, waves, summary)
must also equal the oracle's."""
import calendar
import time

import pytest

import e2e
import e2e_budgets
from e2e import K

BACKENDS = ["oracle", pytest.param("device", marks=pytest.mark.gpu)]
SIZE = K + "instance-size"
NOW = calendar.timegm((2025, 6, 30, 23, 50, 17))  # UTC; the window of the scheduled scenario crosses midnight


@pytest.fixture
def mk(request, lib):
    envs = []

    def make(backend, **kw):
        ctx = request.getfixturevalue("ctx") if backend == "device" else None
        env = e2e_budgets.BudgetEnv(backend, lib, ctx=ctx, **kw)
        envs.append(env)
        return env
    yield make
    for env in envs:
        env.close()


def _cmds(cmds):
    return [(c.method, c.candidates, c.decision) for c in cmds]


def _twin(mk, backend, scenario):
    env = mk(backend)
    out = scenario(env)
    if backend == "device":
        ref = mk("oracle")
        want = scenario(ref)
        assert env.launches == ref.launches, (env.launches, ref.launches)
        assert _cmds(env.commands) == _cmds(ref.commands)
        assert [_cmds(w) for w in env.waves] == [_cmds(w) for w in ref.waves]
        assert env.summary() == ref.summary()
        assert out == want
    return env


def _pod(cpu_m, **kw):
    from kpamd.model import PodShape
    return PodShape({"pods": 1000, "cpu": cpu_m}, **kw)


def _five_nodes_four_empty(env, budgets):
    """The suite's BeforeEach Deployment (five one-CPU pods) with hostname anti-affinity: five nodes; scaled to 1."""
    from kpamd.model import LabelSelector, PodAffinityTerm
    pool = e2e.default_nodepool()
    pool.budgets = budgets
    env.pools = [pool]
    env.deploy("regular-app", _pod(1000, labels={"app": "regular-app"},
                                   required_anti_affinity=[PodAffinityTerm("kubernetes.io/hostname",
                                                                           LabelSelector({"app": "regular-app"}))]), 5)
    env.provision()
    assert not env.pending() and len(env.nodes) == 5, env.summary()
    env.scale("regular-app", 1)
    assert sum(1 for n in env.nodes if not env.pods_on(n)) == 4


def _assert_forty_percent(env, waves):
    """ConsistentlyExpectDisruptionsUntilNoneLeft(5, 2): never more than two nodes disrupting; one node is left."""
    assert [[(c.method, len(c.candidates), c.decision) for c in w] for w in waves] == \
        [[("emptiness", 2, 1)], [("emptiness", 2, 1)]], waves
    assert env.peak_held == 2
    assert len(env.nodes) == 1 and len(env.pods_on(next(iter(env.nodes)))) == 1


@pytest.mark.parametrize("backend", BACKENDS)
def test_budget_empty_delete(mk, backend):
    """:207-244 "should respect budgets for empty delete consolidation": nodes "40%" of five nodes lets two empty nodes
    go at a time."""
    from kpamd.model import Budget

    def scenario(env):
        _five_nodes_four_empty(env, [Budget("40%")])
        waves = env.consolidate_budgeted(now=NOW)
        _assert_forty_percent(env, waves)
        return env.summary()
    _twin(mk, backend, scenario)


@pytest.mark.parametrize("backend", BACKENDS)
def test_budget_non_empty_delete(mk, backend):
    """:245-304 "should respect budgets for non-empty delete consolidation": three 2xlarge nodes of three 2100m pods,
    one pod kept on each; nodes "50%" allows two of them, which one multi-node command deletes."""
    from kpamd.model import Budget

    def scenario(env):
        pool = e2e.default_nodepool()
        pool.requirements = pool.requirements + [(SIZE, "In", ["2xlarge"])]
        pool.budgets = [Budget("50%")]
        env.pools = [pool]
        env.deploy("large-app", _pod(2100, labels={"app": "large-app"}), 9)
        env.provision()
        assert not env.pending() and [len(env.pods_on(n)) for n in env.nodes] == [3, 3, 3], env.summary()
        env.keep_one_per_node("large-app")
        assert [len(env.pods_on(n)) for n in env.nodes] == [1, 1, 1]
        waves = env.consolidate_budgeted(now=NOW)
        assert [[(c.method, len(c.candidates), c.decision) for c in w] for w in waves] == [[("multi", 2, 1)]], waves
        assert env.peak_held == 2
        assert [len(env.pods_on(n)) for n in env.nodes] == [3] and not env.pending()
        return env.summary()
    _twin(mk, backend, scenario)


@pytest.mark.parametrize("backend", BACKENDS)
def test_budget_replace(mk, backend):
    """:305-419 "should respect budgets for non-empty replace consolidation": five 3-CPU pods, each pinned to its own
    test-partition, next to a 3-CPU daemonset: five 2xlarge nodes. Without the daemonset every node can be replaced by
    an xlarge; nodes "3" lets three replacements run at once (eight nodes at the peak), then the other two."""
    from kpamd.model import Budget

    def scenario(env):
        pool = e2e.default_nodepool()
        pool.requirements = pool.requirements + [(SIZE, "In", ["xlarge", "2xlarge"]), ("test-partition", "Exists", [])]
        pool.budgets = [Budget("3")]
        pool.daemon_requests = {"cpu": 3000}
        env.pools = [pool]
        for i in range(5):
            env.deploy(f"large-app-{i}", _pod(3000, labels={"app": "large-app"}, node_selector={"test-partition": str(i)}), 1)
        env.provision()
        assert not env.pending() and len(env.nodes) == 5, env.summary()
        assert all(env.type_of(n).endswith(".2xlarge") for n in env.nodes), env.summary()
        pool.daemon_requests = {}  # env.ExpectDeleted(ds)
        waves = env.consolidate_budgeted(now=NOW)
        assert [[(c.method, len(c.candidates), c.decision) for c in w] for w in waves] == \
            [[("single", 1, 2)] * 3, [("single", 1, 2)] * 2], waves
        assert env.peak_held == 3 and env.peak_nodes == 8
        assert len(env.nodes) == 5 and all(env.type_of(n).endswith(".xlarge") for n in env.nodes), env.summary()
        assert len(env.launches) == 10 and not env.pending()
        return env.summary()
    _twin(mk, backend, scenario)


@pytest.mark.parametrize("backend", BACKENDS)
def test_budget_fully_blocking(mk, backend):
    """:420-449 "should not allow consolidation if the budget is fully blocking": nodes "0"."""
    from kpamd.model import Budget

    def scenario(env):
        _five_nodes_four_empty(env, [Budget("0")])
        assert env.consolidate_budgeted(now=NOW) == []
        assert len(env.nodes) == 5 and not env.commands
        return env.summary()
    _twin(mk, backend, scenario)


@pytest.mark.parametrize("backend", BACKENDS)
def test_budget_blocking_during_a_scheduled_window(mk, backend):
    """:450-485 "... fully blocking during a scheduled time": nodes "0" on a schedule that fired 15 minutes ago and lasts
    30 minutes blocks everything now; once the window is over the NodePool's other budget ("40%") applies."""
    from kpamd.model import Budget

    def scenario(env):
        start = time.gmtime(NOW - 15 * 60)
        window = Budget("0", schedule=f"{start.tm_min} {start.tm_hour} * * *", duration_s=30 * 60)
        _five_nodes_four_empty(env, [window, Budget("40%")])
        assert env.consolidate_budgeted(now=NOW) == []
        assert env.consolidate_budgeted(now=NOW + 14 * 60) == []
        assert len(env.nodes) == 5 and not env.commands
        waves = env.consolidate_budgeted(now=NOW + 16 * 60)
        _assert_forty_percent(env, waves)
        return env.summary()
    _twin(mk, backend, scenario)
