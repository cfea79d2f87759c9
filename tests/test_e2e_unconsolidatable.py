"""The Unconsolidatable reasons at the fixed point of the reference's consolidation e2e scenarios (tests/e2e.py, as
tests/test_e2e_suites.py runs them): once the disruption controller finds nothing more to do, no remaining node's
singleton may still read "can be consolidated", the device says of every node what the oracle-backed plan
(why_ref.OracleWhyPlan) says, and the three .large nodes the replace scenario ends on read the documented
"can't replace with a lower-priced node" (R:website/content/en/preview/concepts/disruption.md:105-113)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import e2e  # noqa: E402
import why_ref  # noqa: E402
from e2e import CT, K, NOT_BURSTABLE  # noqa: E402

BACKENDS = ["oracle", pytest.param("device", marks=pytest.mark.gpu)]
SIZE = K + "instance-size"


@pytest.fixture
def mk(request, lib):
    envs = []

    def make(backend, **kw):
        ctx = request.getfixturevalue("ctx") if backend == "device" else None
        env = e2e.Env(backend, lib, ctx=ctx, **kw)
        envs.append(env)
        return env
    yield make
    for env in envs:
        env.close()


def _pod(cpu_m, **kw):
    from kpamd.model import PodShape
    return PodShape({"pods": 1000, "cpu": cpu_m}, **kw)


def _spread(app):
    from kpamd.model import LabelSelector, TopologySpread
    return TopologySpread("kubernetes.io/hostname", 1, LabelSelector({"app": app}), "DoNotSchedule", None)


def _entries(env):
    """unconsolidatable() at the environment's present state, on the oracle-backed plan and, for a device environment,
    on the device: the same entries, floats bit for bit."""
    from kpamd import disruption
    cl, names = env.cluster()
    want = disruption.unconsolidatable(cl, why_ref.OracleWhyPlan(cl))
    if env.backend == "device":
        plan = env._plan(cl)
        try:
            got = disruption.unconsolidatable(cl, plan)
        finally:
            plan.close()
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert (g["node"], g["candidate_reason"], g["detail"], g["pdb"]) == \
                (w["node"], w["candidate_reason"], w["detail"], w["pdb"])
            assert why_ref.bits(g["why"]) == why_ref.bits(w["why"]), (names[g["node"]], g["why"], w["why"])
            assert why_ref.bits(g["sim"]) == why_ref.bits(w["sim"])
    assert [e["node"] for e in want] == list(range(len(names)))  # every node of the scenario is managed
    return want, names


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("capacity_type", ["on-demand", "spot"])
def test_replace_fixed_point(mk, backend, capacity_type):
    """test_consolidation_replace's scenario: after its three replacements nothing is left to do, and each of the three
    .large nodes stays because no cheaper type holds its pod."""
    from kpamd import disruption
    from kpamd.model import NodePool
    env = mk(backend)
    env.pools = [NodePool("default", 0, 0, [(CT, "In", [capacity_type]), (SIZE, "In", ["large", "2xlarge"]),
                                            NOT_BURSTABLE, ("kubernetes.io/os", "In", ["linux"])])]
    env.deploy("large-app", _pod(4000, labels={"app": "large-app"}, topology_spread=[_spread("large-app")]), 3)
    env.deploy("small-app", _pod(1800, labels={"app": "small-app"}, topology_spread=[_spread("small-app")]), 3)
    env.provision()
    env.scale("large-app", 0)
    assert len(env.consolidate()) == 3
    entries, names = _entries(env)
    assert len(entries) == 3 and all(env.type_of(n).endswith(".large") for n in names)
    for e in entries:
        assert e["why"]["reason"] == why_ref.NOT_CHEAPER, e
        assert disruption.unconsolidatable_message(e) == "can't replace with a lower-priced node"


@pytest.mark.parametrize("backend", BACKENDS)
def test_delete_fixed_point(mk, backend):
    """test_consolidation_delete's scenario with a random scale-down: after multi-node consolidation has packed the
    nodes, no remaining node's singleton can be deleted or replaced, and every one of them says why."""
    from kpamd import disruption
    from kpamd.model import NodePool
    env = mk(backend)
    env.pools = [NodePool("default", 0, 0, [(CT, "In", ["on-demand"]), (SIZE, "In", ["medium", "large", "xlarge"]),
                                            NOT_BURSTABLE])]
    env.deploy("large-app", _pod(1000, labels={"app": "large-app"}), 100)
    env.provision()
    env.scale("large-app", 40, seed=1)
    assert env.consolidate()
    entries, names = _entries(env)
    assert entries
    for e in entries:
        assert e["candidate_reason"] == 0 and e["why"]["reason"] != why_ref.NONE, (names[e["node"]], e)
        assert disruption.unconsolidatable_message(e)
