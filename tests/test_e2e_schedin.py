"""One provisioning scenario (tests/scenarios.py) and one consolidation scenario (tests/e2e.py) with two daemonsets,
the scheduler's inputs computed by kp_scheduler_inputs (backend "device") or by the plain-Python reference (backend
"oracle") before every Solve and every consolidation pass.

  node-agent   150m, no toleration: the tainted NodePool "infra" does not take it, "default" does
  zone-agent   100m, tolerates everything, nodeSelector zone test-zone-1a: both templates count it (the zone is a
               well-known label a template leaves undefined: R:website/content/en/preview/faq.md:105-108), a node
               runs it only in that zone

The kube-scheduler half of the model binds, on every new node, one pod of each daemonset compatible with the node.
Both backends must give equal trajectories, and every NodeClaim's requests are its pods' plus exactly the overhead of
the daemonsets compatible with its NodePool's template: 250m on "default", 100m on "infra"."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import e2e  # noqa: E402
import scenarios  # noqa: E402
import schedin_ref as ref  # noqa: E402
from e2e import CT, NOT_BURSTABLE, POOL, ZONE, K  # noqa: E402

BACKENDS = ["oracle", pytest.param("device", marks=pytest.mark.gpu)]
SIZE = K + "instance-size"
INFRA = ("dedicated", "infra", "NoSchedule")
OVERHEAD = {"default": {"cpu": 250, "pods": 2000}, "infra": {"cpu": 100, "pods": 1000}}


def daemonsets():
    from kpamd.model import PodShape
    return [PodShape({"cpu": 150, "pods": 1000}),
            PodShape({"cpu": 100, "pods": 1000}, node_selector={ZONE: "test-zone-1a"}, tolerations=[("", "Exists", "", "")])]


def pools(sizes):
    from kpamd.model import NodePool
    base = [(CT, "In", ["on-demand"]), (SIZE, "In", sizes), NOT_BURSTABLE, ("kubernetes.io/os", "In", ["linux"])]
    return [NodePool("default", 0, 0, list(base), limits={"cpu": 400000}),
            NodePool("infra", 0, 0, list(base), taints=[INFRA])]


def workloads():
    from kpamd.model import PodShape
    return [PodShape({"cpu": 1000, "pods": 1000}, labels={"app": "app"}),
            PodShape({"cpu": 500, "pods": 1000}, labels={"app": "infra-app"}, node_selector={POOL: "infra"},
                     tolerations=[("dedicated", "Equal", "infra", "NoSchedule")])]


def inputs(env, state):
    """the four tables from the backend under test"""
    if env.backend == "device":
        return env.ctx.scheduler_inputs(state).apply
    return lambda target: ref.apply(state, target)


def check_overhead(env, res, prob):
    for nc in res["nodeclaims"]:
        want = dict(OVERHEAD[prob.nodepools[nc["nodepool"]].name])
        for p in nc["pods"]:
            for k, v in prob.shapes[int(prob.pod_shape[p])].requests.items():
                want[k] = want.get(k, 0) + v
        assert nc["requests"] == want, (env.backend, nc["requests"], want)
        env.checked += 1


class ProvisioningEnv(scenarios.Env):
    """scenarios.Env whose Solve takes its NodePool inputs from kp_scheduler_inputs (no node exists yet)"""
    checked = 0

    def _solve(self, prob):
        from kpamd.model import SchedulerState
        prob.nodepools = copy.deepcopy(prob.nodepools)
        inputs(self, SchedulerState(copy.deepcopy(prob.nodepools), daemonsets(), []))(prob)
        assert [p.daemon_requests for p in prob.nodepools] == [OVERHEAD["default"], OVERHEAD["infra"]]
        assert prob.nodepools[0].limits == {"cpu": 400000} and prob.nodepools[1].limits == {}
        res = super()._solve(prob)
        check_overhead(self, res, prob)
        return res


class DaemonEnv(e2e.Env):
    """e2e.Env with daemonsets: the state of every Solve and of every consolidation snapshot goes through
    kp_scheduler_inputs; a new node gets its daemonset pods bound at once"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.daemon_pods = {}   # node name -> the requests of the daemonset pods bound to it
        self.checked = 0

    def _create(self, reqs, requests, options, pool):
        name = super()._create(reqs, requests, options, pool)
        if name is not None:
            labels, taints = self.labels(name), list(self.pools[pool].taints)
            self.daemon_pods[name] = [d.requests for d in daemonsets() if ref.node_compatible(d, labels, taints)]
        return name

    def state(self, names, existing):
        from kpamd.model import SchedNode, SchedulerState
        nodes = []
        for name, e in zip(names, existing):
            it = self.types()[self.nodes[name]["type"]]
            bound = [(self.shapes[self.pod_shape[p]].requests, False) for p in self.pods_on(name)]
            bound += [(r, True) for r in self.daemon_pods[name]]
            nodes.append(SchedNode(name, dict(e.labels), list(e.taints), it.allocatable(), dict(it.capacity), bound))
        return SchedulerState(copy.deepcopy(self.pools), daemonsets(), nodes)

    def _solve(self, pods, names):
        from kpamd.model import Problem
        existing, bound = self._existing(names)
        prob = Problem([self.types()], copy.deepcopy(self.pools), self.shapes,
                       np.array([self.pod_shape[p] for p in pods], np.uint32),
                       np.array([self.pod_created[p] for p in pods], np.int64),
                       np.array([p + 1 for p in pods], np.uint64), existing=existing, bound_pods=bound,
                       name="e2e-daemonsets", reserved_offering_mode=1)
        inputs(self, self.state(names, existing))(prob)
        for n in prob.existing:   # every expected daemonset pod is bound: nothing remains to reserve
            assert all(v == 0 for v in n.requests.values()), n
        if self.backend == "device":
            import kpamd
            self.types()
            res = kpamd.Scheduler(self.ctx, prob, catalogs=[self._cat]).solve()
        else:
            from oracle import pyoracle
            res = pyoracle.solve(prob)
        check_overhead(self, res, prob)
        return res

    def cluster(self):
        cl, names = super().cluster()
        cl.nodepools = copy.deepcopy(cl.nodepools)
        inputs(self, self.state(names, [n.node for n in cl.nodes]))(cl)
        return cl, names


@pytest.fixture
def mk(request, lib):
    envs = []

    def make(cls, backend, *a, **kw):
        ctx = request.getfixturevalue("ctx") if backend == "device" else None
        env = cls(backend, *a, ctx=ctx, **kw)
        envs.append(env)
        return env
    yield make
    for env in envs:
        env.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_provisioning_carries_the_overhead(mk, lib, backend):
    """ExpectProvisioned of 12 app pods and 5 infra pods on the fake catalogue: the NodeClaims of "default" carry 250m,
    those of "infra" 100m, and the device's launches are the oracle's"""
    def scenario(env):
        nodes, pod_node = env.provision(pools(["large", "xlarge", "2xlarge"]), workloads(), [12, 5])
        assert all(n is not None for n in pod_node)
        assert env.checked >= 2
        return [(n["type"], n["zone"], n["capacity_type"], n["pods"]) for n in nodes]
    out = scenario(mk(ProvisioningEnv, backend, scenarios.fake_catalog(lib)))
    if backend == "device":
        assert out == scenario(mk(ProvisioningEnv, "oracle", scenarios.fake_catalog(lib)))


@pytest.mark.parametrize("backend", BACKENDS)
def test_consolidation_with_daemonsets(mk, lib, backend):
    """The consolidation suite's delete scenario with the two daemonsets: 40 app pods and 6 infra pods provisioned,
    the Deployment scaled to 12, consolidation raises the utilization; every Solve on the way (the provisioner's and
    each command's) carries the overhead"""
    def scenario(env):
        env.pools = pools(["medium", "large", "xlarge"])
        app, infra = workloads()
        env.deploy("app", app, 40)
        env.deploy("infra-app", infra, 6)
        env.provision()
        assert not env.pending()
        assert {v["pool"] for v in env.nodes.values()} == {0, 1}
        env.scale("app", 12, seed=2)
        low = env.utilization()
        cmds = env.consolidate()
        assert cmds and not env.pending()
        assert env.utilization() > low
        assert env.checked >= 2
        return round(low, 6), round(env.utilization(), 6), len(env.nodes)
    env = mk(DaemonEnv, backend, lib)
    out = scenario(env)
    if backend == "device":
        twin = mk(DaemonEnv, "oracle", lib)
        assert out == scenario(twin)
        assert env.launches == twin.launches
        assert [(c.method, c.candidates, c.decision) for c in env.commands] == \
            [(c.method, c.candidates, c.decision) for c in twin.commands]
        assert env.summary() == twin.summary()
