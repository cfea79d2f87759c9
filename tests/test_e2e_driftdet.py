"""Drift detection end to end over the cluster model of tests/e2e.py and the Drift commands of tests/test_e2e_drift.py
(DriftEnv), extended here with an EC2NodeClass status and an instance per node: the model launches each node with the
AMI its type maps to (types without one are not launched, as the launch path's resolver drops them), a subnet of its
zone and the nodeclass's security groups. In every scenario the nodeclass status changes, detect_drift marks the
nodes, and the controller replaces them under the default budget (10%) until a fixed point, where no node is drifted
and every node carries the new value. Every scenario runs on the oracle-backed plan with the reference detection
(tests/driftdet_ref.py) and on the device (-m gpu); on the device the whole trajectory must equal the oracle's.

The reference's statements: R:test/suites/drift/suite_test.go:93-113 (AMI), :151-171 (the AMI no longer matches the
type), :172-245 (security group), :246-266 (subnet), :453-474 (the reservation is no longer selected)."""
import pytest

import drift_ref
import driftdet_ref
import test_e2e_drift as base
from e2e import CT, NOT_BURSTABLE

BACKENDS = base.BACKENDS
ARCH = "kubernetes.io/arch"


class RefDetectPlan(drift_ref.OracleDriftPlan):
    """The oracle's simulations and the reference's detection, in the device's record format"""

    def detect_drift(self, inputs=None, records=True):
        import numpy as np
        from kpamd import abi
        recs, counts = driftdet_ref.detect(self.cluster, inputs)
        out = np.zeros(len(recs), dtype=abi.node_drift_dtype())
        for i, r in enumerate(recs):
            out[i] = (*r, 0)
        return (out if records else None), counts, {}


class DetectEnv(base.DriftEnv):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        from kpamd.model import AMI, NodeClassStatus
        zones = list(self.cmod.ZONES)
        self.nodeclass = NodeClassStatus([AMI("ami-amd64-v1", [(ARCH, "In", ["amd64"])]), AMI("ami-arm64-v1", [(ARCH, "In", ["arm64"])])],
                                         [f"subnet-{z}" for z in zones], ["sg-a", "sg-b"], [c for c in self.crs],
                                         "class-hash", "v1")
        self.instances = {}   # node name -> NodeDrift (its annotations at launch and its instance)
        self.records = []     # the detection's records of every pass, by node name

    def subnet_of(self, zone):
        return self.nodeclass.subnets[list(self.cmod.ZONES).index(zone)]

    def _create(self, reqs, requests, options, pool):
        from kpamd import synth
        from kpamd.model import InstanceInfo, NodeDrift
        types = self.types()
        options = [t for t in options if synth.ami_for_type(types[t], self.nodeclass.amis) is not None]
        if not options:
            return None
        name = super()._create(reqs, requests, options, pool)
        if name is not None:
            n = self.nodes[name]
            ami = self.nodeclass.amis[synth.ami_for_type(types[n["type"]], self.nodeclass.amis)]
            inst = InstanceInfo(ami.id, self.subnet_of(n["zone"]), list(self.nodeclass.security_groups), n["rid"])
            self.instances[name] = NodeDrift("pool-hash", "v1", self.nodeclass.hash, self.nodeclass.hash_version, inst)
        return name

    def cluster(self):
        from kpamd.model import DriftInputs, PoolDrift
        cl, names = super().cluster()
        cl.drift_inputs = DriftInputs([self.nodeclass], [PoolDrift(0, "pool-hash", "v1") for _ in self.pools],
                                      [self.instances[n] for n in names])
        return cl, names

    def _plan(self, cl):
        if self.backend == "device":
            return super()._plan(cl)
        return RefDetectPlan(cl)

    def _apply(self, cl, names, cmd):
        super()._apply(cl, names, cmd)
        for n in set(self.instances) - set(self.nodes):
            del self.instances[n]


def passes(env, max_passes=12):
    """One command per pass until the controller finds nothing: detection first (Controller.compute_command), the
    Drifted conditions kept between passes. Returns the commands."""
    from kpamd import disruption
    done = []
    for _ in range(max_passes):
        cl, names = env.cluster()
        plan = env._plan(cl)
        try:
            cmd = disruption.Controller().compute_command(cl, plan, now=env.clock)
            recs = plan.detect_drift()[0]
        finally:
            plan.close()
        env.clock += 1
        env.records.append({n: (int(r["reason"]), int(r["status"]), int(r["detail"])) for n, r in zip(names, recs)})
        for node, name in zip(cl.nodes, names):
            if node.drifted is None:
                env.drifted.pop(name, None)
            else:
                env.drifted[name] = node.drifted
        if cmd is None:
            return done
        env._apply(cl, names, cmd)
        env.commands.append(cmd)
        done.append((cmd.method, [names[c] for c in cmd.candidates], cmd.decision, len(cmd.result.get("replacements", []))))
    raise AssertionError(f"no fixed point after {max_passes} passes: {done}")


@pytest.fixture
def mk(request, lib):
    envs = []

    def make(backend, **kw):
        ctx = request.getfixturevalue("ctx") if backend == "device" else None
        env = DetectEnv(backend, lib, ctx=ctx, **kw)
        envs.append(env)
        return env
    yield make
    for env in envs:
        env.close()


def twin(mk, backend, scenario, **kw):
    env = mk(backend, **kw)
    out = scenario(env)
    if backend == "device":
        ref = mk("oracle", **kw)
        want = scenario(ref)
        assert env.launches == ref.launches, (env.launches, ref.launches)
        assert [(c.method, c.candidates, c.decision) for c in env.commands] == \
            [(c.method, c.candidates, c.decision) for c in ref.commands]
        assert env.records == ref.records
        assert env.summary() == ref.summary()
        assert out == want
    return env


def three_nodes(env, consolidate=True):
    """Three pods spread over three nodes of a pool under the API server's default budget. consolidate=False adds a
    budget of 0 for Underutilized: the scheduler of this model does not know that a nodeclass's AMIs narrow the types,
    so consolidation would propose types that cannot be launched."""
    from kpamd.model import Budget, LabelSelector, NodePool, PodShape, TopologySpread
    pool = NodePool("default", 0, 0, [(CT, "In", ["on-demand"]), NOT_BURSTABLE])
    pool.budgets = [Budget("10%")] + ([] if consolidate else [Budget("0", reasons=["Underutilized"])])
    env.pools = [pool]
    host = TopologySpread("kubernetes.io/hostname", 1, LabelSelector({"app": "app"}), "DoNotSchedule")
    env.deploy("app", PodShape({"pods": 1000, "cpu": 1000}, labels={"app": "app"}, topology_spread=[host]), 3)
    env.provision()
    old = list(env.nodes)
    assert len(old) == 3 and not env.pending()
    assert passes(env) == [] and not env.drifted                     # nothing drifted: nothing to do
    assert set(env.records[-1].values()) == {(driftdet_ref.NONE, driftdet_ref.OK, 0)}
    return old


def replaced(env, old, reason):
    """The fixed point: one Drift REPLACE per old node, one per pass (10% of three nodes is one), every old node gone,
    nothing drifted"""
    from kpamd import disruption
    first = len(env.records)
    done = passes(env)
    assert [(m, d, r) for m, _, d, r in done] == [("drift", disruption.REPLACE, 1)] * 3
    assert sorted(c[0] for _, c, _, _ in done) == sorted(old)
    assert {r[0] for r in env.records[first].values()} == {reason}   # the first pass saw every node drifted
    assert len(env.nodes) == 3 and not set(old) & set(env.nodes) and not env.pending() and not env.drifted
    assert set(env.records[-1].values()) == {(driftdet_ref.NONE, driftdet_ref.OK, 0)}
    return done


@pytest.mark.parametrize("backend", BACKENDS)
def test_ami_drift(mk, backend):
    """:93-113: the nodeclass publishes new AMIs; every node is replaced and runs its architecture's new one."""
    from kpamd.model import AMI

    def scenario(env):
        old = three_nodes(env)
        env.nodeclass.amis = [AMI(f"ami-{arch}-v2", [(ARCH, "In", [arch])]) for arch in ("amd64", "arm64")]
        done = replaced(env, old, driftdet_ref.AMI)
        assert {i.instance.image_id for n, i in env.instances.items()} == {f"ami-{env.labels(n)[ARCH]}-v2" for n in env.nodes}
        return done, env.summary()
    twin(mk, backend, scenario)


@pytest.mark.parametrize("backend", BACKENDS)
def test_ami_no_longer_matches_the_type(mk, backend):
    """:151-171: the nodeclass selected an arm64 AMI, so arm64 nodes were launched; it now selects an amd64 AMI: the
    nodes' types map to no AMI, they drift and amd64 nodes replace them."""
    from kpamd.model import AMI

    def scenario(env):
        env.nodeclass.amis = [AMI("ami-arm64-v1", [(ARCH, "In", ["arm64"])])]
        old = three_nodes(env, consolidate=False)
        assert {env.labels(n)[ARCH] for n in old} == {"arm64"}
        env.nodeclass.amis = [AMI("ami-amd64-v1", [(ARCH, "In", ["amd64"])])]
        first = len(env.records)
        done = replaced(env, old, driftdet_ref.AMI)
        assert {r[2] for r in env.records[first].values()} == {driftdet_ref.NO_AMI}
        assert {env.labels(n)[ARCH] for n in env.nodes} == {"amd64"}
        assert {i.instance.image_id for i in env.instances.values()} == {"ami-amd64-v1"}
        return done, env.summary()
    twin(mk, backend, scenario)


@pytest.mark.parametrize("backend", BACKENDS)
def test_security_group_drift(mk, backend):
    """:172-245: one security group leaves the nodeclass's status; every node is replaced with the remaining one."""
    def scenario(env):
        old = three_nodes(env)
        env.nodeclass.security_groups = ["sg-b"]
        done = replaced(env, old, driftdet_ref.SECURITY_GROUP)
        assert {tuple(i.instance.security_groups) for i in env.instances.values()} == {("sg-b",)}
        return done, env.summary()
    twin(mk, backend, scenario)


@pytest.mark.parametrize("backend", BACKENDS)
def test_subnet_drift(mk, backend):
    """:246-266: the nodeclass selects other subnets; every node is replaced into one of them."""
    def scenario(env):
        old = three_nodes(env)
        env.nodeclass.subnets = [s + "-new" for s in env.nodeclass.subnets]
        done = replaced(env, old, driftdet_ref.SUBNET)
        assert all(i.instance.subnet_id.endswith("-new") for i in env.instances.values())
        return done, env.summary()
    twin(mk, backend, scenario)


@pytest.mark.parametrize("backend", BACKENDS)
def test_reservation_no_longer_selected(mk, backend):
    """:453-474: a node launched into a capacity reservation; the nodeclass stops selecting it (and selects another):
    the node drifts and its replacement does not run in the old reservation."""
    from kpamd import catalog as cmod
    from kpamd import disruption
    from kpamd.model import NodePool, PodShape
    large = cmod.CapacityReservation("cr-large", "m5.large", "test-zone-1a", "default", 1)
    xlarge = cmod.CapacityReservation("cr-xlarge", "m5.xlarge", "test-zone-1a", "default", 1)

    def scenario(env):
        env.pools = [NodePool("default", 0, 0, [(CT, "In", ["reserved", "on-demand"]), NOT_BURSTABLE])]
        env.deploy("app", PodShape({"pods": 1000, "cpu": 1000}, labels={"app": "app"}), 1)
        env.provision()
        (old,) = list(env.nodes)
        assert env.nodes[old]["rid"] == "cr-large" and env.instances[old].instance.capacity_reservation_id == "cr-large"
        assert passes(env) == [] and not env.drifted
        del env.crs["cr-large"]
        env.add_reservation(xlarge)
        env.nodeclass.capacity_reservations = ["cr-xlarge"]
        first = len(env.records)
        done = passes(env)
        assert env.records[first] == {old: (driftdet_ref.CAPACITY_RESERVATION, driftdet_ref.OK, 0)}
        assert done[0][:3] == ("drift", [old], disruption.REPLACE)
        assert old not in env.nodes and not env.pending() and not env.drifted
        assert all(i.instance.capacity_reservation_id in (None, "cr-xlarge") for i in env.instances.values())
        return done, env.summary()
    twin(mk, backend, scenario, reservations=[large])
