"""Launch reuse on the general path: GeneralBatchRun pipelines its launches over two slots whose arenas are reused
dirty. batch_init_kernel restores an arena from the pristine block except the existing nodes' request rows when four or
fewer resources are requested ("never read before written"), the existing nodes' requirements are copy-on-write
(ex_own bits), and every other per-simulation bit is reset by a fill. A production launch holds up to 4,096
simulations, so every other test's batch is one launch on fresh arenas; kp_overrides.general_launch caps a launch at a
few simulations, so that a 58-subset batch takes up to 58 launches, each slot's arenas reused by a simulation of
another size. Every run must equal the CPU oracle (oracle/pyoracle.py simulate_batch) in every field; stats
phase_cycles[2] (batched launches) shows that the arenas were reused."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

EPH, ENI = "ephemeral-storage", "vpc.amazonaws.com/pod-eni"


def _csr(subs):
    from test_gpu_budget_sweep import _csr as csr
    return csr(subs)


def _dicts(res):
    import kpamd
    return [kpamd.sim_dict(r) for r in res]


def _assert_oracle(res, want):
    from test_gpu_consolidation import FIELDS
    got = _dicts(res)
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if tuple(g[f] for f in FIELDS) != tuple(w[f] for f in FIELDS)]
    assert not bad, f"{len(bad)}/{len(want)} subsets differ; first {bad[0]}: device {got[bad[0]]} oracle {want[bad[0]]}"


def _ceil(a, b):
    return (a + b - 1) // b


def _subsets(cl):
    """test_gpu_budget_sweep.test_general_path's 58 subsets: the prefixes 2..19 and 40 random ones of 2..24 nodes."""
    from kpamd import synth
    subs = [cl.candidates[:k] for k in range(2, 20)]
    subs += synth.consolidation_subsets(cl, 40, seed=5, max_size=24, prefixes=False)
    assert len(subs) == 58
    return subs


def requested_resources(cl):
    """The resources some pod shape or some NodePool's daemonsets request: the Python model's view of what the host
    compile collects (RequestedResources: shape requests and template daemon requests > 0)."""
    out = set()
    for sh in cl.shapes:
        out |= {r for r, v in sh.requests.items() if v > 0}
    for p in cl.nodepools:
        out |= {r for r, v in (p.daemon_requests or {}).items() if v > 0}
    return out


def five_resource_cluster(catalog):
    """A spread cluster (synth.spread_cluster's labels and zone spread on config 4 with 30 % loose nodes, so that the
    decisions mix no-op, delete and replace) with two more requested resources: every odd shape asks for 1 GiB of
    ephemeral storage, every fourth a pod ENI. Each node's free ephemeral storage is its type's allocatable less its
    pods' requests; of the pod ENIs a node has one left at most (the rest taken outside the model), so the fifth
    resource binds: two displaced ENI pods cannot share a remaining node (on the CPU, 5 of the 58 records differ from
    those of the same cluster with every ENI free). pod-eni is the fifth requested resource in ABI order (cpu, memory,
    ephemeral-storage, pods, pod-eni), the first one read from the existing nodes' request rows."""
    from kpamd import synth
    from kpamd.model import LabelSelector, TopologySpread
    from test_gpu_budget_sweep import _two_pools
    cl = _two_pools(synth.config4(catalog, n_nodes=120, seed=4, loose=0.3))
    for i, sh in enumerate(cl.shapes):
        sh.labels = dict(sh.labels or {}, app=f"app-{i % 8}")
        if i % 2 == 0:
            sh.topology_spread = [TopologySpread("topology.kubernetes.io/zone", 1, LabelSelector({"app": f"app-{i % 8}"}),
                                                 "DoNotSchedule")]
        else:
            sh.requests = dict(sh.requests, **{EPH: 1024 * synth.MI * 1000})
        if i % 4 == 1:
            sh.requests = dict(sh.requests, **{ENI: 1000})
    for n in cl.nodes:
        alloc = cl.catalogs[0][n.instance_type].allocatable()
        used = {r: sum(cl.shapes[int(cl.pod_shape[p])].requests.get(r, 0) for p in n.pods) for r in (EPH, ENI)}
        assert all(alloc[r] >= used[r] for r in used)
        n.node.available = dict(n.node.available, **{EPH: alloc[EPH] - used[EPH], ENI: min(alloc[ENI] - used[ENI], 1000)})
    return cl


@pytest.fixture(scope="module")
def spread(catalog):
    """The two-pool spread cluster of test_general_path, its 58 subsets and the oracle's record for each (once)."""
    from kpamd import synth
    from oracle import pyoracle
    from test_gpu_budget_sweep import _two_pools
    cl = _two_pools(synth.spread_cluster(catalog, 120, seed=4))
    subs = _subsets(cl)
    oracle, _ = pyoracle.simulate_batch(cl, subs)
    assert len({r["decision"] for r in oracle}) > 1
    return cl, subs, oracle


@pytest.fixture(scope="module")
def plan(ctx, spread):
    import kpamd
    p = kpamd.ClusterPlan(ctx, spread[0])
    yield p
    p.close()


@pytest.fixture(scope="module")
def prod(ctx, spread, plan):
    """The production run (every override 0): one launch."""
    ctx.set_overrides()
    res, st = plan.simulate_csr(*_csr(spread[1]))
    assert st["phase_cycles"][:3] == [len(spread[1]), 0, 1]
    _assert_oracle(res, spread[2])
    return res, st


@pytest.mark.parametrize("per_launch", [1, 7, 16])
def test_many_launches(spread, plan, prod, ov, per_launch):
    """58, 9 and 4 launches over the two slots (at 7: at least 4 launches per slot)."""
    _, subs, oracle = spread
    ov(general_launch=per_launch)
    res, st = plan.simulate_csr(*_csr(subs))
    assert st["phase_cycles"][:3] == [len(subs), 0, _ceil(len(subs), per_launch)]
    _assert_oracle(res, oracle)
    assert (res == prod[0]).all()


def test_warm_dirty_arenas(ctx, spread, ov):
    """One plan, three calls under 7 simulations per launch: the large subsets, the whole list reversed, then 20
    single-node subsets. Launches take the longest simulations first, so across the calls a small simulation runs in an
    arena a large one just left, and the reverse."""
    import kpamd
    from oracle import pyoracle
    cl, subs, oracle = spread
    large = [i for i, s in enumerate(subs) if len(s) >= 16]
    assert len(large) >= 15
    singles = [[c] for c in cl.candidates[:20]]
    want1, _ = pyoracle.simulate_batch(cl, singles)
    ov(general_launch=7)
    p = kpamd.ClusterPlan(ctx, cl)
    try:
        for batch, want in (([subs[i] for i in large], [oracle[i] for i in large]), (subs[::-1], oracle[::-1]),
                            (singles, want1)):
            res, st = p.simulate_csr(*_csr(batch))
            assert st["phase_cycles"][:3] == [len(batch), 0, _ceil(len(batch), 7)]
            _assert_oracle(res, want)
    finally:
        p.close()


def test_uncopied_range_both_ways(ctx, catalog, spread, ov):
    """batch_init_kernel skips the existing nodes' request rows when at most four resources are requested and copies
    them otherwise. The module's cluster requests three; a second one requests five, the fifth binding. Each: a warm
    pass, then the list reversed on the now dirty arenas, both equal to the oracle."""
    import kpamd
    from oracle import pyoracle
    cl3, subs, oracle3 = spread
    assert len(requested_resources(cl3)) <= 4
    cl5 = five_resource_cluster(catalog)
    assert len(requested_resources(cl5)) >= 5 and {EPH, ENI} <= requested_resources(cl5)
    subs5 = _subsets(cl5)
    oracle5, _ = pyoracle.simulate_batch(cl5, subs5)
    assert {r["decision"] for r in oracle5} == {0, 1, 2}
    ov(general_launch=7)
    for cl, subs, oracle in ((cl3, subs, oracle3), (cl5, subs5, oracle5)):
        p = kpamd.ClusterPlan(ctx, cl)
        try:
            for batch, want in ((subs, oracle), (subs[::-1], oracle[::-1])):
                res, st = p.simulate_csr(*_csr(batch))
                assert st["phase_cycles"][:3] == [len(subs), 0, _ceil(len(subs), 7)]
                _assert_oracle(res, want)
        finally:
            p.close()


def anti_affinity_cluster(catalog):
    """test_pod_antiaffinity's consolidation cluster (seed 0), and subsets of which some hold every node that runs a
    pod owning one required anti-affinity term: its inverse group vanishes, so that subset is compiled on its own."""
    from kpamd import synth
    from test_pod_antiaffinity import aff, anti
    cl = synth.random_cluster(catalog, 70, n_nodes=20)
    rng = np.random.default_rng(0)
    for i, sh in enumerate(cl.shapes):
        sh.labels = {"app": f"app-{i % 4}"}
        if rng.random() < 0.4:
            sh.required_anti_affinity = [anti(f"app-{int(rng.integers(0, 4))}")]
        elif rng.random() < 0.2:
            sh.preferred_affinity = [aff(f"app-{int(rng.integers(0, 4))}", 5)]
    owners = {}
    for ni, n in enumerate(cl.nodes):
        for p in n.pods:
            for t in cl.shapes[int(cl.pod_shape[p])].required_anti_affinity or []:
                owners.setdefault(t.selector.match_labels["app"], set()).add(ni)
    assert owners
    subs = synth.consolidation_subsets(cl, 15, seed=0, max_size=12) + [[c] for c in cl.candidates[:10]]
    for own in owners.values():
        rest = [c for c in cl.candidates if c not in own]
        subs.append([c for c in cl.candidates if c in own])
        subs.append([c for c in cl.candidates if c in own or c == rest[0]])
    return cl, subs


def test_mixed_batched_and_per_subset(ctx, catalog, ov):
    import kpamd
    from oracle import pyoracle
    cl, subs = anti_affinity_cluster(catalog)
    want, _ = pyoracle.simulate_batch(cl, subs)
    ov(general_launch=4)
    p = kpamd.ClusterPlan(ctx, cl)
    try:
        res, st = p.simulate_csr(*_csr(subs))
    finally:
        p.close()
    batched, single, launches = st["phase_cycles"][:3]
    assert batched + single == len(subs) and batched > 0 and single > 0
    assert launches == _ceil(batched, 4) >= 8
    _assert_oracle(res, want)


def test_reservations(ctx, lib, catalog, ov):
    """Strict reservation mode and the held-reservation word (nc_held) across 7 launches."""
    import kpamd
    from kpamd import synth
    from oracle import pyoracle
    from test_reserved_consolidation import _reserve_nodes, reservation_cluster
    cl, crs = reservation_cluster(catalog, 70)
    cl = _reserve_nodes(lib, cl, crs, launch_into=True)
    assert any(n.node.labels.get("karpenter.sh/capacity-type") == "reserved" for n in cl.nodes)
    subs = synth.consolidation_subsets(cl, 12, seed=70, max_size=4) + [[c] for c in cl.candidates[:8]]
    want, _ = pyoracle.simulate_batch(cl, subs)
    ov(general_launch=3)
    p = kpamd.ClusterPlan(ctx, cl)
    try:
        res, st = p.simulate_csr(*_csr(subs))
    finally:
        p.close()
    assert st["phase_cycles"][0] + st["phase_cycles"][1] == len(subs)
    assert st["phase_cycles"][2] == _ceil(st["phase_cycles"][0], 3) >= 4
    _assert_oracle(res, want)


def test_budgeted(spread, plan, ov):
    """allowed = [3, 0] as in test_general_path: the blocked subsets take no place in a launch."""
    import kpamd
    from kpamd import disruption
    from test_gpu_budget_sweep import ZERO
    cl, subs, oracle = spread
    offs, flat = _csr(subs)
    adm = disruption.admissible(cl, offs, flat, [3, 0])
    live = int(adm.sum())
    assert 0 < live < len(subs)
    want = [w if a else dict(ZERO) for w, a in zip(oracle, adm)]
    choice = kpamd.choice_dict(kpamd.choice_reduce([disruption.local_choice(want, 0)]))
    ov(general_launch=7)
    ch, res, st = plan.argmin(offs, flat, read_all=True, allowed=[3, 0])
    assert _dicts(res) == want and ch == choice
    assert st["budget_blocked"] == len(subs) - live
    assert st["phase_cycles"][:3] == [live, 0, _ceil(live, 7)]


def test_after_a_cancelled_call(ctx, spread, plan, prod, ov):
    import kpamd
    from kpamd import abi
    _, subs, oracle = spread
    offs, flat = _csr(subs)
    ov(general_launch=7)
    tok = kpamd.Cancel(ctx)
    try:
        tok.set()
        with pytest.raises(kpamd.KPError) as e:
            plan.argmin(offs, flat, read_all=True, cancel=tok)
        assert e.value.code == abi.KP_E_CANCELED
    finally:
        tok.close()
    res, st = plan.simulate_csr(offs, flat)
    assert st["phase_cycles"][:3] == [len(subs), 0, _ceil(len(subs), 7)]
    _assert_oracle(res, oracle)
    assert (res == prod[0]).all()


def test_modes_share_slots(ctx, spread, ov):
    """One plan's two launch slots (arenas, argument blocks, record buffer, pinned buffers) serve every result mode of
    the launch loop. On one fresh plan, 7 simulations per launch (9 launches a call, each slot reused at least 4
    times): simulate, drift, command, validate (checks taken from the commands just returned, so every subset that
    decided is valid), simulate again. Each call's whole output equals the same call made first on a fresh plan of its
    own, and both simulate calls equal the oracle."""
    import kpamd
    import command_ref
    import validate_ref as vr
    from test_gpu_command import _bits
    cl, subs, oracle = spread
    offs, flat = _csr(subs)
    ov(general_launch=7)
    shape = [len(subs), 0, _ceil(len(subs), 7)]
    assert shape[2] == 9

    def simulate(p):
        res, st = p.simulate_csr(offs, flat)
        assert st["phase_cycles"][:3] == shape
        _assert_oracle(res, oracle)
        return res.tobytes()

    def drift(p):
        d = p.drift(subs, read_all=True)
        assert d["stats"]["phase_cycles"][:3] == shape
        return d["results"], d["first"], d["blocked"], command_ref.command_fields(d["replacements"])

    def command(p):
        sims, cmds, st = p.command(subs, multi_node=True)
        assert st["phase_cycles"][:3] == shape
        return [_bits(d) for d in sims], [command_ref.command_fields(c) for c in cmds], cmds

    def validate(p, cmds):
        checks = [vr.check_of(cl, c) if c is not None else {"decision": vr.DELETE} for c in cmds]
        got, st = p.validate(subs, checks)
        assert st["phase_cycles"][:3] == shape
        return got

    def alone(call, *args):
        p = kpamd.ClusterPlan(ctx, cl)
        try:
            return call(p, *args)
        finally:
            p.close()

    shared = kpamd.ClusterPlan(ctx, cl)
    try:
        assert simulate(shared) == alone(simulate)
        assert drift(shared) == alone(drift)
        sims, fields, cmds = command(shared)
        assert (sims, fields) == alone(command)[:2]
        assert any(c is not None for c in cmds) and any(c is None for c in cmds)
        verdicts = validate(shared, cmds)
        assert verdicts == alone(validate, cmds)
        assert all(v["verdict"] == vr.VALID for v, c in zip(verdicts, cmds) if c is not None)
        assert simulate(shared) == alone(simulate)
    finally:
        shared.close()
