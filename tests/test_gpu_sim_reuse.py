"""Slot reuse in the batched sweep: sim_kernel is persistent (wave `slot` runs subsets slot, slot + n_slots, ...), and
between two subsets a wave re-initialises or lazily invalidates its LDS areas (excl, dirty, keys, ring, the option-sort
arrays aliasing dirty), its global scratch rows (s_pod, s_start, s_ovl, s_ovlhp, s_nc), s_ncfail (cleared once per
launch) and the version counter that makes stale s_ncfail entries harmless. With the production grid every batch the
other tests send gives each wave one subset; kp_overrides.sim_slots shrinks the grid so that small batches run 15 to
100 subsets per wave, as the 1M-subset sweep does (about 120). Every run here must equal the CPU oracle
(oracle/pyoracle.py simulate_batch) in every field and the production run bit for bit; stats phase_cycles[1] (wave slots)
and phase_cycles[2] (most subsets any wave ran) show that the regime was reached."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _csr(subs):
    from test_gpu_budget_sweep import _csr as csr
    return csr(subs)


def _dicts(res):
    import kpamd
    return [kpamd.sim_dict(r) for r in res]


def _assert_oracle(res, want):
    """Every field of test_gpu_consolidation.FIELDS, subset by subset."""
    from test_gpu_consolidation import FIELDS
    got = _dicts(res)
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if tuple(g[f] for f in FIELDS) != tuple(w[f] for f in FIELDS)]
    assert not bad, f"{len(bad)}/{len(want)} subsets differ; first {bad[0]}: device {got[bad[0]]} oracle {want[bad[0]]}"


def _ceil(a, b):
    return (a + b - 1) // b


@pytest.fixture(scope="module")
def base(catalog):
    """The near-capacity config-4 cluster, its 399 subsets (99 prefixes + 300 random, up to 100 nodes) and the oracle's
    record for each, computed once. The decisions include no-op, delete and replace, so a wave's reuse crosses every
    transition between them."""
    from kpamd import synth
    from oracle import pyoracle
    cl = synth.config4(catalog, n_nodes=120, seed=4, loose=0.05)
    subs = synth.consolidation_subsets(cl, 300, seed=5)
    assert len(subs) == 399 and max(len(s) for s in subs) == 100
    oracle, _ = pyoracle.simulate_batch(cl, subs)
    assert {r["decision"] for r in oracle} == {0, 1, 2}
    return cl, subs, oracle


@pytest.fixture(scope="module")
def plan(ctx, base):
    import kpamd
    p = kpamd.ClusterPlan(ctx, base[0])
    yield p
    p.close()


@pytest.fixture(scope="module")
def prod(ctx, base, plan):
    """The production run (every override 0) of the 399 subsets: raw records and stats."""
    ctx.set_overrides()
    res, st = plan.simulate_csr(*_csr(base[1]))
    _assert_oracle(res, base[2])
    return res, st


@pytest.mark.parametrize("slots", [4, 8, 28])
def test_slots(base, plan, prod, ov, slots):
    """About 100, 50 and 15 subsets per wave."""
    _, subs, oracle = base
    ov(sim_slots=slots)
    res, st = plan.simulate_csr(*_csr(subs))
    assert st["phase_cycles"][1] == slots and st["phase_cycles"][2] == _ceil(len(subs), slots)
    _assert_oracle(res, oracle)
    assert (res == prod[0]).all()


def test_override_never_raises_the_grid(base, plan, prod, ov):
    """sim_slots above the production grid's slot count leaves the production grid."""
    _, subs, _ = base
    ov(sim_slots=1 << 20)
    res, st = plan.simulate_csr(*_csr(subs))
    assert st["phase_cycles"][1:3] == prod[1]["phase_cycles"][1:3]
    assert st["phase_cycles"][1] <= 4 * _ceil(len(subs), 4)
    assert (res == prod[0]).all()


def test_predecessor_independence(base, plan, prod, ov):
    """The same subsets reversed and in a fixed shuffle under 4 slots: every subset then runs after another
    predecessor on another wave; permuted back, the records are those of the production run."""
    _, subs, _ = base
    ov(sim_slots=4)
    n = len(subs)
    for perm in (np.arange(n)[::-1], np.random.default_rng(11).permutation(n)):
        res, st = plan.simulate_csr(*_csr([subs[int(i)] for i in perm]))
        assert st["phase_cycles"][1] == 4 and st["phase_cycles"][2] == _ceil(n, 4)
        back = np.empty_like(res)
        back[perm] = res
        assert (back == prod[0]).all()


def test_size_whiplash(base, plan, ov):
    """With 4 slots a subset's slot is its index mod 4. Slot 0 sees a 100-node subset, a 1-node subset, the empty
    subset, another 100-node subset and a 2-node subset; slot 1 the same five in another order; slots 2 and 3 run
    mid-sized subsets beside them. The power-of-two key padding, the ring and the option-sort arrays (aliased over the
    dirty list) then meet stale data of a much larger or much smaller predecessor."""
    from oracle import pyoracle
    cl, subs, oracle = base
    c = cl.candidates
    big_a, two = subs[98], subs[0]
    assert len(big_a) == 100 and len(two) == 2
    big_b, one, empty = list(c[20:120]), [c[0]], []
    extra, _ = pyoracle.simulate_batch(cl, [big_b, one, empty])
    known = {id(big_a): oracle[98], id(two): oracle[0], id(big_b): extra[0], id(one): extra[1], id(empty): extra[2]}
    slot0 = [big_a, one, empty, big_b, two]
    slot1 = [empty, big_a, two, one, big_b]
    mid = [i for i, s in enumerate(subs) if 20 <= len(s) <= 60][:10]
    assert len(mid) == 10
    batch, want = [], []
    for r in range(5):
        for s in (slot0[r], slot1[r]):
            batch.append(s)
            want.append(known[id(s)])
        for i in (mid[2 * r], mid[2 * r + 1]):
            batch.append(subs[i])
            want.append(oracle[i])
    tail = list(range(100, 120))  # (more subsets behind the sequence: 10 per wave in all)
    batch += [subs[i] for i in tail]
    want += [oracle[i] for i in tail]
    assert [len(batch[i]) for i in range(0, 20, 4)] == [100, 1, 0, 100, 2]
    ov(sim_slots=4)
    res, st = plan.simulate_csr(*_csr(batch))
    assert st["phase_cycles"][1] == 4 and st["phase_cycles"][2] == 10
    _assert_oracle(res, want)


def _check_reused(ctx, cl, subs, multi_node=True):
    """One cluster under the override the caller set: device == oracle, and every wave ran at least 8 subsets."""
    import kpamd
    from oracle import pyoracle
    want, _ = pyoracle.simulate_batch(cl, subs, multi_node=multi_node)
    p = kpamd.ClusterPlan(ctx, cl)
    try:
        res, st = p.simulate_csr(*_csr(subs), multi_node=multi_node)
    finally:
        p.close()
    assert st["phase_cycles"][1] == 4 and st["phase_cycles"][2] == _ceil(len(subs), 4) >= 8
    _assert_oracle(res, want)
    return want


def test_disruption_state(ctx, catalog, ov):
    """Pending pods, deleting nodes' pods (n_base > 0: every simulation's queue starts with them) and binding
    NodePool limits."""
    from kpamd import synth
    base_cl = synth.config4(catalog, n_nodes=120, seed=4, loose=0.05)
    cl = synth.with_disruption_state(base_cl, 7, cpu_limit_m=4000)
    subs = [[c for c in s if not cl.nodes[c].deleting] for s in synth.consolidation_subsets(base_cl, 30, seed=5)]
    subs = [s for s in subs if s]
    ov(sim_slots=4)
    want = _check_reused(ctx, cl, subs)
    assert {r["n_pods"] for r in want} != {0} and len({r["decision"] for r in want}) > 1


@pytest.mark.parametrize("seed,multi_node", [(1, True), (2, False)])
def test_random_clusters(ctx, catalog, ov, seed, multi_node):
    """Taints, minValues and uninitialised nodes, multi- and single-node."""
    from kpamd import synth
    cl = synth.random_cluster(catalog, seed, n_nodes=[20, 40, 70][seed % 3])
    subs = synth.consolidation_subsets(cl, 25, seed=seed, max_size=min(30, len(cl.nodes)))
    subs += [[c] for c in cl.candidates[:15]]
    ov(sim_slots=4)
    _check_reused(ctx, cl, subs, multi_node=multi_node)


def test_spot_to_spot(ctx, catalog, ov):
    from kpamd import synth
    cl = synth.random_cluster(catalog, 201, n_nodes=40)
    cl.spot_to_spot = True
    spot = [c for c in cl.candidates if dict(cl.nodes[c].node.labels).get("karpenter.sh/capacity-type") == "spot"]
    assert len(spot) >= 3
    subs = [[c] for c in spot[:15]] + [spot[i:i + 3] for i in range(0, max(0, len(spot) - 2), 2)]
    subs += synth.consolidation_subsets(cl, 25, seed=1, max_size=10)
    ov(sim_slots=4)
    _check_reused(ctx, cl, [s for s in subs if s])


def test_host_ports(ctx, catalog, ov):
    """The host-port overlay rows (s_ovlhp) of a slot, reused."""
    from kpamd import synth
    from test_hostports_volumes import cluster_with_ports
    cl = cluster_with_ports(catalog, 1)
    assert any(sh.host_ports for sh in cl.shapes) and any(n.node.host_ports for n in cl.nodes)
    subs = synth.consolidation_subsets(cl, 25, seed=1, max_size=min(30, len(cl.nodes)))
    subs += [[c] for c in cl.candidates[:15]]
    ov(sim_slots=4)
    _check_reused(ctx, cl, subs)


def test_gated_instantiation(ctx, catalog, base, ov):
    """sim_kernel's budget-gated instantiation (the live list instead of the subset index) under 4 slots: per-subset
    records, choice and blocked count as test_gpu_budget_sweep expects them; the stats count the live subsets only.
    The two-pool cluster differs from the module's only in the nodes' karpenter.sh/nodepool labels, which no pod of it
    selects on: the oracle's records are the module's (compared on the CPU when this test was written)."""
    import kpamd
    from kpamd import synth
    from test_gpu_budget_sweep import _expect, _two_pools
    _, subs, oracle = base
    cl = _two_pools(synth.config4(catalog, n_nodes=120, seed=4, loose=0.05))
    want, choice, blocked = _expect(cl, subs, oracle, [12, 4])
    live = len(subs) - blocked
    assert live >= 32 and blocked > 0
    offs, flat = _csr(subs)
    ov(sim_slots=4)
    p = kpamd.ClusterPlan(ctx, cl)
    try:
        ch, res, st = p.argmin(offs, flat, read_all=True, allowed=[12, 4])
        none, res0, st0 = p.argmin(offs, flat, read_all=True, allowed=[0, 0])
    finally:
        p.close()
    assert _dicts(res) == want
    assert ch == choice and st["budget_blocked"] == blocked
    assert st["phase_cycles"][1] == 4 and st["phase_cycles"][2] == _ceil(live, 4)
    # everything blocked: no wave is launched
    assert none["subset"] == -1 and st0["budget_blocked"] == len(subs) and st0["phase_cycles"][1:3] == [0, 0]
    assert not res0["decision"].any()


def test_device_argmax(base, plan, ov):
    import kpamd
    from kpamd import disruption
    _, subs, oracle = base
    ov(sim_slots=8)
    ch, _, st = plan.argmin(*_csr(subs))
    assert st["phase_cycles"][1] == 8 and st["phase_cycles"][2] == _ceil(len(subs), 8)
    assert ch == kpamd.choice_dict(kpamd.choice_reduce([disruption.local_choice(oracle, 0)]))


def test_after_a_cancelled_call(ctx, base, plan, prod, ov):
    """A call whose token is already set returns KP_E_CANCELED; the same plan and batch without a token then equal
    the oracle."""
    import kpamd
    from kpamd import abi
    _, subs, oracle = base
    offs, flat = _csr(subs)
    ov(sim_slots=4)
    tok = kpamd.Cancel(ctx)
    try:
        tok.set()
        with pytest.raises(kpamd.KPError) as e:
            plan.argmin(offs, flat, read_all=True, cancel=tok)
        assert e.value.code == abi.KP_E_CANCELED
    finally:
        tok.close()
    res, st = plan.simulate_csr(offs, flat)
    assert st["phase_cycles"][1] == 4 and st["phase_cycles"][2] == _ceil(len(subs), 4)
    _assert_oracle(res, oracle)
    assert (res == prod[0]).all()
