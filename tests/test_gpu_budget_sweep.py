"""NodePool disruption budgets on the device (kp_cluster_simulate_budgeted / kp_consolidate_argmin_budgeted): the
budget gate decides per subset, before the simulations, whether any NodePool owns more of its members than it allows.
Expected result of a budgeted call: the oracle's result for each admissible subset (kpamd.disruption.admissible) and the
zero no-op for each blocked one, reduced with disruption.local_choice / kpamd.choice_reduce."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

POOL = "karpenter.sh/nodepool"
ZERO = {"decision": 0, "nodepool": 0, "candidate_price": 0.0, "replacement_price": 0.0, "savings": 0.0, "n_options": 0,
        "n_pods": 0}


def _csr(subs):
    offs = np.zeros(len(subs) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(s) for s in subs])
    flat = np.concatenate([np.asarray(s, dtype=np.uint32) for s in subs] + [np.zeros(0, dtype=np.uint32)])
    return offs, flat


def _two_pools(cl):
    """Every node with i % 3 == 0 moves to the NodePool burst: 80 default and 40 burst nodes of 120."""
    for i, n in enumerate(cl.nodes):
        n.node.labels[POOL] = "burst" if i % 3 == 0 else "default"
    assert [p.name for p in cl.nodepools] == ["default", "burst"]
    return cl


def _expect(cl, subs, oracle, allowed, base=0):
    """(per-subset dicts, choice dict, blocked count) a budgeted call must return."""
    import kpamd
    from kpamd import disruption
    adm = disruption.admissible(cl, *_csr(subs), allowed)
    want = [w if a else dict(ZERO) for w, a in zip(oracle, adm)]
    choice = kpamd.choice_dict(kpamd.choice_reduce([disruption.local_choice(want, base)]))
    return want, choice, int((~adm).sum())


def _dicts(res):
    import kpamd
    return [kpamd.sim_dict(r) for r in res]


@pytest.fixture(scope="module")
def batched(catalog):
    """The batched-path cluster, its 399 subsets and the oracle's results for all of them (computed once)."""
    from kpamd import synth
    from oracle import pyoracle
    cl = _two_pools(synth.config4(catalog, n_nodes=120, seed=4))
    subs = synth.consolidation_subsets(cl, 300, seed=5)
    assert len(subs) == 399 and sum(len(s) > 64 for s in subs) > 0
    oracle, _ = pyoracle.simulate_batch(cl, subs)
    return cl, subs, oracle


@pytest.fixture(scope="module")
def plan(ctx, batched):
    import kpamd
    p = kpamd.ClusterPlan(ctx, batched[0])
    yield p
    p.close()


def test_budget_changes_the_choice(ctx, batched, plan):
    import kpamd
    from kpamd.disruption import UNLIMITED
    cl, subs, oracle = batched
    offs, flat = _csr(subs)
    want, choice, blocked = _expect(cl, subs, oracle, [12, 4])
    assert 0 < blocked < len(subs)
    ch, res, st = plan.argmin(offs, flat, read_all=True, allowed=[12, 4])
    assert _dicts(res) == want
    assert ch == choice
    assert st["budget_blocked"] == blocked
    assert ch["counts"][0] >= blocked and sum(ch["counts"]) == len(subs)
    free, _, _ = plan.argmin(offs, flat)
    assert free["subset"] >= 0 and ch["subset"] >= 0 and ch["subset"] != free["subset"]  # the budget changes the choice
    # the plain simulate calls take the budget too
    got, st2 = plan.simulate(subs, allowed=[12, 4])
    assert got == want and st2["budget_blocked"] == blocked
    got_csr, st3 = plan.simulate_csr(offs, flat, allowed=[12, 4])
    assert _dicts(got_csr) == want and st3["budget_blocked"] == blocked
    # everything blocked: no simulation is launched
    none, res0, st0 = plan.argmin(offs, flat, read_all=True, allowed=[0, 0])
    assert none["subset"] == -1 and none["counts"] == [len(subs), 0, 0] and st0["budget_blocked"] == len(subs)
    assert _dicts(res0) == [ZERO] * len(subs)
    # all-unlimited: identical to the call without budgets
    unl, resu, stu = plan.argmin(offs, flat, read_all=True, allowed=[UNLIMITED, UNLIMITED])
    free2, resf, _ = plan.argmin(offs, flat, read_all=True)
    assert unl == free2 == free and stu["budget_blocked"] == 0 and (resu == resf).all()
    assert _dicts(resu) == oracle
    # a one-rank communicator and a base index
    comm = kpamd.Comm(ctx, kpamd.comm_unique_id(), 1, 0)
    try:
        chc, _, stc = plan.argmin(offs, flat, base_index=1000, comm=comm, allowed=[12, 4])
    finally:
        comm.close()
    assert chc == _expect(cl, subs, oracle, [12, 4], base=1000)[1] and stc["budget_blocked"] == blocked
    assert chc["subset"] == ch["subset"] + 1000 and chc["result"] == ch["result"]


def test_chunk_boundary(batched, plan):
    """A pool's members straddle the 64-member chunk: 30 burst nodes, then 66 / 67 default nodes, allowed 66."""
    from kpamd.disruption import UNLIMITED, admissible
    cl = batched[0]
    burst = [i for i in range(len(cl.nodes)) if i % 3 == 0][:30]
    default = [i for i in range(len(cl.nodes)) if i % 3 != 0]
    subs = [burst + default[:66], burst + default[:67], [default[0]], [], default[:67][::-1] + burst, burst[:1]]
    allowed = [66, UNLIMITED]
    adm = admissible(cl, *_csr(subs), allowed).tolist()
    assert adm == [True, False, True, True, False, True]
    free, _ = plan.simulate(subs)
    got, st = plan.simulate(subs, allowed=allowed)
    assert got == [f if a else ZERO for f, a in zip(free, adm)]
    assert st["budget_blocked"] == 2
    assert free[1] != ZERO  # (a blocked subset's zero record is not what its simulation gives)


def test_many_subsets_cross_gate_blocks(batched, plan):
    """3,192 subsets in one call: the live list's scatter and the block scan cross block boundaries; the results of
    the eight repeats are the same, and equal the expectation."""
    cl, subs, oracle = batched
    want, choice, blocked = _expect(cl, subs, oracle, [12, 4])
    offs, flat = _csr(subs * 8)
    ch, res, st = plan.argmin(offs, flat, read_all=True, allowed=[12, 4])
    got = _dicts(res)
    for r in range(8):
        assert got[r * len(subs):(r + 1) * len(subs)] == want, r
    assert st["budget_blocked"] == 8 * blocked
    assert ch["subset"] == choice["subset"] and ch["result"] == choice["result"]
    assert ch["counts"] == [8 * c for c in choice["counts"]]


def test_general_path(ctx, catalog):
    """A cluster with topology spread (whole Solves per subset): blocked subsets are neither batched nor compiled."""
    import kpamd
    from kpamd import disruption, synth
    from oracle import pyoracle
    cl = _two_pools(synth.spread_cluster(catalog, 120, seed=4))
    subs = [cl.candidates[:k] for k in range(2, 20)]
    subs += synth.consolidation_subsets(cl, 40, seed=5, max_size=24, prefixes=False)
    offs, flat = _csr(subs)
    allowed = [3, 0]
    adm = disruption.admissible(cl, offs, flat, allowed)
    assert 0 < adm.sum() < len(subs)
    live = [i for i in range(len(subs)) if adm[i]]
    oracle, _ = pyoracle.simulate_batch(cl, [subs[i] for i in live])  # (the oracle on the admissible subsets only)
    want = [dict(ZERO) for _ in subs]
    for i, w in zip(live, oracle):
        want[i] = w
    choice = kpamd.choice_dict(kpamd.choice_reduce([disruption.local_choice(want, 0)]))
    p = kpamd.ClusterPlan(ctx, cl)
    try:
        ch, res, st = p.argmin(offs, flat, read_all=True, allowed=allowed)
        free, resf, stf = p.argmin(offs, flat, read_all=True)
    finally:
        p.close()
    assert _dicts(res) == want and ch == choice
    assert st["budget_blocked"] == len(subs) - len(live)
    assert st["phase_cycles"][0] + st["phase_cycles"][1] == len(live)       # no launch for a blocked subset
    assert stf["phase_cycles"][0] + stf["phase_cycles"][1] == len(subs)
    assert [_dicts(resf)[i] for i in live] == oracle
    assert free["subset"] >= 0 and ch["subset"] >= 0 and ch["subset"] != free["subset"]


def test_errors(ctx, batched, plan):
    import kpamd
    from kpamd import abi
    cl, subs, _ = batched
    offs, flat = _csr(subs[:20])
    with pytest.raises(kpamd.KPError) as e:
        plan.argmin(offs, flat, allowed=[1, 2, 3])
    assert e.value.code == abi.KP_E_INVAL
    with pytest.raises(kpamd.KPError) as e:
        plan.simulate(subs[:20], allowed=[1])
    assert e.value.code == abi.KP_E_INVAL
    # a set cancel token; the plan stays usable
    tok = kpamd.Cancel(ctx)
    try:
        tok.set()
        with pytest.raises(kpamd.KPError) as e:
            plan.argmin(offs, flat, allowed=[12, 4], cancel=tok)
        assert e.value.code == abi.KP_E_CANCELED
        tok.reset()
        a, _, sa = plan.argmin(offs, flat, allowed=[12, 4], cancel=tok)
    finally:
        tok.close()
    b, _, sb = plan.argmin(offs, flat, allowed=[12, 4])
    assert a == b and sa["budget_blocked"] == sb["budget_blocked"]
    # a member node without a NodePool label: refused with the subset and the node, but only under a budget
    bad = copy.copy(cl)
    bad.nodes = list(cl.nodes)
    victim = subs[3][1]
    bad.nodes[victim] = copy.copy(cl.nodes[victim])
    bad.nodes[victim].node = copy.copy(cl.nodes[victim].node)
    bad.nodes[victim].node.labels = {k: v for k, v in cl.nodes[victim].node.labels.items() if k != POOL}
    p = kpamd.ClusterPlan(ctx, bad)
    try:
        first = next(i for i, s in enumerate(subs) if victim in s)
        with pytest.raises(kpamd.KPError) as e:
            p.simulate(subs[:20], allowed=[12, 4])
        assert e.value.code == abi.KP_E_INVAL and f"subset {first}" in str(e.value) and f"node {victim}" in str(e.value)
        p.simulate(subs[:20])
    finally:
        p.close()
