"""kp_scheduler_inputs on the device against the plain-Python reference (tests/schedin_ref.py) with == on
every field, the present masks and the compatibility words included, at the smallest shapes where the kernels can go
wrong (tests/schedin_cases.py; tests/test_schedin.py holds the reference to the hand-written cases on the CPU)."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import schedin_cases as cases  # noqa: E402
import schedin_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def compare(ctx, state, want=None, name=""):
    expect = ref.compute(state)
    for table, value in (want or {}).items():   # the hand-written part, as on the CPU
        assert expect[table] == value, (name, table)
    got = ctx.scheduler_inputs(state)
    ref.assert_equal(got, expect, name)
    assert got.stats["device_ms"] >= 0 and got.stats["host_ms"] > 0
    return got, expect


@pytest.mark.parametrize("case", cases.ALL, ids=lambda f: f.__name__)
def test_hand_written(ctx, case):
    state, want = case()
    compare(ctx, state, want, case.__name__)


def test_pinned_subset(ctx):
    state, want = cases.pinned()
    got, _ = compare(ctx, state, {"pool_matrix": want})
    assert got.pool_compatible == [sum(row) for row in want]


@pytest.mark.parametrize("D", [0, 1, 63, 64, 65, 129])
def test_template_counts(ctx, D):
    """the only compatible template in the last lane of a word, or alone in the last word"""
    state, want = cases.template_count(D)
    got, _ = compare(ctx, state, want)
    words = [int(x) for x in got.compat[0]]
    assert words == [0] * ((D - 1) // 64) + [1 << ((D - 1) % 64)] if D else words == [0]


@pytest.mark.parametrize("N", [1, 255, 256, 257, 2100])
def test_node_counts(ctx, N):
    """2100 nodes of one pool: more than SI_POOL_CHUNKS (8) slices of one block stride (256) each, so every block of
    the pool kernel walks its slice in more than one stride"""
    state = cases.node_count(N, n_pools=2 if N == 2100 else 3)
    got, expect = compare(ctx, state)
    if N == 2100:
        assert expect["remaining"][0] == {"cpu": 1000 * N - sum(4100 + i for i in range(N))}


def test_pod_rows(ctx):
    state, want = cases.pod_rows()
    compare(ctx, state, want)


@pytest.mark.parametrize("V", [1, 64, 65])
def test_value_counts(ctx, V):
    state, want = cases.value_count(V)
    compare(ctx, state, want)


@pytest.mark.parametrize("P", [1, 9])
def test_pool_counts(ctx, P):
    state = cases.node_count(40, n_pools=P)
    got, expect = compare(ctx, state)
    if P == 9:   # the last pool owns no node: its limits are not limited (odd index: none) or untouched
        assert expect["remaining"][8] == {"cpu": 40000} and expect["remaining"][7] is None


SEEDS = (0, 1, 2, 3, 4, 5)   # chosen on the CPU from the reference alone: each meets the conditions asserted below


@pytest.mark.parametrize("seed", SEEDS)
def test_randomized(ctx, catalog, seed):
    from kpamd import synth
    cl = synth.config4(catalog, n_nodes=60, seed=5)
    state = synth.add_scheduler_state(cl, seed, n_daemonsets=12)
    expect = ref.compute(state)
    ones = sum(sum(row) for row in expect["matrix"]) / (60 * 12)
    assert 0.2 <= ones <= 0.8, ones
    assert any(expect["clamped"]) and not all(expect["clamped"])
    assert any(v < 0 for a in expect["available"] for v in a.values())
    ref.assert_equal(ctx.scheduler_inputs(state), expect, f"seed {seed}")


def test_two_calls_identical_bytes(ctx, catalog):
    """No atomics and no leftover state: two consecutive calls on one context write the same bytes; a call on another
    state in between changes nothing"""
    from kpamd import synth
    state = synth.add_scheduler_state(synth.config4(catalog, n_nodes=300, seed=6), 3, n_daemonsets=70)

    def raw():
        g = ctx.scheduler_inputs(state)
        return bytes(g.raw_nodes), bytes(g.raw_pools), g.compat.tobytes()

    first = raw()
    assert raw() == first
    compare(ctx, cases.arithmetic()[0])
    assert raw() == first


def test_solve_and_simulate_on_applied_inputs(ctx, catalog):
    """A Solve, and kp_cluster_simulate of ten subsets, on inputs filled by apply from the device equal the same calls
    on inputs filled from the reference"""
    import kpamd
    from kpamd import synth
    prob = synth.random_problem(catalog, 3, n_pods=120, n_existing=8)
    state = synth.add_scheduler_state(prob, 1, n_daemonsets=6)
    a, b = copy.deepcopy(prob), copy.deepcopy(prob)
    ctx.scheduler_inputs(state).apply(a)
    ref.apply(state, b)
    assert a.existing == b.existing and a.nodepools == b.nodepools
    ra, rb = kpamd.Scheduler(ctx, a).solve(), kpamd.Scheduler(ctx, b).solve()
    assert (ra["placement"] == rb["placement"]).all()
    key = lambda r: [(n["nodepool"], n["pods"], n["options"], n["requests"]) for n in r["nodeclaims"]]
    assert key(ra) == key(rb)
    cl = synth.config4(catalog, n_nodes=60, seed=5)
    state = synth.add_scheduler_state(cl, 2, n_daemonsets=6, taint_share=0.0)
    ca, cb = copy.deepcopy(cl), copy.deepcopy(cl)
    ctx.scheduler_inputs(state).apply(ca)
    ref.apply(state, cb)
    assert [n.node for n in ca.nodes] == [n.node for n in cb.nodes] and ca.nodepools == cb.nodepools
    subsets = [cl.candidates[:k] for k in (1, 2, 3, 5, 8)] + [[c] for c in cl.candidates[8:13]]
    sims = []
    for c in (ca, cb):
        plan = kpamd.ClusterPlan(ctx, c)
        try:
            sims.append(plan.simulate(subsets, multi_node=True)[0])
        finally:
            plan.close()
            for cat in plan.catalogs:
                cat.close()
    assert sims[0] == sims[1]


def test_errors_leave_the_context_serving(ctx):
    """a refused call (KP_E_INVAL) on a live context, then a good one"""
    from kpamd import abi
    state, want = cases.arithmetic()
    arena = abi.Arena()
    st = abi.build_sched_state(arena, state)
    st.pods[0].requests = st.n_request_rows
    nodes, pools = (abi.SchedNodeOut * st.n_nodes)(), (abi.SchedPoolOut * st.n_nodepools)()
    out = abi.SchedOut(nodes, pools, None)
    assert ctx.lib.kp_scheduler_inputs(ctx.h, C.byref(st), C.byref(out), None) == abi.KP_E_INVAL
    compare(ctx, state, want)
