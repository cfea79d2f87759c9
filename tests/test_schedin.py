"""kp_scheduler_inputs on the CPU: the plain-Python reference (tests/schedin_ref.py) against the
hand-written cases (tests/schedin_cases.py), the tables reaching a Solve through SchedulerInputs.apply, and the host's
argument validation (ctx = NULL: no device). tests/test_gpu_schedin.py holds the device to the reference."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import schedin_cases as cases  # noqa: E402
import schedin_ref as ref  # noqa: E402


@pytest.mark.parametrize("case", cases.ALL, ids=lambda f: f.__name__)
def test_reference_meets_hand_written(lib, case):
    state, want = case()
    got = ref.compute(state)
    for table, value in want.items():
        assert got[table] == value, (case.__name__, table)


def test_pinned_subset(lib):
    """On the pinned subset the per-template rule is the reference helper's (expectations.go GetDaemonSetOverhead)"""
    state, want = cases.pinned()
    rule = [[cases.expectations_rule(p, d) for d in state.daemonsets] for p in state.nodepools]
    assert rule == want
    assert ref.compute(state)["pool_matrix"] == want


def test_size_edge_cases_by_hand(lib):
    for built in (cases.template_count(0), cases.template_count(65), cases.pod_rows(), cases.value_count(65)):
        state, want = built
        got = ref.compute(state)
        for table, value in want.items():
            assert got[table] == value, table


def _problem(catalog, daemon_cpu):
    """Six 900m pods, one existing 2-vCPU-class node with 1000m free before daemonsets, one NodePool; the state holds
    one daemonset of daemon_cpu (or none) that is not yet bound on the node"""
    import e2e
    from kpamd import synth
    from kpamd.model import ExistingNode, PodShape, Problem, SchedNode, SchedulerState
    pool = e2e.default_nodepool()
    it = next(t for t in catalog if t.name == "m5.large")
    labels = synth.node_labels(it, 0, "on-demand", pool.name, "node-a")
    alloc = it.allocatable()
    bound = {"cpu": alloc["cpu"] - 1000, "memory": 1000, "pods": 1000}
    shape = PodShape(synth.req_res(900, 128))
    prob = Problem([catalog], [pool], [shape], np.zeros(6, np.uint32), 1_750_000_000 + np.arange(6, dtype=np.int64),
                   np.arange(1, 7, dtype=np.uint64), existing=[ExistingNode("node-a", labels, {}, {}, [], True)])
    dss = [PodShape(synth.req_res(daemon_cpu, 64))] if daemon_cpu else []
    state = SchedulerState([copy.deepcopy(pool)], dss, [SchedNode("node-a", labels, [], alloc, dict(it.capacity), [(bound, False)])])
    return prob, state


def test_apply_reaches_the_solve(lib, catalog):
    """The same pods with a 250m daemonset and without: without it one pod fits the existing node's 1000m; with it
    the node's remaining daemonset requests take 250m of them and the pod goes to a NodeClaim, and every NodeClaim's
    requests carry the 250m."""
    from oracle import pyoracle
    out = {}
    for cpu in (0, 250):
        prob, state = _problem(catalog, cpu)
        ref.apply(state, prob)
        assert prob.existing[0].available["cpu"] == 1000
        assert prob.existing[0].requests == ({"cpu": 250, "memory": 64 * 1000 << 20, "pods": 1000} if cpu else {})
        assert prob.nodepools[0].daemon_requests.get("cpu", 0) == cpu
        out[cpu] = pyoracle.solve(prob)
    on_node = {cpu: int((out[cpu]["placement"] <= -2).sum()) for cpu in out}
    assert on_node == {0: 1, 250: 0}
    for cpu, res in out.items():
        for nc in res["nodeclaims"]:
            assert nc["requests"]["cpu"] == cpu + 900 * len(nc["pods"])
    assert out[0]["placement"].tolist() != out[250]["placement"].tolist()


def test_scheduler_inputs_apply_matches_reference_apply(lib, catalog):
    """SchedulerInputs.apply writes what the reference's apply writes (no device: the object is built from the
    reference's tables)"""
    import kpamd
    prob, state = _problem(catalog, 250)
    want = ref.compute(state)
    fake = kpamd.SchedulerInputs.__new__(kpamd.SchedulerInputs)
    for t in ref.TABLES:
        setattr(fake, t, want[t])
    other = copy.deepcopy(prob)
    fake.apply(prob)
    ref.apply(state, other)
    assert prob.existing == other.existing and prob.nodepools == other.nodepools
    other.existing = []
    with pytest.raises(ValueError):
        fake.apply(other)


def _call(lib, st, nodes=True, pools=True):
    from kpamd import abi
    n = (abi.SchedNodeOut * max(1, st.n_nodes))() if st is not None else None
    p = (abi.SchedPoolOut * max(1, st.n_nodepools))() if st is not None else None
    out = abi.SchedOut(n if nodes else None, p if pools else None, None)
    return lib.kp_scheduler_inputs(None, C.byref(st) if st is not None else None, C.byref(out), None)


def test_argument_validation(lib):
    """KP_E_INVAL without a device (ctx = NULL, kp_solve_validate's convention): NULL arrays, a CSR that does not end
    at the pod count, a request row out of range; a well-formed state validates as KP_OK"""
    from kpamd import abi
    state, _ = cases.arithmetic()

    def fresh(edit=None, **kw):
        arena = abi.Arena()
        st = abi.build_sched_state(arena, state)
        for k, v in kw.items():
            setattr(st, k, v)
        if edit:
            edit(st)
        return arena, st

    def csr_short(st):
        st.pod_offsets[st.n_nodes] -= 1

    def csr_start(st):
        st.pod_offsets[0] = 1

    def csr_decreasing(st):
        st.pod_offsets[1], st.pod_offsets[2] = st.pod_offsets[2], st.pod_offsets[1] - 1

    def row_high(st):
        st.pods[0].requests = st.n_request_rows

    def bad_op(st):
        st.nodepools[0].requirements.items[0].op = 9

    def null_label_key(st):
        st.nodes[0].labels[0].key = None

    def null_pool_name(st):
        st.nodepools[0].name = None

    keep, st = fresh()
    assert _call(lib, st) == abi.KP_OK
    for kw in (dict(nodepools=None), dict(daemonsets=None), dict(nodes=None), dict(pod_offsets=None), dict(pods=None),
               dict(request_rows=None), dict(n_pods=st.n_pods + 1), dict(n_request_rows=1)):
        keep, bad = fresh(**kw)
        assert _call(lib, bad) == abi.KP_E_INVAL, kw
        assert lib.kp_last_error()
    state.nodepools[0].requirements = [("team", "In", ["x"])]
    for edit in (csr_short, csr_start, csr_decreasing, row_high, bad_op, null_label_key, null_pool_name):
        keep, bad = fresh(edit)
        assert _call(lib, bad) == abi.KP_E_INVAL, edit.__name__
    keep, st = fresh()
    assert _call(lib, st, nodes=False) == abi.KP_E_INVAL and _call(lib, st, pools=False) == abi.KP_E_INVAL
    assert lib.kp_scheduler_inputs(None, None, None, None) == abi.KP_E_INVAL
    assert _call(lib, st) == abi.KP_OK
