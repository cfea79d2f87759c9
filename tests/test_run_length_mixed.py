"""The run-length commit across shapes of one request row (mixed runs). The queue is sorted by (cpu, memory), so pods of
different shapes with equal requests lie together; the continuation variant of the fast lane commits the next k of
them onto the NodeClaim it is filling in one step when each is of the same request class (and names no host port), its
level is already merged into that NodeClaim and tolerates its taints, its first-fit scan starts exactly there (cursor
and mutation stack), sort.Slice leaves the NodeClaim in place and Fits holds in closed form. Parity: device == the
one-pod-at-a-time oracle on crafted queues where each of those conditions cuts runs, under the default overrides
(kp_solve picks the variant from the queue), with either run-length variant forced (kp_overrides.fast_lane 2: with the
continuation round, 3: without) and with the batching forced off; the stats count the batched pods."""
import numpy as np
import pytest

ARCH = [("kubernetes.io/arch", "NotIn", ["arm64"])]
ZONE = "topology.kubernetes.io/zone"
M5 = [("karpenter.k8s.aws/instance-family", "In", ["m5"]), ("karpenter.sh/capacity-type", "In", ["on-demand"])]


def _problem(catalog, pools, shapes, order, name):
    """Pods in the given queue order: equal (cpu, memory) keep the order of their creation times."""
    from kpamd.model import Problem
    shape = np.asarray(order, dtype=np.uint32)
    creation = (1_750_000_000 + np.arange(len(order))).astype(np.int64)
    uid = np.arange(1, len(order) + 1, dtype=np.uint64)
    return Problem([catalog], pools, shapes, shape, creation, uid, name=name)


def _both(ctx, ov, prob, expect_runs=True):
    """Default overrides, both forced run-length variants and forced plain against the oracle; returns (default
    result, oracle result)."""
    import kpamd
    from oracle import pyoracle
    from test_gpu_parity import check_same
    want = pyoracle.solve(prob)
    ov()
    got = kpamd.Scheduler(ctx, prob).solve()
    check_same(got, want)
    print(prob.name, "run_length_pods", got["stats"]["run_length_pods"], "of", len(prob.pod_shape))
    if expect_runs:
        assert got["stats"]["run_length_pods"] > 0
    for forced in (2, 3):
        ov(fast_lane=forced)
        on = kpamd.Scheduler(ctx, prob).solve()
        check_same(on, want)
        print(prob.name, "fast_lane", forced, "run_length_pods", on["stats"]["run_length_pods"])
        if expect_runs:
            assert on["stats"]["run_length_pods"] > 0
    ov(fast_lane=1)
    off = kpamd.Scheduler(ctx, prob).solve()
    check_same(off, want)
    assert off["stats"]["run_length_pods"] == 0
    return got, want


def _pool():
    from kpamd.model import NodePool
    return NodePool("m5", 0, 0, list(M5))


def _ab():
    from kpamd import synth
    from kpamd.model import PodShape
    return [PodShape(synth.req_res(250, 512)), PodShape(synth.req_res(250, 512), required_terms=[list(ARCH)])]


@pytest.mark.gpu
def test_alternating_shapes_batch(ctx, catalog, ov):
    """Two shapes, equal requests, strictly alternating: no two neighbours share a shape, so every batched pod is a
    mixed one. A larger shape in front moves the run's start into the middle of a window."""
    from kpamd import synth
    from kpamd.model import PodShape
    shapes = _ab() + [PodShape(synth.req_res(1000, 2048))]
    order = [2] * 23 + [i % 2 for i in range(300)]
    _both(ctx, ov, _problem(catalog, [_pool()], shapes, order, "mixed-basic"))


@pytest.mark.gpu
@pytest.mark.parametrize("every", [3, 5, 7])
@pytest.mark.parametrize("third_first", [False, True])
def test_cursor_both_ways(ctx, catalog, ov, every, third_first):
    """A third shape of the same requests whose zone the shared NodeClaim cannot take, interleaved: its own NodeClaim
    holds fewer pods than the shared one (it sorts before it) or more (after it), so the other levels' scans start
    below or at the NodeClaim being filled. (No count is asserted: where the third shape's NodeClaim sorts first, the
    pod behind each of its pods must scan from there again, and with a third pod in every three no run is left.)"""
    from kpamd import synth
    from kpamd.catalog import ZONES
    from kpamd.model import PodShape
    a = PodShape(synth.req_res(250, 512), node_selector={ZONE: ZONES[0]})
    b = PodShape(synth.req_res(250, 512), node_selector={ZONE: ZONES[0]}, required_terms=[list(ARCH)])
    c = PodShape(synth.req_res(250, 512), node_selector={ZONE: ZONES[1]})
    order, j = [], 0
    for i in range(300):
        third = (i % every == every - 1) != third_first  # third_first: the third shape everywhere but those slots
        if third:
            order.append(2)
        else:
            order.append(j % 2)
            j += 1
    # (third shape in every 5th or 7th slot only: runs of the other two, merged into the shared NodeClaim, lie between)
    _both(ctx, ov, _problem(catalog, [_pool()], [a, b, c], order, f"mixed-cursor-{every}-{int(third_first)}"),
          expect_runs=not third_first and every in (5, 7))


@pytest.mark.gpu
def test_level_not_merged(ctx, catalog, ov):
    """A compatible shape that first appears in the middle of a run goes through the full NodeClaim.Add once, then
    joins the batches."""
    from kpamd import synth
    from kpamd.model import PodShape
    shapes = _ab() + [PodShape(synth.req_res(250, 512),
                               required_terms=[[("karpenter.k8s.aws/instance-cpu", "Gt", ["3"])]])]
    order = [i % 2 for i in range(101)] + [i % 3 for i in range(199)]
    _both(ctx, ov, _problem(catalog, [_pool()], shapes, order, "mixed-unmerged"))


@pytest.mark.gpu
def test_toleration_cuts_run(ctx, catalog, ov):
    """The heavier pool is tainted: the tolerating shape fills its NodeClaim, the other shape (same requests, merged
    levels aside) must not follow it there."""
    from kpamd import synth
    from kpamd.model import NodePool, PodShape
    pools = [NodePool("tainted", 10, 0, list(M5), taints=[("dedicated", "x", "NoSchedule")]),
             NodePool("plain", 1, 0, list(M5))]
    tol = [("dedicated", "Equal", "x", "NoSchedule")]
    shapes = [PodShape(synth.req_res(250, 512), tolerations=tol), PodShape(synth.req_res(250, 512)),
              PodShape(synth.req_res(250, 512), tolerations=tol, required_terms=[list(ARCH)])]
    order = [i % 3 for i in range(150)] + [0, 2, 0, 2, 1, 1] * 25
    _both(ctx, ov, _problem(catalog, pools, shapes, order, "mixed-taints"))


@pytest.mark.gpu
def test_sort_ties_and_moves(ctx, catalog, ov):
    """The block pattern of test_run_length's tie case, the alternating blocks with equal requests and different
    requirements: NodeClaims tie on len(Pods) and sort.Slice moves them inside mixed runs."""
    from kpamd import synth
    from kpamd.model import PodShape
    shapes = _ab() + [PodShape(synth.req_res(1000, 2048))]
    order = [0] * 40 + [1] * 40 + [0] * 25 + [2] * 30 + [1] * 60 + [0] * 100 + [2] * 10 + [1] * 5
    _both(ctx, ov, _problem(catalog, [_pool()], shapes, order, "mixed-ties"))


@pytest.mark.gpu
def test_fits_thresholds(ctx, catalog, ov):
    """m5 only: mixed runs whose requests cross every m5 size's allocatable cpu and memory inside the runs."""
    from kpamd import synth
    from kpamd.model import PodShape
    shapes = [PodShape(synth.req_res(1000, 4096)), PodShape(synth.req_res(1000, 4096), required_terms=[list(ARCH)]),
              PodShape(synth.req_res(1000, 4096), required_terms=[[("kubernetes.io/os", "In", ["linux"])]])]
    order = [i % 3 for i in range(230)]
    _both(ctx, ov, _problem(catalog, [_pool()], shapes, order, "mixed-fits"))


@pytest.mark.gpu
def test_host_port_shape_cuts_run(ctx, catalog, ov):
    """One interleaved shape names a host port: the full path places it (a new NodeClaim per conflict), the run is cut
    there and resumes behind it."""
    from kpamd import synth
    from kpamd.model import PodShape
    shapes = _ab() + [PodShape(synth.req_res(250, 512), host_ports=[(None, 8080, "TCP")])]
    order = [2 if i % 10 == 9 else i % 2 for i in range(300)]
    _both(ctx, ov, _problem(catalog, [_pool()], shapes, order, "mixed-hostports"))


@pytest.mark.gpu
def test_requeued_pods(ctx, catalog, ov):
    """A cpu limit leaves pods unschedulable (re-queued: lastLen stops inside windows), and a preferred term adds
    relaxation levels, with equal requests across the shapes."""
    from kpamd import synth
    from kpamd.catalog import ZONES
    from kpamd.model import NodePool, PodShape
    pool = NodePool("m5", 0, 0, list(M5), limits={"cpu": 40_000})
    pref = [(1, [(ZONE, "In", [ZONES[0]]), ("karpenter.k8s.aws/instance-family", "In", ["c5"])])]
    shapes = _ab() + [PodShape(synth.req_res(250, 512), preferred_terms=pref),
                      PodShape(synth.req_res(250, 512), preferred_terms=pref, required_terms=[list(ARCH)])]
    order = [i % 4 for i in range(300)]
    _both(ctx, ov, _problem(catalog, [pool], shapes, order, "mixed-requeue"), expect_runs=False)


@pytest.mark.gpu
@pytest.mark.parametrize("n_pods,seed", [(3_000, 5), (12_000, 6)])
def test_config2_mixed_runs(ctx, catalog, ov, n_pods, seed):
    """The headline generator (creation times spread over 600 s: queue neighbours rarely share a shape). Under the
    default overrides the device equals the oracle and batches more pods than there are queue neighbours of one shape
    on one NodeClaim in the oracle's result, which is the most a single-level commit could take."""
    from kpamd import synth
    prob = synth.config2(catalog, n_pods=n_pods, seed=seed)
    got, want = _both(ctx, ov, prob)
    cpu = np.array([s.requests["cpu"] for s in prob.shapes], dtype=np.int64)[prob.pod_shape]
    mem = np.array([s.requests["memory"] for s in prob.shapes], dtype=np.int64)[prob.pod_shape]
    q = np.lexsort((prob.pod_uid, prob.pod_creation, -mem, -cpu))  # byCPUAndMemoryDescending, creation, uid
    sh, pl = prob.pod_shape[q], want["placement"][q]
    single = int(np.sum((sh[1:] == sh[:-1]) & (pl[1:] == pl[:-1]) & (pl[1:] >= 0)))
    print(prob.name, "same-shape same-NodeClaim neighbours", single)
    assert got["stats"]["run_length_pods"] > single, (got["stats"]["run_length_pods"], single)
