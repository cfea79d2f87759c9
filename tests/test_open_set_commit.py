"""The open set of the Solve fast lane (kp_overrides.fast_lane 4, SolveArgs::cont 3). After an append commit the fast
lane pops the following window entries one at a time and places each on one of the last few NodeClaims it committed
to, from state held in LDS: requests, remaining types, threshold indices, headroom, version, the levels' failure memo
and one first-fit cursor per window entry, shifted with every sort.Slice move. An entry is taken only when the pod loop
would take exactly the same steps; a wrong decision changes the result silently. Every case is a builder, a CPU-only
test that shows from the one-pod-at-a-time oracle that the queue holds the situation, and a gpu test that holds the
device to the oracle under the default overrides, the open set forced (4), the closed-form run-length commit (3) and
the plain loop (1, which never batches). No number asserted here comes from the device. run_length_pods counts the
pods committed in a run onto the NodeClaim of the pod before them (the loop's pods on another open NodeClaim are not
counted), so it stays under test_run_length_edges' _class_bound under every variant, is 0 where the queue strictly
alternates, and is positive under the open set where the oracle's result holds run witnesses on NodeClaims without
minValues."""
import numpy as np
import pytest

from test_run_length_edges import (FAMILY, ON_DEMAND, _case, _class_bound, _first_pop, _m5, _problem, _queue, _requests,
                                   _run_witnesses, _shape)
from test_run_length_mixed import ARCH, ZONE

OPEN_SET, CLOSED_FORM, PLAIN = 4, 3, 1
POOL_LABEL = "example.com/pool"
TAINT = [("dedicated", "x", "NoSchedule")]
TOL = [("dedicated", "Equal", "x", "NoSchedule")]


def _zone(i, **kw):
    from kpamd.catalog import ZONES
    return _shape(node_selector={ZONE: ZONES[i]}, **kw)


def _tainted_pool(weight=10):
    from kpamd.model import NodePool
    from test_run_length_mixed import M5
    return NodePool("tainted", weight, 0, list(M5), labels={POOL_LABEL: "tainted"}, taints=list(TAINT))


def _placed_seq(prob, want):
    """NodeClaim and shape of every pod in queue order (first-pop Solves: the order of the commits)."""
    q = _queue(prob)
    return want["placement"][q], prob.pod_shape[q]


def _switches(prob, want):
    """Queue neighbours placed on different NodeClaims that both held their pod's shape before: what the closed-form
    commit on one NodeClaim cannot take and the open set can."""
    pl, sh = _placed_seq(prob, want)
    seen, n = set(), 0
    for i in range(len(pl)):
        if i and pl[i] != pl[i - 1] and pl[i] >= 0 and (int(pl[i]), int(sh[i])) in seen \
                and (int(pl[i - 1]), int(sh[i - 1])) in seen:
            n += 1
        seen.add((int(pl[i]), int(sh[i])))
    return n


def _recent(prob, want, k):
    """Pods that land on one of the last k distinct NodeClaims committed to before them."""
    pl, _ = _placed_seq(prob, want)
    last, n = [], 0
    for x in (int(v) for v in pl):
        n += x in last[-k:]
        if x in last:
            last.remove(x)
        last.append(x)
    return n


# ---- the cases ------------------------------------------------------------------------------------------------------
def build_two_zones(catalog):
    """1. Two zone-pinned shapes of equal requests, strictly alternating onto two NodeClaims."""
    return _problem([catalog], [_m5()], [_zone(0), _zone(1)], [i % 2 for i in range(300)], "open-two-zones")


def pre_two_zones(prob, want):
    assert _first_pop(prob, want) and len(want["nodeclaims"]) == 2
    assert _switches(prob, want) >= 290


def build_rotation(catalog):
    """2. Three zones on the plain pool and two on a tainted, labelled pool: five NodeClaims take pods in turn, one
    more than the set holds, so every commit evicts and the evicted NodeClaim comes back four pods later."""
    from kpamd.catalog import ZONES
    shapes = [_zone(0), _zone(1), _zone(2)]
    for i in (0, 1):
        shapes.append(_shape(node_selector={ZONE: ZONES[i], POOL_LABEL: "tainted"}, tolerations=list(TOL)))
    order = [i % 5 for i in range(200)] + [[0, 1, 2, 0, 1, 3, 4][i % 7] for i in range(210)]
    return _problem([catalog], [_tainted_pool(), _m5()], shapes, order, "open-rotation")


def pre_rotation(prob, want):
    assert _first_pop(prob, want) and len(want["nodeclaims"]) == 5
    pools = [n["nodepool"] for n in want["nodeclaims"]]
    assert sorted(pools) == [0, 0, 1, 1, 1]
    assert _recent(prob, want, 5) > _recent(prob, want, 4) + 100  # the fifth NodeClaim is always the one evicted


def build_follower(catalog):
    """3. A shape without requirements between two pinned ones, in blocks of changing length: the two NodeClaims
    swap places in the order as they overtake each other, and the free shape follows whichever is first."""
    order = []
    for i in range(60):
        order += [0] * (i % 4 + 1) + [2] + [1] * ((3 * i) % 5 + 1) + [2]
    return _problem([catalog], [_m5()], [_zone(0), _zone(1), _shape()], order[:420], "open-follower")


def pre_follower(prob, want):
    assert _first_pop(prob, want) and len(want["nodeclaims"]) == 2
    pl, sh = _placed_seq(prob, want)
    free = pl[sh == 2]
    assert 40 < int(np.sum(free == 0)) < len(free) - 40  # the free shape lands on both, many times
    assert int(np.sum(free[1:] != free[:-1])) > 20


def build_ties(catalog, fillers):
    """4. `fillers` NodeClaims filled by one large pod each, then two open NodeClaims that tie on len(Pods) at every
    second commit, so sort.Slice moves one: insertion sort up to 12 NodeClaims, the literal pdqsort between 13 and
    49 (the loop must stop), partialInsertionSort from 50."""
    shapes = [_zone(0), _zone(1), _shape(cpu=95_500, mem=1024)]
    return _problem([catalog], [_m5()], shapes, [2] * fillers + [i % 2 for i in range(240)], f"open-ties-{fillers}")


def pre_ties(prob, want, fillers):
    assert _first_pop(prob, want) and len(want["nodeclaims"]) == fillers + 2
    sizes = sorted(len(n["pods"]) for n in want["nodeclaims"])
    assert sizes[:fillers] == [1] * fillers and sizes[fillers:] == [120, 120]
    n = fillers + 2
    assert n <= 12 if fillers == 8 else 12 < n < 50 if fillers == 30 else n >= 50


def build_thresholds(catalog):
    """5 and 10. Pods of 1 cpu / 4 Gi alternating between two zones: the totals cross every m5 size's allocatable
    values (the remaining types narrow inside the runs) until the NodeClaims are full (the remaining types would be
    empty: a rejection), where a NodeClaim is created in mid-run and the set starts again."""
    return _problem([catalog], [_m5()], [_zone(0, cpu=1000, mem=4096), _zone(1, cpu=1000, mem=4096)],
                    [i % 2 for i in range(420)], "open-thresholds")


def pre_thresholds(prob, want):
    assert _first_pop(prob, want) and len(want["nodeclaims"]) >= 4
    first = [n for n in want["nodeclaims"] if len(n["pods"]) > 80]
    assert len(first) >= 2 and all(len(n["options"]) <= 2 for n in first)  # narrowed to the largest sizes
    firsts = sorted(min(n["pods"]) for n in want["nodeclaims"])
    assert firsts[2] > 100  # a creation well inside the alternating run


def build_unmerged(catalog):
    """6. A third shape, compatible with both open NodeClaims and new to them, appears in mid-run: one full
    NodeClaim.Add on each, then it joins."""
    gt = [[("karpenter.k8s.aws/instance-cpu", "Gt", ["3"])]]
    order = [i % 2 for i in range(100)] + [[0, 2, 1, 2][i % 4] for i in range(200)]
    return _problem([catalog], [_m5()], [_zone(0), _zone(1), _shape(required_terms=gt)], order, "open-unmerged")


def pre_unmerged(prob, want):
    assert _first_pop(prob, want) and len(want["nodeclaims"]) == 2
    pl, sh = _placed_seq(prob, want)
    assert (sh[:100] != 2).all() and len(set(pl[sh == 2].tolist())) == 2  # merged into both, after the run began


def build_taints(catalog):
    """7. A tainted NodeClaim open beside a plain one; the shape without the toleration has the same requests and no
    requirement that keeps it off the tainted NodeClaim but the taint."""
    shapes = [_shape(node_selector={POOL_LABEL: "tainted"}, tolerations=list(TOL)), _shape(),
              _shape(tolerations=list(TOL))]
    order = [i % 2 for i in range(150)] + [i % 3 for i in range(150)]
    return _problem([catalog], [_tainted_pool(), _m5()], shapes, order, "open-taints")


def pre_taints(prob, want):
    assert _first_pop(prob, want)
    pools = np.array([n["nodepool"] for n in want["nodeclaims"]])
    pl, sh = _placed_seq(prob, want)
    assert (pools[pl[sh == 1]] == 1).all() and (pools[pl[sh == 0]] == 0).all()
    assert _switches(prob, want) > 100


def build_requeue(catalog):
    """8. A cpu limit leaves pods unschedulable: they are pushed again and popped at the same length (Queue.Pop stops
    inside a run), the 300 entries span five windows, and the re-pushed entries wrap the ring."""
    from kpamd.model import NodePool
    from test_run_length_mixed import M5
    pool = NodePool("m5", 0, 0, list(M5), limits={"cpu": 40_000})
    return _problem([catalog], [pool], [_zone(0), _zone(1)], [i % 2 for i in range(300)], "open-requeue")


def pre_requeue(prob, want):
    assert int((want["placement"] < 0).sum()) > 50 and int((want["placement"] >= 0).sum()) > 128
    assert int(want["stats"]["pops"]) > prob.n_pods  # re-queued pods were popped again


def build_hostport_minvalues(catalog):
    """9. A host-port shape of the same requests between the pinned ones (its class is its own: it ends every run),
    and a heavier pool with minValues taking a fourth shape: its NodeClaims never enter the set."""
    from kpamd.model import NodePool
    flexible = NodePool("flexible", 10, 0, [(FAMILY, "In", ["m5", "c5", "r5"], 2), ON_DEMAND],
                        labels={POOL_LABEL: "flexible"})
    m5 = [[(FAMILY, "In", ["m5"])]]  # (one family: below the flexible pool's minValues, so the plain pool's)
    shapes = [_zone(0, required_terms=m5), _zone(1, required_terms=m5),
              _shape(host_ports=[(None, 8080, "TCP")], required_terms=m5),
              _shape(node_selector={POOL_LABEL: "flexible"}), _shape(node_selector={POOL_LABEL: "flexible"},
                                                                     required_terms=[list(ARCH)])]
    pattern = [0, 0, 1, 1, 0, 1, 3, 4, 3, 4, 0, 1, 2]  # (runs on the plain NodeClaims between the others)
    order = [pattern[i % 13] for i in range(364)]
    return _problem([catalog], [flexible, _m5()], shapes, order, "open-hostport-minvalues")


def pre_hostport_minvalues(prob, want):
    assert prob.nodepools[0].requirements[0][3] == 2
    pools = np.array([n["nodepool"] for n in want["nodeclaims"]])
    pl, sh = _placed_seq(prob, want)
    assert (pl >= 0).all() and (pools[pl[sh >= 3]] == 0).all() and (pools[pl[sh < 2]] == 1).all()
    assert len(set(pl[sh == 2].tolist())) == int((sh == 2).sum())  # one NodeClaim per host-port pod


CASES = {"two-zones": (build_two_zones, pre_two_zones, ()),
         "rotation": (build_rotation, pre_rotation, ()),
         "follower": (build_follower, pre_follower, ()),
         "ties-12": (build_ties, pre_ties, (8,)),
         "ties-pdqsort": (build_ties, pre_ties, (30,)),
         "ties-50": (build_ties, pre_ties, (60,)),
         "thresholds": (build_thresholds, pre_thresholds, ()),
         "unmerged": (build_unmerged, pre_unmerged, ()),
         "taints": (build_taints, pre_taints, ()),
         "requeue": (build_requeue, pre_requeue, ()),
         "hostport-minvalues": (build_hostport_minvalues, pre_hostport_minvalues, ())}


@pytest.mark.parametrize("which", sorted(CASES))
def test_open_set_inputs(catalog, which):
    build, pre, args = CASES[which]
    pre(*_case(catalog, build, *args), *args)


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(CASES))
def test_open_set_parity(ctx, catalog, ov, which):
    import kpamd
    from test_gpu_parity import check_same
    build, pre, args = CASES[which]
    prob, want = _case(catalog, build, *args)
    pre(prob, want, *args)
    bound, runs = None, False
    if _first_pop(prob, want):  # (the bound and the witnesses read the queue order as the order of the commits)
        bound = _class_bound(prob, want)
        plain = {i for i, n in enumerate(want["nodeclaims"])
                 if not any(len(r) > 3 and r[3] for r in prob.nodepools[n["nodepool"]].requirements)}
        runs = _run_witnesses(prob, want, only=plain) > 0
    print(prob.name, "bound", bound, "runs", runs)
    for v in (0, OPEN_SET, CLOSED_FORM, PLAIN):
        ov(fast_lane=v)
        got = kpamd.Scheduler(ctx, prob).solve()
        n = int(got["stats"]["run_length_pods"])
        print(prob.name, "fast_lane", v, "run_length_pods", n, "of", prob.n_pods)
        check_same(got, want)
        assert _requests(got) == _requests(want), f"fast_lane {v}: NodeClaim requests differ"
        if v == PLAIN:
            assert n == 0
        if bound is not None:
            assert n <= bound, (v, n, bound)
        if runs and v == OPEN_SET:
            assert n > 0
