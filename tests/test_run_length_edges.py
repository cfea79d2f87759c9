"""The fast lane's run-length commit at its class and window edges. After a pod is appended to a NodeClaim
the commit takes up to 63 further window entries in closed form (requests + k * pod, len(Pods) + k, one mutation-stack
entry, k cursors, k placements); a wrong k changes the result silently. Every case here is a builder function, a
CPU-only test that proves from the one-pod-at-a-time oracle alone that the input is the edge it claims to be, and a
gpu test that re-asserts it and holds the device to the oracle under every variant: auto (0), the run-length commit with
the continuation round (2: SolveArgs::cont 1) and without it (3: cont 2), and plain (1), which never batches.

No number asserted here comes from the device. The batched pods are bounded from above by _class_bound, which is
computed from the oracle's result, and from below only by "some": where a case is built so that runs exist
(_run_witnesses > 0 in the oracle's result), run_length_pods > 0 under the two forced run-length variants.

Resource slots follow kp_abi.h: cpu, memory, ephemeral-storage, pods, pod-eni, ... The closed-form Fits tests the
first four resources requested anywhere in the Solve; in a Solve requesting cpu, memory, ephemeral-storage and pods
the fourth is pods, in one requesting cpu, memory, pods and pod-eni it is pod-eni."""
import numpy as np
import pytest

from test_run_length_mixed import ARCH, M5

EPH = "ephemeral-storage"
ENI = "vpc.amazonaws.com/pod-eni"
GPU = "nvidia.com/gpu"
FAMILY = "karpenter.k8s.aws/instance-family"
ON_DEMAND = ("karpenter.sh/capacity-type", "In", ["on-demand"])
MI_M = (1 << 20) * 1000  # one Mi in milli-units
PLAIN = 1
VARIANTS = [0, 2, 3]  # kp_overrides.fast_lane: auto, cont 1, cont 2
MODE_FLAT, MODE_CHUNKED = 0, 2  # kp_solve_stats.order_chunks[4]


# ---- shared pieces -------------------------------------------------------------------------------------------------
def _problem(catalogs, pools, shapes, order, name):
    """Pods in the given input order: equal (cpu, memory) keep it in the queue (creation times ascend)."""
    from kpamd.model import Problem
    n = len(order)
    return Problem(list(catalogs), pools, shapes, np.asarray(order, dtype=np.uint32),
                   (1_750_000_000 + np.arange(n)).astype(np.int64), np.arange(1, n + 1, dtype=np.uint64), name=name)


def _m5():
    from kpamd.model import NodePool
    return NodePool("m5", 0, 0, list(M5))


def _shape(cpu=250, mem=512, extra=None, **kw):
    from kpamd import synth
    from kpamd.model import PodShape
    return PodShape(synth.req_res(cpu, mem, extra), **kw)


def _quad(extra):
    """Equal (cpu, memory), two request rows: plain; plus a required term; plus `extra`; plus both."""
    return [_shape(), _shape(required_terms=[list(ARCH)]), _shape(extra=extra),
            _shape(extra=extra, required_terms=[list(ARCH)])]


def _blocks(n, shapes_of_class=((0, 1), (2, 3))):
    """Blocks of 1 to 5 pods, the classes in turn, each class alternating its shapes."""
    order, b, used = [], 0, [0] * len(shapes_of_class)
    while len(order) < n:
        c = b % len(shapes_of_class)
        for _ in range(b % 5 + 1):
            order.append(shapes_of_class[c][used[c] % len(shapes_of_class[c])])
            used[c] += 1
        b += 1
    return order[:n]


def _family(it):
    return next((r[2][0] for r in it.requirements if r[0] == FAMILY and r[2]), None)


def _row(shape):
    """The whole request row (a zero request is no request)."""
    return tuple(sorted((k, v) for k, v in shape.requests.items() if v))


def _queue(prob):
    """Queue order: byCPUAndMemoryDescending, then creation, then uid."""
    cpu = np.array([s.requests.get("cpu", 0) for s in prob.shapes], dtype=np.int64)[prob.pod_shape]
    mem = np.array([s.requests.get("memory", 0) for s in prob.shapes], dtype=np.int64)[prob.pod_shape]
    return np.lexsort((prob.pod_uid, prob.pod_creation, -mem, -cpu))


def _classes(prob):
    """Per shape: an id of its whole request row; and whether it names a host port."""
    ids = {}
    rc = np.array([ids.setdefault(_row(s), len(ids)) for s in prob.shapes])
    return rc, np.array([bool(s.host_ports) for s in prob.shapes])


def _first_pop(prob, want):
    """The oracle placed every pod on its first pop (nothing re-queued)."""
    return int(want["stats"]["pops"]) == prob.n_pods and bool((want["placement"] >= 0).all())


def _class_bound(prob, want):
    """An upper bound on the batched pods, from the oracle alone: the queue positions p >= 1 whose pod has the
    request row of its queue predecessor, names no host port and sits on the predecessor's NodeClaim. A batched pod's
    ring predecessor is the batch's first pod or another batched pod, of its class and committed to the same NodeClaim;
    where every pod is placed on its first pop the ring order is the queue order, so every batched pod is counted."""
    assert _first_pop(prob, want)
    q = _queue(prob)
    rc, hp = _classes(prob)
    rc, hp, pl = rc[prob.pod_shape][q], hp[prob.pod_shape][q], want["placement"][q]
    return int(np.sum((rc[1:] == rc[:-1]) & ~hp[1:] & (pl[1:] == pl[:-1]) & (pl[1:] >= 0)))


def _run_witnesses(prob, want, seq=None, only=None):
    """Pairs of pods adjacent in the order of their successful pops (seq; default: the queue order, for first-pop
    Solves) that the commit can take together: one class, no host port, one NodeClaim that already held both their
    shapes (levels merged) and takes yet another pod after them (room). only: count those on these NodeClaims."""
    seq = _queue(prob) if seq is None else seq
    rc, hp = _classes(prob)
    pl = want["placement"]
    last = {i: n["pods"][-1] for i, n in enumerate(want["nodeclaims"]) if n["pods"]}
    seen, prev, count = {}, None, 0
    for p in (int(x) for x in seq):
        nc, sh = int(pl[p]), int(prob.pod_shape[p])
        had = nc >= 0 and sh in seen.setdefault(nc, set())
        if prev is not None and had and prev[0] == nc and prev[1] and rc[prev[2]] == rc[sh] and not hp[sh] \
                and not hp[prev[2]] and last[nc] != p and (only is None or nc in only):
            count += 1
        if nc >= 0:
            seen[nc].add(sh)
        prev = (nc, had, sh)
    return count


def _queue_shares(prob):
    """Queue neighbours that share their shape / their class (what the auto variant is chosen from)."""
    sh = prob.pod_shape[_queue(prob)]
    rc = _classes(prob)[0][sh]
    return int(np.sum(sh[1:] == sh[:-1])), int(np.sum(rc[1:] == rc[:-1]))


def _requests(res):
    return [{k: v for k, v in n["requests"].items() if v} for n in res["nodeclaims"]]


_CASES = {}


def _case(catalog, builder, *args):
    """(problem, oracle result) of a builder, computed once for the CPU-only test and the gpu test."""
    from oracle import pyoracle
    key = (builder.__name__,) + args
    if key not in _CASES:
        prob = builder(catalog, *args)
        _CASES[key] = (prob, pyoracle.solve(prob))
    return _CASES[key]


def _all_variants(ctx, ov, prob, want, runs=False, bound=None, more=None, **ov_kw):
    """Device == oracle (placements, NodeClaims, their summed requests) under every variant; nothing batched under
    plain; at most `bound` pods batched under any; some under the forced run-length variants where `runs`. `more` is
    called with (variant, device result) for the case's own asserts."""
    import kpamd
    from test_gpu_parity import check_same
    same, same_rc = _queue_shares(prob)
    print(prob.name, "pods", prob.n_pods, "same-shape neighbours", same, "same-class neighbours", same_rc,
          "classes", len(set(_classes(prob)[0])), "shapes", len(prob.shapes), "bound", bound)
    for v in VARIANTS + [PLAIN]:
        ov(fast_lane=v, **ov_kw)
        got = kpamd.Scheduler(ctx, prob).solve()
        n = int(got["stats"]["run_length_pods"])
        print(prob.name, "fast_lane", v, "run_length_pods", n, "order", list(got["stats"]["order_chunks"]))
        check_same(got, want)
        assert _requests(got) == _requests(want), f"fast_lane {v}: NodeClaim requests differ"
        if v == PLAIN:
            assert n == 0
        if bound is not None:
            assert n <= bound, (v, n, bound)
        if runs and v in (2, 3):
            assert n > 0, v
        if more:
            more(v, got)


# ---- a. the class is the whole request row -------------------------------------------------------------------------
A_EXTRA = {"eph": {EPH: 64 * MI_M}, "eni": {ENI: 1000}}
A_PARAMS = [(r, p) for r in ("eph", "eni") for p in ("alternating", "blocks")]


def build_whole_row(catalog, res, pattern):
    """Two classes that differ only outside cpu and memory (an ephemeral-storage or a pod-eni request), two shapes
    each: queue neighbours throughout. alternating: no pod follows one of its class; blocks: 1 to 5 of a class."""
    order = [[0, 2, 1, 3][i % 4] for i in range(300)] if pattern == "alternating" else _blocks(300)
    return _problem([catalog], [_m5()], _quad(A_EXTRA[res]), order, f"edge-row-{res}-{pattern}")


def _pre_whole_row(prob, want, pattern):
    rows = [dict(_row(s)) for s in prob.shapes]
    assert rows[0] == rows[1] and rows[2] == rows[3] and rows[0] != rows[2]
    assert all(r["cpu"] == rows[0]["cpu"] and r["memory"] == rows[0]["memory"] for r in rows)
    assert {k for k in rows[2] if rows[2][k] != rows[0].get(k)}.isdisjoint({"cpu", "memory"})
    bound = _class_bound(prob, want)
    if pattern == "alternating":
        assert bound == 0
    else:
        assert _run_witnesses(prob, want) > 0
    return bound


@pytest.mark.parametrize("res,pattern", A_PARAMS)
def test_whole_row_inputs(catalog, res, pattern):
    _pre_whole_row(*_case(catalog, build_whole_row, res, pattern), pattern)


@pytest.mark.gpu
@pytest.mark.parametrize("res,pattern", A_PARAMS)
def test_whole_row(ctx, catalog, ov, res, pattern):
    """alternating: the bound is 0, so nothing may be batched under any variant, the forced ones included (a class
    keyed on (cpu, memory) would batch here and add the first pod's row for pods that request something else)."""
    prob, want = _case(catalog, build_whole_row, res, pattern)
    bound = _pre_whole_row(prob, want, pattern)
    _all_variants(ctx, ov, prob, want, runs=pattern == "blocks", bound=bound)


# ---- b. four requested resources, the one beyond cpu, memory and pods binding --------------------------------------
B_EXTRA = {"eph": (EPH, 1024 * MI_M), "eni": (ENI, 5000)}


def build_fourth_binding(catalog, res):
    """Case a's classes in blocks of seven, the request large enough that it closes NodeClaims before cpu, memory or
    pods do: every m5 size allocates 17 Gi of ephemeral-storage (17 pods of 1 Gi), and 9 to 120 pod-eni (1, 3, 7, 10,
    21 and 24 pods of 5). Neither 17 nor 24 is a multiple of seven, so blocks straddle the closing value. eph:
    ephemeral-storage is the third of the four requested slots; eni: pod-eni is the fourth. The shapes without the
    request carry a zero in that slot."""
    k, v = B_EXTRA[res]
    order = [2 * (i // 7 % 2) + i % 2 for i in range(300)]
    return _problem([catalog], [_m5()], _quad({k: v}), order, f"edge-fourth-{res}")


def _pre_fourth_binding(prob, want, res):
    k, v = B_EXTRA[res]
    add = dict(_row(prob.shapes[2]))
    assert set(add) == {"cpu", "memory", "pods", k} and set(dict(_row(prob.shapes[0]))) == {"cpu", "memory", "pods"}
    closed = set()  # NodeClaims that one more pod of the class fits on every resource but this one
    for i, n in enumerate(want["nodeclaims"]):
        alloc = [prob.catalogs[0][t].allocatable() for t in n["options"]]
        others = any(all(a[r] >= n["requests"].get(r, 0) + add[r] for r in ("cpu", "memory", "pods")) for a in alloc)
        this = any(a[k] >= n["requests"].get(k, 0) + v for a in alloc)
        if others and not this and n["requests"].get(k, 0) > 0:
            closed.add(i)
    assert closed
    # ... and a run that this resource cut: a pod of the class behind another of it that sits on such a NodeClaim
    q = _queue(prob)
    sh, pl = prob.pod_shape[q], want["placement"][q]
    cut = int(np.sum((sh[1:] >= 2) & (sh[:-1] >= 2) & (pl[1:] != pl[:-1]) & np.isin(pl[:-1], list(closed))))
    assert cut > 0
    assert _run_witnesses(prob, want) > 0
    return _class_bound(prob, want)


@pytest.mark.parametrize("res", ["eph", "eni"])
def test_fourth_binding_inputs(catalog, res):
    _pre_fourth_binding(*_case(catalog, build_fourth_binding, res), res)


@pytest.mark.gpu
@pytest.mark.parametrize("res", ["eph", "eni"])
def test_fourth_binding(ctx, catalog, ov, res):
    prob, want = _case(catalog, build_fourth_binding, res)
    _all_variants(ctx, ov, prob, want, runs=True, bound=_pre_fourth_binding(prob, want, res))


# ---- c. pods thresholds --------------------------------------------------------------------------------------------
def build_pods_thresholds(catalog, eph):
    """Three shapes of one class at 10m / 16Mi: a NodeClaim's requests cross every m5 size's pod capacity (29, 58,
    234, 737) long before cpu or memory, inside runs. eph: each also requests 1Mi of ephemeral-storage, which makes
    pods the fourth requested slot instead of the third."""
    extra = {EPH: MI_M} if eph else None
    shapes = [_shape(10, 16, extra), _shape(10, 16, extra, required_terms=[list(ARCH)]),
              _shape(10, 16, extra, required_terms=[[("kubernetes.io/os", "In", ["linux"])]])]
    return _problem([catalog], [_m5()], shapes, [i % 3 for i in range(1600)], f"edge-pods-{int(eph)}")


def _pre_pods_thresholds(prob, want):
    m5 = [it for it in prob.catalogs[0] if (FAMILY, "In", ["m5"]) in [tuple(r[:3]) for r in it.requirements]
          and any(o.available and o.capacity_type == "on-demand" for o in it.offerings)]
    large = min(it.allocatable()["pods"] for it in m5) // 1000
    assert large == 29 and len({it.allocatable()["pods"] for it in m5}) >= 4
    assert any(len(n["pods"]) > large and n["n_remaining"] < len(m5) for n in want["nodeclaims"])
    assert _run_witnesses(prob, want) > 0
    return _class_bound(prob, want)


@pytest.mark.parametrize("eph", [False, True])
def test_pods_thresholds_inputs(catalog, eph):
    _pre_pods_thresholds(*_case(catalog, build_pods_thresholds, eph))


@pytest.mark.gpu
@pytest.mark.parametrize("eph", [False, True])
def test_pods_thresholds(ctx, catalog, ov, eph):
    prob, want = _case(catalog, build_pods_thresholds, eph)
    _all_variants(ctx, ov, prob, want, runs=True, bound=_pre_pods_thresholds(prob, want))


# ---- d. zero requests ----------------------------------------------------------------------------------------------
def build_zero_requests(catalog):
    """Two BestEffort shapes (no cpu, no memory; one with a required term) interleaved with each other and, in input
    order, with a 250m class: cpu and memory are in the Solve's mask and zero in their rows."""
    shapes = [_shape(0, 0), _shape(0, 0, required_terms=[list(ARCH)]), _shape(), _shape(required_terms=[list(ARCH)])]
    return _problem([catalog], [_m5()], shapes, [i % 4 for i in range(300)], "edge-zero")


def _pre_zero_requests(prob, want):
    assert set(dict(_row(prob.shapes[0]))) == {"pods"} and _row(prob.shapes[0]) == _row(prob.shapes[1])
    assert set(dict(_row(prob.shapes[2]))) == {"cpu", "memory", "pods"}
    q = _queue(prob)
    assert (prob.pod_shape[q][:150] >= 2).all() and (prob.pod_shape[q][150:] < 2).all()
    assert _run_witnesses(prob, want) > 0
    return _class_bound(prob, want)


def test_zero_requests_inputs(catalog):
    _pre_zero_requests(*_case(catalog, build_zero_requests))


@pytest.mark.gpu
def test_zero_requests(ctx, catalog, ov):
    prob, want = _case(catalog, build_zero_requests)
    _all_variants(ctx, ov, prob, want, bound=_pre_zero_requests(prob, want))


# ---- e. five resources in the Solve --------------------------------------------------------------------------------
def build_five_resources(catalog):
    """Case a's block queue plus a shape of the same cpu and memory that requests a GPU, in a pool that admits a GPU
    family: five resources are requested in the Solve, more than the closed-form Fits covers."""
    from kpamd.model import NodePool
    shapes = _quad(A_EXTRA["eph"]) + [_shape(extra={GPU: 1000})]
    order = []
    for i, s in enumerate(_blocks(300)):
        order.append(s)
        if i % 15 == 14:
            order.append(4)
    pool = NodePool("m5-g4dn", 0, 0, [(FAMILY, "In", ["m5", "g4dn"]), ON_DEMAND])
    return _problem([catalog], [pool], shapes, order, "edge-five")


def _pre_five_resources(prob, want):
    assert len({k for s in prob.shapes for k, _ in _row(s)}) == 5
    gpu_pods = np.nonzero(prob.pod_shape == 4)[0]
    assert len(gpu_pods) == 20
    for p in gpu_pods:
        assert want["nodeclaims"][want["placement"][p]]["requests"].get(GPU, 0) > 0
    assert _run_witnesses(prob, want) > 0  # (shapes that would batch, were the Solve's fifth resource not there)
    return _class_bound(prob, want)


def test_five_resources_inputs(catalog):
    _pre_five_resources(*_case(catalog, build_five_resources))


@pytest.mark.gpu
def test_five_resources(ctx, catalog, ov):
    prob, want = _case(catalog, build_five_resources)
    _all_variants(ctx, ov, prob, want, bound=_pre_five_resources(prob, want))


# ---- f. window and buffer alignment --------------------------------------------------------------------------------
F_PARAMS = [(pre, kind) for kind in ("larger", "classes") for pre in (0, 1, 62, 63, 64, 65, 127)]


def _small():
    """Two shapes of one class at 10m / 16Mi: an m5 NodeClaim's Fits thresholds lie at 29, 58, 193 (cpu), 234 and 737
    pods, so that between them the window alone cuts the runs."""
    return [_shape(10, 16), _shape(10, 16, required_terms=[list(ARCH)])]


def build_window(catalog, pre, kind):
    """`pre` pods in front of 200 pods alternating two shapes of one class, everything on one NodeClaim, so the runs
    are cut by the 64-lane window alone and reach its last entry. larger: the prefix is one larger shape (a run of
    its own under the run-length variants). classes: the prefix has the same cpu and memory and alternates two other
    classes behind one pod of each shape (levels merged), so it is committed pod by pod and the first batch meets a
    placement buffer holding the prefix's pods."""
    if kind == "larger":
        shapes = _small() + [_shape(12, 20)]
        order = [2] * pre
    else:
        shapes = _small() + [_shape(10, 16, {EPH: MI_M}), _shape(10, 16, {EPH: 2 * MI_M})]
        order = [0, 1, 2, 3] + [2 + i % 2 for i in range(pre)]
    return _problem([catalog], [_m5()], shapes, order + [i % 2 for i in range(200)], f"edge-window-{kind}-{pre}")


def _pre_one_nodeclaim(prob, want):
    assert len(want["nodeclaims"]) == 1
    assert list(want["nodeclaims"][0]["pods"]) == list(_queue(prob))
    assert _run_witnesses(prob, want) >= 190
    return _class_bound(prob, want)


@pytest.mark.parametrize("pre,kind", F_PARAMS)
def test_window_inputs(catalog, pre, kind):
    prob, want = _case(catalog, build_window, pre, kind)
    bound = _pre_one_nodeclaim(prob, want)
    # (the 199 behind the first of the 200; larger: the prefix's own run; classes: the second of the four leading pods)
    assert bound == 199 + (max(pre - 1, 0) if kind == "larger" else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("pre,kind", F_PARAMS)
def test_window(ctx, catalog, ov, pre, kind):
    prob, want = _case(catalog, build_window, pre, kind)
    _all_variants(ctx, ov, prob, want, runs=True, bound=_pre_one_nodeclaim(prob, want))


G_PARAMS = [(n, lead) for n in (64, 65) for lead in (0, 60)]


def build_stretch(catalog, n, lead):
    """A stretch of exactly n pods of one class between two pods of another: k can reach 63 and no further, with the
    stretch starting at queue position 4 + lead (60: a multiple of the window). In front, one pod of each shape and
    `lead` pods alternating two more classes, committed pod by pod."""
    shapes = _small() + [_shape(10, 16, {EPH: MI_M}), _shape(10, 16, {EPH: 2 * MI_M})]
    order = [0, 1, 2, 3] + [2 + i % 2 for i in range(lead)] + [i % 2 for i in range(n)] + [2]
    order += [i % 2 for i in range(20)]
    return _problem([catalog], [_m5()], shapes, order, f"edge-stretch-{n}-{lead}")


def _pre_stretch(prob, want, n, lead):
    rc = _classes(prob)[0][prob.pod_shape[_queue(prob)]]
    cuts = np.nonzero(rc[1:] != rc[:-1])[0] + 1
    lens = np.diff(np.concatenate(([0], cuts, [len(rc)])))
    starts = np.concatenate(([0], cuts))
    assert [int(x) for x in lens[starts == 4 + lead]] == [n]
    assert len(want["nodeclaims"]) == 1 and _run_witnesses(prob, want) >= n - 1
    return _class_bound(prob, want)


@pytest.mark.parametrize("n,lead", G_PARAMS)
def test_stretch_inputs(catalog, n, lead):
    _pre_stretch(*_case(catalog, build_stretch, n, lead), n, lead)


@pytest.mark.gpu
@pytest.mark.parametrize("n,lead", G_PARAMS)
def test_stretch(ctx, catalog, ov, n, lead):
    prob, want = _case(catalog, build_stretch, n, lead)
    _all_variants(ctx, ov, prob, want, runs=True, bound=_pre_stretch(prob, want, n, lead))


# ---- g. ring wrap under batching -----------------------------------------------------------------------------------
PREFS = [(2, [(FAMILY, "In", ["c5"])]), (1, [(FAMILY, "In", ["r5"])])]  # neither can hold on an m5-only pool
N_RELAXED = 200


def build_ring_wrap(catalog, m):
    """200 pods of two shapes with two unsatisfiable preferred terms are placed on their third pass; the m pods in
    front of them (same class) are placed on the first. Each pass re-pushes the 200 behind the ring's tail, so the
    third starts at ring position n - m and its runs cross n_pods."""
    shapes = [_shape(), _shape(preferred_terms=list(PREFS)),
              _shape(preferred_terms=list(PREFS), required_terms=[list(ARCH)])]
    return _problem([catalog], [_m5()], shapes, [0] * m + [1 + i % 2 for i in range(N_RELAXED)], f"edge-ring-{m}")


def _pre_ring_wrap(catalog, prob, want, m):
    from oracle import pyoracle
    for _, term in PREFS:  # each term, required, leaves a pod unschedulable: both are relaxed before the pod fits
        key = ("pref", str(term))
        if key not in _CASES:
            one = _problem([catalog], [_m5()], [_shape(required_terms=[list(term)])], [0], "edge-ring-term")
            _CASES[key] = pyoracle.solve(one)
        assert _CASES[key]["placement"][0] < 0
    n = prob.n_pods
    assert (want["placement"] >= 0).all() and int(want["stats"]["pops"]) == n + 2 * N_RELAXED  # three pops each
    assert len(want["nodeclaims"]) == 1
    seq = list(want["nodeclaims"][0]["pods"])  # add order: the first pass's m pods, then the third pass
    assert seq == list(range(n))
    assert _run_witnesses(prob, want, seq) >= N_RELAXED - 10


@pytest.mark.parametrize("m", [1, 37, 63])
def test_ring_wrap_inputs(catalog, m):
    _pre_ring_wrap(catalog, *_case(catalog, build_ring_wrap, m), m)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 37, 63])
def test_ring_wrap(ctx, catalog, ov, m):
    """(No bound: pods re-queue, so the ring order is not the queue order.)"""
    prob, want = _case(catalog, build_ring_wrap, m)
    _pre_ring_wrap(catalog, prob, want, m)
    _all_variants(ctx, ov, prob, want, runs=True)


# ---- h. taint-set id >= 32 -----------------------------------------------------------------------------------------
N_TAINTED = 34


def build_taint_sets(catalog):
    """34 pools with distinct taints in input order, only the last tolerated (by shape 0 and by shape 2, which adds a
    required term); under them an untainted pool for shape 1, which has their request row and no toleration. The
    NodeClaim that the tolerating shapes fill has a taint-set id past 31. The queue of test_toleration_cuts_run. (The
    tolerating shapes also select their pool by name: in-flight NodeClaims are tried before templates, fewest pods
    first, so without it they would fill the untainted pool's NodeClaim as well, and mixed batches there read a low
    toleration bit.)"""
    from kpamd.model import NodePool
    pools = [NodePool(f"tainted-{i:02d}", 10, 0, list(M5), taints=[("dedicated", f"t{i:02d}", "NoSchedule")])
             for i in range(N_TAINTED)] + [NodePool("plain", 1, 0, list(M5))]
    tol = [("dedicated", "Equal", f"t{N_TAINTED - 1:02d}", "NoSchedule")]
    sel = {"karpenter.sh/nodepool": pools[N_TAINTED - 1].name}
    shapes = [_shape(tolerations=tol, node_selector=sel), _shape(),
              _shape(tolerations=tol, node_selector=sel, required_terms=[list(ARCH)])]
    order = [i % 3 for i in range(150)] + [0, 2, 0, 2, 1, 1] * 25
    return _problem([catalog], pools, shapes, order, "edge-taint-sets")


def _pre_taint_sets(prob, want):
    bound = _class_bound(prob, want)
    tolerated = N_TAINTED - 1
    assert tolerated >= 32 and prob.nodepools[tolerated].taints and not prob.nodepools[N_TAINTED].taints
    assert len({tuple(p.taints) for p in prob.nodepools}) == N_TAINTED + 1
    pool_of = np.array([n["nodepool"] for n in want["nodeclaims"]])[want["placement"]]
    assert (pool_of[prob.pod_shape == 1] == N_TAINTED).all() and (pool_of[prob.pod_shape != 1] == tolerated).all()
    assert _run_witnesses(prob, want) > 0
    q = _queue(prob)
    sh, pl = prob.pod_shape[q], want["placement"][q]
    single = int(np.sum((sh[1:] == sh[:-1]) & (pl[1:] == pl[:-1])))  # the most that commits of one level could take
    mixed = int(np.sum((sh[1:] != sh[:-1]) & (pl[1:] == pl[:-1])))
    assert mixed > single  # most neighbours on one NodeClaim are of different shapes: both tolerate the taint set
    return bound, single


def test_taint_sets_inputs(catalog):
    _pre_taint_sets(*_case(catalog, build_taint_sets))


@pytest.mark.gpu
def test_taint_sets(ctx, catalog, ov):
    """The forced run-length variants batch across the two tolerating shapes: more pods than there are neighbours of
    one shape on one NodeClaim (a toleration bit read from the low 32 bits would leave only those)."""
    prob, want = _case(catalog, build_taint_sets)
    bound, single = _pre_taint_sets(prob, want)

    def more(v, got):
        if v in (2, 3):
            assert got["stats"]["run_length_pods"] > single, (v, got["stats"]["run_length_pods"], single)
    _all_variants(ctx, ov, prob, want, runs=True, bound=bound, more=more)


# ---- i. spill after batches ----------------------------------------------------------------------------------------
def build_spill(catalog):
    """100 pods that batch onto the first NodeClaim, then 8 pods naming one host port (a NodeClaim each past the
    first), then 100 more: the NodeClaim order leaves LDS once it outgrows kp_overrides.sort_capacity, with cursors,
    a mutation stack and buffered placements that batches wrote."""
    shapes = [_shape(), _shape(required_terms=[list(ARCH)]), _shape(host_ports=[(None, 8080, "TCP")])]
    order = [i % 2 for i in range(100)] + [2] * 8 + [i % 2 for i in range(100)]
    return _problem([catalog], [_m5()], shapes, order, "edge-spill")


def _pre_spill(prob, want, sort_cap):
    assert len(want["nodeclaims"]) > sort_cap and len(want["nodeclaims"]) >= 8
    q = _queue(prob)
    assert (want["placement"][q[:100]] == 0).all()  # the first NodeClaim takes the first hundred, all of one class
    assert _run_witnesses(prob, want, q[:100]) >= 90
    return _class_bound(prob, want)


@pytest.mark.parametrize("sort_cap", [1, 3])
def test_spill_inputs(catalog, sort_cap):
    _pre_spill(*_case(catalog, build_spill), sort_cap)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_capacity,mode", [(0, MODE_CHUNKED), (-1, MODE_FLAT)])
@pytest.mark.parametrize("sort_cap", [1, 3])
def test_spill(ctx, catalog, ov, sort_cap, chunk_capacity, mode):
    """The chunked instantiation (chunk_capacity 0), or the full path on the flat order (-1: no chunks), continues
    where the run-length instantiation stopped."""
    prob, want = _case(catalog, build_spill)
    bound = _pre_spill(prob, want, sort_cap)

    def more(v, got):
        assert got["stats"]["order_chunks"][4] == mode, got["stats"]["order_chunks"]
    _all_variants(ctx, ov, prob, want, runs=True, bound=bound, more=more, sort_capacity=sort_cap,
                  chunk_capacity=chunk_capacity)


# ---- j. catalogue != 0 and minValues -------------------------------------------------------------------------------
def build_second_catalogue(catalog):
    """Two catalogues: the heavier pool on catalogue 1 (c5 only), the lighter on catalogue 0 (m5). One class; two
    shapes require m5 (catalogue-0 NodeClaims), two take either pool's NodeClaims."""
    from kpamd.model import NodePool
    cat1 = [it for it in catalog if _family(it) in ("c5", "m5", "r5")]
    pools = [NodePool("c5", 10, 1, [(FAMILY, "In", ["c5"]), ON_DEMAND]), NodePool("m5", 1, 0, list(M5))]
    shapes = [_shape(), _shape(required_terms=[list(ARCH)]), _shape(required_terms=[[(FAMILY, "In", ["m5"])]]),
              _shape(required_terms=[[(FAMILY, "In", ["m5"]), ARCH[0]]])]
    return _problem([catalog, cat1], pools, shapes, _blocks(300), "edge-catalogue")


def _pre_second_catalogue(prob, want):
    assert len({_row(s) for s in prob.shapes}) == 1
    pool_of = np.array([n["nodepool"] for n in want["nodeclaims"]])[want["placement"]]
    bound = _class_bound(prob, want)
    assert prob.nodepools[0].catalog == 1 and prob.nodepools[1].catalog == 0
    # the m5 shapes on catalogue 0 alone; the others open catalogue-1 NodeClaims and also join those of catalogue 0
    # (in-flight NodeClaims come before templates): pairs that could batch exist on both catalogues
    assert (pool_of[prob.pod_shape >= 2] == 1).all() and (pool_of[prob.pod_shape < 2] == 0).any()
    for pool in (0, 1):
        ncs = {i for i, n in enumerate(want["nodeclaims"]) if n["nodepool"] == pool}
        assert _run_witnesses(prob, want, only=ncs) > 0
    return bound


def build_min_values(catalog):
    """One pool with minValues on instance-family; two shapes of one class alternating."""
    from kpamd.model import NodePool
    pool = NodePool("flexible", 0, 0, [(FAMILY, "In", ["m5", "c5", "r5"], 2), ON_DEMAND])
    return _problem([catalog], [pool], [_shape(), _shape(required_terms=[list(ARCH)])], [i % 2 for i in range(300)],
                    "edge-minvalues")


def _pre_min_values(prob, want):
    assert prob.nodepools[0].requirements[0][3] == 2
    for n in want["nodeclaims"]:
        assert len({_family(prob.catalogs[0][t]) for t in n["options"]}) >= 2
    assert _run_witnesses(prob, want) > 0  # (they would batch, did the NodeClaim not carry minValues)
    return _class_bound(prob, want)


J_CASES = {"catalogue": (build_second_catalogue, _pre_second_catalogue),
           "minvalues": (build_min_values, _pre_min_values)}


@pytest.mark.parametrize("which", sorted(J_CASES))
def test_catalogue_minvalues_inputs(catalog, which):
    build, pre = J_CASES[which]
    pre(*_case(catalog, build))


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(J_CASES))
def test_catalogue_minvalues(ctx, catalog, ov, which):
    build, pre = J_CASES[which]
    prob, want = _case(catalog, build)
    _all_variants(ctx, ov, prob, want, bound=pre(prob, want))


# ---- k. random problems under the forced run-length variants -------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("n_catalogs", [1, 3, 10])
def test_forced_variants_on_random_problems(ctx, catalog, ov, n_catalogs, seed):
    """Limits, taints, minValues, relaxations, daemon requests, and pools on up to ten catalogues (ids past the eight
    LDS headers): parity under cont 1 and cont 2."""
    import kpamd
    from kpamd import synth
    from oracle import pyoracle
    from test_gpu_parity import check_same
    prob = synth.random_problem(catalog, 2600 + 10 * n_catalogs + seed, n_types=150, n_pods=1600,
                                n_pools=max(3, n_catalogs), n_shapes=6, n_catalogs=n_catalogs)
    want = pyoracle.solve(prob)
    for v in (2, 3):
        ov(fast_lane=v)
        got = kpamd.Scheduler(ctx, prob).solve()
        print(prob.name, "catalogues", n_catalogs, "fast_lane", v, "run_length_pods", got["stats"]["run_length_pods"])
        check_same(got, want)
