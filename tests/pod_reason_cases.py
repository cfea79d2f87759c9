"""Inputs and the plain reference for the per-NodePool reasons of unschedulable pods (test_pod_reasons.py).

`plain_reasons(problem, oracle_result)` restates what upstream `Scheduler.add` reports from `addToNewNodeClaim` for every
pod the oracle's Solve left unscheduled, one entry per NodeClaimTemplate, at the Solve's final state. It is plain Python
over the problem's InstanceType / Offering / NodePool / PodShape objects, built on the oracle's primitives only
(`pyoracle.requirements_compatible`, `pyoracle.requirements_intersects`) and numpy `alloc >= need`; no number in it comes
from the device.

What it models and what it does not:
* the final relaxation level is the fully relaxed pod: preferred terms and ScheduleAnyway spreads dropped, required
  node-affinity terms reduced to the last one, the PreferNoSchedule toleration appended when some NodePool carries such a
  taint (Preferences.Relax runs until nothing is left to relax before a pod stays failed);
* the merged requirements are the template's and the pod's requirement lists concatenated: the oracle's FromABI Adds
  entry by entry, which intersects a repeated key (pinned by a two-entry KAT in test_pod_reasons.py);
* remaining limits are the NodePool's limits minus, per NodeClaim the oracle created from the pool, the largest capacity
  over the NodeClaim's options as the result lists them. That equals subtractMax only when the options did not narrow
  after the NodeClaim's creation and were not truncated, which holds for the two limits builders (no NodeClaim at all;
  a one-type catalogue). The randomized problems carry no limits;
* topology counts are not modelled (code 4 never comes out of it): the topology KAT is asserted by hand.
"""
import copy
import functools

import numpy as np

from kpamd import abi, synth
from kpamd.model import ExistingNode, LabelSelector, NodePool, PodShape, Problem, TopologySpread

import feasibility_cases as fc
import scenarios

K = fc.K
IT = fc.IT
ARCH = fc.ARCH
ZONE = "topology.kubernetes.io/zone"
ZONE_ID = "topology.k8s.aws/zone-id"
CT = "karpenter.sh/capacity-type"
NODEPOOL = "karpenter.sh/nodepool"
TEAM = fc.TEAM
RES_ID = K + "capacity-reservation-id"
RES_TYPE = K + "capacity-reservation-type"
PNS = "PreferNoSchedule"
PNS_TOLERATION = ("", "Exists", "", PNS)
NONE, LIMITS, TAINT, REQUIREMENTS, TOPOLOGY, INSTANCE_TYPES, MIN_VALUES = range(7)
COUNTS = ("n_requirements", "n_fits", "n_offering", "n_requirements_fits", "n_requirements_offering", "n_fits_offering",
          "n_remaining")
HUGE = 1 << 62


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
def template_order(problem):
    """NodePool indices in the Solve's template order: weight descending, name ascending."""
    return sorted(range(len(problem.nodepools)), key=lambda i: (-problem.nodepools[i].weight, problem.nodepools[i].name))


def template_requirements(np_):
    """NewNodeClaimTemplate: spec requirements, then the template labels, then karpenter.sh/nodepool."""
    return list(np_.requirements) + [(k, "In", [v]) for k, v in np_.labels.items()] + [(NODEPOOL, "In", [np_.name])]


def offering_requirements(o):
    reqs = [(CT, "In", [o.capacity_type]), (ZONE, "In", [o.zone])]
    if o.zone_id:
        reqs.append((ZONE_ID, "In", [o.zone_id]))
    reqs.append((RES_ID, "In", [o.reservation_id]) if o.reservation_id else (RES_ID, "DoesNotExist", []))
    reqs.append((RES_TYPE, "In", [o.reservation_type]) if o.reservation_type else (RES_TYPE, "DoesNotExist", []))
    return reqs


def relaxed_shape(shape, pns_any):
    """The pod after every Preferences.Relax step that applies."""
    sh = copy.deepcopy(shape)
    sh.preferred_terms = []
    sh.preferred_affinity = []
    sh.preferred_anti_affinity = []
    sh.required_terms = sh.required_terms[-1:]
    sh.topology_spread = [t for t in sh.topology_spread if t.when_unsatisfiable != "ScheduleAnyway"]
    if pns_any and PNS_TOLERATION not in [tuple(t) for t in sh.tolerations]:
        sh.tolerations = list(sh.tolerations) + [PNS_TOLERATION]
    return sh


def pod_requirements(sh):
    """NewPodRequirements of a relaxed pod: nodeSelector, then the (first) required term; the volume requirements are
    appended to every required term (one is created when there is none)."""
    reqs = [(k, "In", [v]) for k, v in sh.node_selector.items()]
    term = list(sh.required_terms[0]) if sh.required_terms else []
    return reqs + term + list(sh.volume_requirements)


def tolerates(tol, taint):
    key, op, value, effect = tol
    if (effect or "") != "" and effect != taint[2]:
        return False
    if (key or "") != "" and key != taint[0]:
        return False
    if op in ("Equal", ""):
        return (value or "") == (taint[1] or "")
    return op == "Exists"


def first_untolerated(taints, tolerations):
    for i, t in enumerate(taints):
        if not any(tolerates(tol, t) for tol in tolerations):
            return i
    return -1


def _min_values_ok(its, idx, reqs):
    """SatisfiesMinValues over the types `idx`: per key with minValues, the distinct values the types carry."""
    need = {}
    for r in reqs:
        if len(r) > 3 and r[3] is not None:
            need[r[0]] = max(need.get(r[0], 0), int(r[3]))
    for key, n in need.items():
        vals = set()
        for t in idx:
            for r in its[t].requirements:
                if r[0] == key and r[1] == "In":
                    vals.update(r[2])
        if len(vals) < n:
            return False
    return True


class _Catalog:
    """Per catalogue: allocatable matrix and memoised oracle calls (a type's Intersects, an offering class's Compatible)."""

    def __init__(self, its):
        self.its = its
        self.alloc, present = fc.alloc_matrix(its)
        self.nonneg = ~(present & (self.alloc < 0)).any(axis=1)
        self.cap = np.zeros((len(its), abi.NUM_RES), dtype=np.int64)
        for t, it in enumerate(its):
            for k, v in it.capacity.items():
                self.cap[t, abi.RES_INDEX[k]] = int(v)
        self._memo = {}

    def criteria(self, merged, need):
        """(R, F, O) bool[T]: Intersects(type, merged); Fits(need, allocatable); an available offering Compatible."""
        from oracle import pyoracle
        key = (repr(merged), tuple(sorted(need.items())))
        if key in self._memo:
            return self._memo[key]
        T = len(self.its)
        R = np.array([pyoracle.requirements_intersects(it.requirements, merged) for it in self.its], dtype=bool)
        F = self.nonneg.copy()
        for k, v in need.items():
            F &= self.alloc[:, abi.RES_INDEX[k]] >= int(v)
        cls = {}
        O = np.zeros(T, dtype=bool)
        for t, it in enumerate(self.its):
            for o in it.offerings:
                if not o.available:
                    continue
                sig = (o.capacity_type, o.zone, o.zone_id, o.reservation_id, o.reservation_type)
                if sig not in cls:
                    cls[sig] = pyoracle.requirements_compatible(merged, offering_requirements(o), True)
                if cls[sig]:
                    O[t] = True
                    break
        self._memo[key] = (R, F, O)
        return R, F, O


def templates_of(problem, cats):
    """The Solve's templates: (nodepool index, requirements, options bool[T]) in template order; NodePools whose own
    requirements leave no instance type (or break their own minValues) have none."""
    out = []
    for i in template_order(problem):
        np_ = problem.nodepools[i]
        treqs = template_requirements(np_)
        c = cats[np_.catalog]
        R, F, O = c.criteria(treqs, {})
        opts = R & F & O
        if not opts.any() or not _min_values_ok(c.its, np.flatnonzero(opts), treqs):
            continue
        out.append((i, treqs, opts))
    return out


def _remaining_limits(problem, oracle_result, cats):
    rem = {}
    for i, np_ in enumerate(problem.nodepools):
        if np_.limits:
            rem[i] = {k: int(v) for k, v in np_.limits.items()}
    for nc in oracle_result["nodeclaims"]:
        i = nc["nodepool"]
        if i in rem and nc["options"]:
            cap = cats[problem.nodepools[i].catalog].cap
            for k in rem[i]:
                rem[i][k] -= int(cap[nc["options"], abi.RES_INDEX[k]].max())
    return rem


def plain_reasons(problem, oracle_result):
    """{pod: [reason dict per template]} for every pod the oracle left unscheduled (placement -1)."""
    from oracle import pyoracle
    cats = [_Catalog(c) for c in problem.catalogs]
    tmpls = templates_of(problem, cats)
    pns_any = any(t[2] == PNS for np_ in problem.nodepools for t in np_.taints)
    rem = _remaining_limits(problem, oracle_result, cats)
    by_shape = {}
    out = {}
    for p in np.flatnonzero(np.asarray(oracle_result["placement"]) == -1):
        s = int(problem.pod_shape[p])
        if s not in by_shape:
            by_shape[s] = _shape_reasons(problem, relaxed_shape(problem.shapes[s], pns_any), tmpls, cats, rem, pyoracle)
        out[int(p)] = copy.deepcopy(by_shape[s])
    return out


def _shape_reasons(problem, sh, tmpls, cats, rem, pyoracle):
    rows = []
    preqs = pod_requirements(sh)
    for i, treqs, opts in tmpls:
        np_ = problem.nodepools[i]
        c = cats[np_.catalog]
        row = {"nodepool": i, "code": NONE, "taint": -1, "keys": [], "n_types": 0}
        row.update({f: 0 for f in COUNTS})
        rows.append(row)
        X = opts.copy()
        if np_.limits:  # filterByRemainingResources: capacity <= remaining for every limited resource
            for k, v in rem[i].items():
                X &= c.cap[:, abi.RES_INDEX[k]] <= v
            if not X.any():
                row["code"] = LIMITS
                continue
        row["n_types"] = int(X.sum())
        ti = first_untolerated(np_.taints, sh.tolerations)
        if ti >= 0:
            row["code"], row["taint"] = TAINT, ti
            continue
        if not pyoracle.requirements_compatible(treqs, preqs, True):
            row["code"] = REQUIREMENTS
            row["keys"] = sorted({r[0] for r in preqs if not pyoracle.requirements_compatible(
                treqs, [q for q in preqs if q[0] == r[0]], True)}, key=lambda k: k.encode())
            continue
        merged = list(treqs) + list(preqs)
        need = {}
        for src in (np_.daemon_requests, sh.requests):
            for k, v in src.items():
                need[k] = need.get(k, 0) + int(v)
        R, F, O = c.criteria(merged, need)
        R, F, O = R & X, F & X, O & X
        row.update(n_requirements=int(R.sum()), n_fits=int(F.sum()), n_offering=int(O.sum()),
                   n_requirements_fits=int((R & F).sum()), n_requirements_offering=int((R & O).sum()),
                   n_fits_offering=int((F & O).sum()), n_remaining=int((R & F & O).sum()))
        if row["n_remaining"] == 0:
            row["code"] = INSTANCE_TYPES
        elif not _min_values_ok(c.its, np.flatnonzero(R & F & O), merged):
            row["code"] = MIN_VALUES
        else:
            row.update({f: 0 for f in COUNTS})
    return rows


# ---------------------------------------------------------------------------------------------------------------
# builders: 3 NodePools over a sized_catalog copy, a few pods; `fail` / `ok` are the pods the oracle must leave
# unscheduled / place; `expect` the hand-written reasons of every failing pod (exact fields; counts named in `zero` are
# 0, in `full` equal n_types, in `positive` > 0); `fixed` the same problem with the named cause removed, on which every
# pod of `fail` schedules
# ---------------------------------------------------------------------------------------------------------------
OD = [(CT, "In", ["on-demand"])]
SMALL = synth.req_res(500, 512)


def pools3(reqs=OD, **kw):
    return [NodePool(f"np-{c}", w, 0, list(reqs), **copy.deepcopy(kw)) for c, w in (("a", 30), ("b", 20), ("c", 10))]


def problem_of(its, pools, shapes, counts, name, **kw):
    s, c, u = scenarios.pods_of(counts)
    return Problem([its], pools, shapes, s, c, u, name=name, **kw)


class Case:
    def __init__(self, name, problem, fixed, fail, ok, expect, exact=True):
        self.name, self.problem, self.fixed, self.fail, self.ok, self.expect, self.exact = \
            name, problem, fixed, fail, ok, expect, exact


def _e(code, **kw):
    d = {"code": code}
    d.update(kw)
    return d


def _swap_shape(problem, i, shape):
    p = copy.deepcopy(problem)
    p.shapes[i] = shape
    return p


def _limits_small(its):
    """np-a and np-b: a cpu limit below every type's capacity. np-c is unlimited but tainted; only the twin tolerates it."""
    pools = pools3()
    pools[0].limits = {"cpu": 1}
    pools[1].limits = {"cpu": 1}
    pools[2].taints = [("dedicated", "twin", "NoSchedule")]
    shapes = [PodShape(dict(SMALL)), PodShape(dict(SMALL), tolerations=[("dedicated", "Exists", "", "NoSchedule")])]
    prob = problem_of(its, pools, shapes, [2, 1], "why-limits-small")
    fixed = copy.deepcopy(prob)
    fixed.nodepools[0].limits = {}
    return Case("limits-small", prob, fixed, [0, 1], [2], [_e(LIMITS, n_types=0), _e(LIMITS, n_types=0), _e(TAINT, taint=0)])


def _limits_exhausted(one):
    """A one-type catalogue; every pool's cpu limit is that type's capacity, so each pool's first NodeClaim takes its
    remaining budget to 0 (subtractMax): three big pods open the three NodeClaims, the fourth finds every pool exhausted.
    The small twin joins an open NodeClaim."""
    cpu = int(one[0].capacity["cpu"])
    big = int(one[0].allocatable()["cpu"] * 0.6)
    pools = pools3(limits={"cpu": cpu})
    shapes = [PodShape(synth.req_res(big, 512)), PodShape(dict(SMALL))]
    prob = problem_of(one, pools, shapes, [4, 1], "why-limits-exhausted")
    fixed = copy.deepcopy(prob)
    fixed.nodepools[2].limits = {}
    return Case("limits-exhausted", prob, fixed, [3], [0, 1, 2, 4], [_e(LIMITS, n_types=0)] * 3)


def _taint(its):
    """Two taints per pool; the pod tolerates the first only: taint == 1."""
    pools = pools3(taints=[("first", "1", "NoSchedule"), ("second", "1", "NoSchedule")])
    tol1 = [("first", "Exists", "", "")]
    shapes = [PodShape(dict(SMALL), tolerations=tol1),
              PodShape(dict(SMALL), tolerations=tol1 + [("second", "Equal", "1", "NoSchedule")])]
    prob = problem_of(its, pools, shapes, [2, 1], "why-taint")
    return Case("taint", prob, _swap_shape(prob, 0, copy.deepcopy(shapes[1])), [0, 1], [2], [_e(TAINT, taint=1)] * 3)


def _req_conflict(its):
    pools = pools3(labels={TEAM: "x"})
    shapes = [PodShape(dict(SMALL), node_selector={TEAM: "y"}), PodShape(dict(SMALL), node_selector={TEAM: "x"})]
    prob = problem_of(its, pools, shapes, [2, 1], "why-requirements-conflict")
    return Case("requirements-conflict", prob, _swap_shape(prob, 0, copy.deepcopy(shapes[1])), [0, 1], [2],
                [_e(REQUIREMENTS, keys=[TEAM])] * 3)


def _req_undefined_custom(its):
    key = "example.com/undefined"
    shapes = [PodShape(dict(SMALL), node_selector={key: "v"}), PodShape(dict(SMALL))]
    prob = problem_of(its, pools3(), shapes, [2, 1], "why-requirements-undefined")
    return Case("requirements-undefined-custom", prob, _swap_shape(prob, 0, PodShape(dict(SMALL))), [0, 1], [2],
                [_e(REQUIREMENTS, keys=[key])] * 3)


def _req_undefined_wellknown(its):
    """instance-type is well known and the pools do not define it: Compatible passes, no type intersects."""
    shapes = [PodShape(dict(SMALL), required_terms=[[(IT, "In", ["no-such.type"])]]), PodShape(dict(SMALL))]
    prob = problem_of(its, pools3(), shapes, [2, 1], "why-undefined-wellknown")
    return Case("undefined-wellknown", prob, _swap_shape(prob, 0, PodShape(dict(SMALL))), [0, 1], [2],
                [_e(INSTANCE_TYPES, zero=["n_requirements", "n_requirements_fits", "n_requirements_offering", "n_remaining"],
                    full=["n_fits", "n_offering", "n_fits_offering"])] * 3)


def _only_fits(its):
    shapes = [PodShape({"cpu": HUGE}), PodShape(dict(SMALL))]
    prob = problem_of(its, pools3(), shapes, [2, 1], "why-only-fits")
    return Case("only-fits", prob, _swap_shape(prob, 0, PodShape(dict(SMALL))), [0, 1], [2],
                [_e(INSTANCE_TYPES, zero=["n_fits", "n_requirements_fits", "n_fits_offering", "n_remaining"],
                    full=["n_requirements", "n_offering", "n_requirements_offering"])] * 3)


def _only_requirements(its):
    shapes = [PodShape(dict(SMALL), required_terms=[[(ARCH, "In", ["s390x"])]]), PodShape(dict(SMALL))]
    prob = problem_of(its, pools3(), shapes, [2, 1], "why-only-requirements")
    return Case("only-requirements", prob, _swap_shape(prob, 0, PodShape(dict(SMALL))), [0, 1], [2],
                [_e(INSTANCE_TYPES, zero=["n_requirements", "n_requirements_fits", "n_requirements_offering", "n_remaining"],
                    full=["n_fits", "n_offering", "n_fits_offering"])] * 3)


def _zone_out(its, zone):
    out = copy.deepcopy(its)
    for it in out:
        for o in it.offerings:
            if o.zone == zone:
                o.available = False
    return out


def _only_offerings(its):
    """The pod admits one zone, whose offerings are all unavailable."""
    zone = "test-zone-1b"
    shapes = [PodShape(dict(SMALL), node_selector={ZONE: zone}), PodShape(dict(SMALL))]
    prob = problem_of(_zone_out(its, zone), pools3(), shapes, [2, 1], "why-only-offerings")
    fixed = copy.deepcopy(prob)
    fixed.catalogs = [copy.deepcopy(its)]
    return Case("only-offerings", prob, fixed, [0, 1], [2],
                [_e(INSTANCE_TYPES, zero=["n_offering", "n_requirements_offering", "n_fits_offering", "n_remaining"],
                    full=["n_requirements", "n_fits", "n_requirements_fits"])] * 3)


def _all_three(its):
    zone = "test-zone-1b"
    shapes = [PodShape({"cpu": HUGE}, node_selector={ZONE: zone}, required_terms=[[(ARCH, "In", ["s390x"])]]),
              PodShape(dict(SMALL))]
    prob = problem_of(_zone_out(its, zone), pools3(), shapes, [2, 1], "why-all-three")
    return Case("all-three", prob, _swap_shape(prob, 0, PodShape(dict(SMALL))), [0, 1], [2],
                [_e(INSTANCE_TYPES, zero=list(COUNTS))] * 3)


def smallest_memory_type(its, pools=None):
    """The on-demand type with the least allocatable memory, and a memory request just above it."""
    a, _ = fc.alloc_matrix(its)
    mem = a[:, abi.RES_INDEX["memory"]]
    od = np.array([any(o.available and o.capacity_type == "on-demand" for o in it.offerings) for it in its])
    t = int(np.flatnonzero(od)[np.argmin(mem[od])])
    return t, int(mem[t]) + 1


def _pairwise(its):
    """instance-type In {a small type}, and a memory request only larger types fit: every criterion alone passes
    somewhere, requirements and Fits never together."""
    t, need = smallest_memory_type(its)
    shapes = [PodShape({"cpu": 100, "memory": need}, required_terms=[[(IT, "In", [its[t].name])]]), PodShape(dict(SMALL))]
    prob = problem_of(its, pools3(), shapes, [2, 1], "why-pairwise")
    return Case("pairwise", prob, _swap_shape(prob, 0, PodShape({"cpu": 100, "memory": need})), [0, 1], [2],
                [_e(INSTANCE_TYPES, n_requirements=1, n_requirements_offering=1, n_requirements_fits=0, n_remaining=0,
                    full=["n_offering"], positive=["n_fits", "n_fits_offering"])] * 3)


def _min_values(its):
    """Pool minValues 3 on instance-type; the pod narrows to 2 types: both pass every criterion, the set is too small."""
    pools = pools3(reqs=OD + [(IT, "Exists", [], 3)])
    a, _ = fc.alloc_matrix(its)
    fit = [i for i, it in enumerate(its) if a[i, 0] >= 2000 and a[i, 1] >= synth.MI * 1000 * 2048 and
           any(o.available and o.capacity_type == "on-demand" for o in it.offerings)]
    names = [its[i].name for i in fit[:3]]
    shapes = [PodShape(dict(SMALL), required_terms=[[(IT, "In", names[:2])]]), PodShape(dict(SMALL))]
    prob = problem_of(its, pools, shapes, [2, 1], "why-min-values")
    return Case("min-values", prob, _swap_shape(prob, 0, PodShape(dict(SMALL), required_terms=[[(IT, "In", names)]])),
                [0, 1], [2], [_e(MIN_VALUES, n_requirements=2, n_requirements_fits=2, n_requirements_offering=2, n_remaining=2,
                                 full=["n_offering"], positive=["n_fits"])] * 3)


def _final_preferred(its):
    """A preferred node affinity no type meets and a request nothing fits: the reasons are the relaxed pod's (the
    preference is gone, so every type meets the requirements)."""
    shapes = [PodShape({"cpu": HUGE}, preferred_terms=[(10, [(ARCH, "In", ["s390x"])])]), PodShape(dict(SMALL))]
    prob = problem_of(its, pools3(), shapes, [2, 1], "why-final-preferred")
    return Case("final-preferred", prob, _swap_shape(prob, 0, PodShape(dict(SMALL))), [0, 1], [2],
                [_e(INSTANCE_TYPES, zero=["n_fits", "n_remaining"], full=["n_requirements", "n_offering"])] * 3)


def _final_pns(its):
    """np-a and np-b carry a PreferNoSchedule taint, which the fully relaxed pod tolerates: no TAINT entry there.
    np-c's NoSchedule taint stays one."""
    pools = pools3()
    pools[0].taints = [("soft", "a", PNS)]
    pools[1].taints = [("soft", "b", PNS)]
    pools[2].taints = [("hard", "c", "NoSchedule")]
    shapes = [PodShape({"cpu": HUGE}), PodShape(dict(SMALL))]
    prob = problem_of(its, pools, shapes, [2, 1], "why-final-pns")
    return Case("final-pns", prob, _swap_shape(prob, 0, PodShape(dict(SMALL))), [0, 1], [2],
                [_e(INSTANCE_TYPES, zero=["n_fits"]), _e(INSTANCE_TYPES, zero=["n_fits"]), _e(TAINT, taint=0)])


WORD_EDGE_SIZES = [1, 63, 64, 65, 1100]


def _word_edge(its):
    """T types. Requirements fail on the last type alone (instance-type NotIn {it}) and pass on the rest of the last
    mask word; a memory request about half the types fit; the one admitted zone has no available offering, so no type
    passes all three and every count is reported."""
    T = len(its)
    zone = "test-zone-1b"
    a, _ = fc.alloc_matrix(its)
    mem = np.sort(a[:, abi.RES_INDEX["memory"]])
    need = int(mem[T // 2])
    shapes = [PodShape({"memory": need}, node_selector={ZONE: zone}, required_terms=[[(IT, "NotIn", [its[-1].name])]]),
              PodShape(dict(SMALL))]
    prob = problem_of(_zone_out(its, zone), pools3(reqs=[]), shapes, [2, 1], f"why-word-edge-{T}")
    return Case(f"word-edge-{T}", prob, _swap_shape(prob, 0, PodShape(dict(SMALL))), [0, 1], [2],
                [_e(INSTANCE_TYPES, n_offering=0, n_remaining=0, n_requirements_offering=0, n_fits_offering=0,
                    positive=["n_fits"], all_but_one=["n_requirements"])] * 3)


def _zone_node(its, name, zone, avail_cpu):
    it = its[0]
    labels = {IT: it.name, ZONE: zone, CT: "on-demand", ARCH: "amd64", "kubernetes.io/os": "linux",
              "kubernetes.io/hostname": name}
    return ExistingNode(name, labels, {"cpu": avail_cpu, "memory": synth.MI * 1000 * 64, "pods": 10}, {"cpu": 0, "pods": 0})


def topology_kat(its, pinned=True, min_domains=2, requests=None):
    """A DoNotSchedule zone spread, maxSkew 1, nodeAffinityPolicy Ignore; two matching pods are bound in zone a, none in
    the registered zone b. The pod is pinned to zone a and asks for more cpu than anything has.

    domainMinCount is taken over the domains the pod's own requirements admit (upstream nextDomainTopologySpread, and
    the oracle): pinned to zone a alone, the minimum would be zone a's own count and the skew 2 + 1 - 2 <= 1, so the
    pinned pod of the plain constraint schedules (test_topology_kat_on_the_oracle shows it). minDomains 2 is what makes
    the pinned pod fail on topology: it admits one domain, fewer than minDomains, so the minimum counts as 0 and the
    skew in zone a is 3. Every template then fails on topology, before its request (which nothing fits) is looked at.
    Not pinned, the pod admits every zone, the spread picks an empty one, and the request is what fails."""
    za, zb = "test-zone-1a", "test-zone-1b"
    sel = LabelSelector(match_labels={"app": "web"})
    spread = TopologySpread(ZONE, 1, sel, "DoNotSchedule", min_domains=min_domains, node_affinity_policy="Ignore")
    sh = PodShape(dict(requests or {"cpu": HUGE}), node_selector={ZONE: za} if pinned else {}, topology_spread=[spread],
                  labels={"app": "web"})
    nodes = [_zone_node(its, "node-a", za, 100), _zone_node(its, "node-b", zb, 100)]
    return problem_of(its, pools3(), [sh, PodShape(dict(SMALL))], [1, 1], "why-topology",
                      existing=nodes, bound_pods=[("default", {"app": "web"}, 0), ("default", {"app": "web"}, 0)])


BUILDERS = {
    "limits-small": _limits_small, "taint": _taint, "requirements-conflict": _req_conflict,
    "requirements-undefined-custom": _req_undefined_custom, "undefined-wellknown": _req_undefined_wellknown,
    "only-fits": _only_fits, "only-requirements": _only_requirements, "only-offerings": _only_offerings,
    "all-three": _all_three, "pairwise": _pairwise, "min-values": _min_values, "final-preferred": _final_preferred,
    "final-pns": _final_pns,
}
CASE_NAMES = list(BUILDERS) + ["limits-exhausted"] + [f"word-edge-{n}" for n in WORD_EDGE_SIZES]
BASE_TYPES = 48


@functools.lru_cache(maxsize=None)
def case(lib, name):
    """(Case, oracle result, plain_reasons of it): computed once per session and shared, never modified."""
    from oracle import pyoracle
    if name == "limits-exhausted":
        c = _limits_exhausted(copy.deepcopy(fc.sized_catalog(lib, 1)))
    elif name.startswith("word-edge-"):
        c = _word_edge(copy.deepcopy(fc.sized_catalog(lib, int(name.rsplit("-", 1)[1]))))
    else:
        c = BUILDERS[name](copy.deepcopy(fc.sized_catalog(lib, BASE_TYPES)))
    want = pyoracle.solve(c.problem)
    return c, want, plain_reasons(c.problem, want)


# ---------------------------------------------------------------------------------------------------------------
# randomized problems: preferences, taints (PreferNoSchedule included) and minValues; no limits, topology or
# reservations, so a pod's explanation is a function of (relaxed pod, template) alone
# ---------------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = [2, 5, 6, 17, 18, 19, 22, 23]  # chosen from the oracle alone (test_random_seeds_cover_the_codes)


@functools.lru_cache(maxsize=None)
def random_case(lib, seed):
    from oracle import pyoracle
    prob = synth.random_problem(_full_catalog(lib), seed, n_types=96, n_pods=36, n_pools=3, n_shapes=18, pns=0.4)
    for p in prob.nodepools:
        p.limits = {}
    want = pyoracle.solve(prob)
    return prob, want, plain_reasons(prob, want)


@functools.lru_cache(maxsize=None)
def _full_catalog(lib):
    from kpamd import catalog as cmod
    return cmod.build_catalog(lib)


def same_solve(a, b):
    return (np.array_equal(a["placement"], b["placement"]) and
            [(n["nodepool"], n["pods"], n["options"], n["n_remaining"], n["requirements"], n["requests"])
             for n in a["nodeclaims"]] ==
            [(n["nodepool"], n["pods"], n["options"], n["n_remaining"], n["requirements"], n["requests"])
             for n in b["nodeclaims"]])
