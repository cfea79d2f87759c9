"""Inputs and the plain reference for the OrderByPrice + Truncate edge tests (tests/test_option_order.py) - TEST
INFRASTRUCTURE.

Every result ends in the same step: order the NodeClaim's remaining instance types by (cheapest compatible available
offering, then name), cut to max types, re-check minValues. plain_options() states that step as a Python sort over the
Offering objects; it shares nothing with oracle.cpp or with the device's encoding (price bits as the key, the name rank
packed above the type index, padding keys). The builders take catalogues from feasibility_cases.sized_catalog through
copy.deepcopy and overwrite offering prices and availability (and, where a case needs names in a chosen byte order, a
type's name together with its instance-type requirement) on the Python objects.

The Solve harness: one NodePool per wanted NodeClaim, selected by a label, carrying instance-type In [the chosen
types] and a capacity-type requirement; one tiny pod per NodePool pinned to one zone. The NodeClaim's remaining set is
then exactly the chosen types that have an available offering of that zone and capacity type and hold the pod."""
import copy
import functools
import math
import sys

import numpy as np

from feasibility_cases import FOUR_ZONES, sized_catalog

IT = "node.kubernetes.io/instance-type"
CT = "karpenter.sh/capacity-type"
ZONE = "topology.kubernetes.io/zone"
FAMILY = "karpenter.k8s.aws/instance-family"
CLAIM = "example.com/claim"
OD = ("on-demand",)
ZA, ZB, ZC = "test-zone-1a", "test-zone-1b", "test-zone-1c"
TINY = (10, 16)  # the pod: 10m / 16Mi
SUBNORMAL = 5e-324
ULP_UP = math.nextafter(1.0, 2.0)
ULP_DOWN = math.nextafter(1.0, 0.0)
PALETTE = [1.0, 0.0, 1e300, ULP_UP, SUBNORMAL]  # the tie recipe: five prices in turn, so every fifth type ties
COUNTS = [1, 2, 63, 64, 65, 99, 100, 101, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]


# ---- the plain reference -------------------------------------------------------------------------------------------
def cheapest(it, zones, capacity_types):
    """The cheapest available offering of the allowed zones and capacity types, else the largest float."""
    return min((o.price for o in it.offerings if o.available and o.zone in zones and o.capacity_type in capacity_types),
               default=sys.float_info.max)


def plain_options(its, remaining, zones, capacity_types, max_types):
    """OrderByPrice + Truncate of the remaining type indices: by (cheapest, name bytes); max_types 0 cuts nothing."""
    out = sorted(remaining, key=lambda t: (cheapest(its[t], zones, capacity_types), its[t].name.encode()))
    return out[:max_types] if max_types else out


def holds_tiny_pod(it):
    a = it.allocatable()
    return all(v >= 0 for v in a.values()) and a.get("cpu", 0) >= TINY[0] \
        and a.get("memory", 0) >= TINY[1] * (1 << 20) * 1000 and a.get("pods", 0) >= 1000


def offered(it, zone, capacity_types=OD):
    return any(o.available and o.zone == zone and o.capacity_type in capacity_types for o in it.offerings)


def usable(its, zone=ZA, capacity_types=OD):
    """The types a tiny pod pinned to the zone can launch on with one of the capacity types, in catalogue order."""
    return [t for t, it in enumerate(its) if holds_tiny_pod(it) and offered(it, zone, capacity_types)]


def offering_classes(its):
    """Distinct (capacity type, zone, reservation) over the catalogue's offerings: the device gathers the cheapest
    price of a class subset from one table up to KP_SUB_MAX_C classes and loops over the class rows past it."""
    return len({(o.capacity_type, o.zone, o.reservation_id) for it in its for o in it.offerings})


# ---- catalogues ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base(lib, n, n_zones):
    kw = {} if n_zones == 3 else {"zones": FOUR_ZONES[0][:n_zones], "zone_ids": FOUR_ZONES[1][:n_zones]}
    return sized_catalog(lib, n, **kw)


def fresh(lib, n=1100, n_zones=3):
    """A private copy of the n-type catalogue: the caller edits its offerings."""
    return copy.deepcopy(_base(lib, n, n_zones))


def rename(it, name):
    """The type under another name (its instance-type requirement follows, as computeRequirements derives it)."""
    it.requirements = [(IT, "In", [name]) if r[0] == IT else r for r in it.requirements]
    it.name = name


def set_prices(its, prices, zone=ZA, capacity_type="on-demand", elsewhere=0.0):
    """prices[t] on type t's offering of (capacity_type, zone). Every other offering of every type gets `elsewhere`:
    the cheapest price there is, in zones and capacity types the NodeClaim does not admit, so it must not count."""
    for t, it in enumerate(its):
        for o in it.offerings:
            if o.reservation_id is not None:
                continue  # (a reserved offering keeps createOfferings' price)
            if o.capacity_type == capacity_type and o.zone == zone:
                if t in prices:
                    o.price = prices[t]
            else:
                o.price = elsewhere


def palette_prices(ts, shift=0):
    """The tie recipe: PALETTE in turn over the types."""
    return {t: PALETTE[(j + shift) % len(PALETTE)] for j, t in enumerate(ts)}


# ---- the Solve harness ---------------------------------------------------------------------------------------------
def claim(types, zone=ZA, capacity_types=OD, catalog=0, extra=()):
    return {"types": list(types), "zone": zone, "cts": tuple(capacity_types), "catalog": catalog, "extra": list(extra)}


def solve_problem(cats, claims, max_types=100, name="option-order"):
    from kpamd import synth
    from kpamd.model import NodePool, PodShape, Problem
    pools, shapes = [], []
    for i, c in enumerate(claims):
        its = cats[c["catalog"]]
        reqs = [(IT, "In", [its[t].name for t in c["types"]]), (CT, "In", list(c["cts"]))] + c["extra"]
        pools.append(NodePool(f"claim-{i:02d}", 0, c["catalog"], reqs, labels={CLAIM: f"c{i:02d}"}))
        shapes.append(PodShape(synth.req_res(*TINY), node_selector={CLAIM: f"c{i:02d}", ZONE: c["zone"]}))
    n = len(claims)
    return Problem(list(cats), pools, shapes, np.arange(n, dtype=np.uint32),
                   (1_750_000_000 + np.arange(n)).astype(np.int64), np.arange(1, n + 1, dtype=np.uint64),
                   max_instance_types=max_types, name=name)


def plain_claim(cats, c, max_types):
    """(remaining count, options) the plain reference gives a claim."""
    its = cats[c["catalog"]]
    remaining = [t for t in c["types"] if holds_tiny_pod(its[t]) and offered(its[t], c["zone"], c["cts"])]
    return len(remaining), plain_options(its, remaining, [c["zone"]], c["cts"], max_types)


def by_claim(res):
    """NodeClaim of each claim (its NodePool's index), or None where the claim's pod failed."""
    out = {}
    for n in res["nodeclaims"]:
        assert n["nodepool"] not in out and len(n["pods"]) == 1
        out[n["nodepool"]] = n
    return out


def assert_plain(cats, claims, max_types, res):
    """The oracle's (or any) Solve result against the plain reference, claim by claim."""
    got = by_claim(res)
    assert sorted(got) == list(range(len(claims)))
    for i, c in enumerate(claims):
        n_rem, opts = plain_claim(cats, c, max_types)
        assert got[i]["n_remaining"] == n_rem, (i, got[i]["n_remaining"], n_rem)
        assert got[i]["options"] == opts, f"claim {i}: options differ from the plain sort"


# ---- A. option-count edges -----------------------------------------------------------------------------------------
def build_counts(lib, n_zones):
    """One claim per count on the 1,100-type catalogue, the first n usable types each, and the whole usable set; the
    tie recipe on the pinned zone's on-demand offering (shifted per count, so the tie groups fall differently)."""
    its = fresh(lib, 1100, n_zones)
    us = usable(its)
    set_prices(its, palette_prices(us))
    return [its], [claim(us[:n]) for n in COUNTS] + [claim(us)]


def build_two_catalogues(lib):
    """A 65-type and the 1,100-type catalogue whose shared names carry different prices; a claim on each over those
    names: the option rows' stride is the larger T, the smaller catalogue's name ranks and masks end at 65."""
    small, large = fresh(lib, 65), fresh(lib, 1100)
    us_s = usable(small)
    index = {it.name: t for t, it in enumerate(large)}
    us_l = [index[small[t].name] for t in us_s]
    assert us_l == [t for t in us_l if t in set(usable(large))]
    set_prices(small, palette_prices(us_s))
    set_prices(large, palette_prices(us_l, shift=2))
    return [small, large], [claim(us_s, catalog=0), claim(us_l, catalog=1), claim(usable(large), catalog=1)]


# ---- B. ties and price values --------------------------------------------------------------------------------------
N_EQUAL = 257


def equal_types(its):
    """257 usable types among which byte order of the name, catalogue index order and numeric order all differ: the
    first clones renamed onto one stem (...-clone10 sorts before ...-clone9), the c5 and m5 families (.12xlarge before .2xlarge,
    .metal), filled up from the catalogue's end."""
    clones = [t for t, it in enumerate(its) if "-clone" in it.name]
    for t in clones[:24]:
        rename(its[t], "c5.large-clone" + its[t].name.rsplit("-clone", 1)[1])
    us = usable(its)
    pick = [t for t in us if its[t].name.startswith(("c5.", "m5."))]
    pick += [t for t in reversed(us) if t not in set(pick)][:N_EQUAL - len(pick)]
    return sorted(pick)


def build_all_equal(lib, price=1.0):
    its = fresh(lib)
    ts = equal_types(its)
    set_prices(its, {t: price for t in ts})
    return [its], [claim(ts)]


def build_signed_zeros(lib):
    """The all-equal case at price zero, every other type's zero negative: equal under <, unequal as bits."""
    its = fresh(lib)
    ts = equal_types(its)
    set_prices(its, {t: (-0.0 if j % 2 else 0.0) for j, t in enumerate(ts)})
    return [its], [claim(ts)]


def build_tie_across_cut(lib, cut=100, n=140):
    """n types in a shuffled order: sorted positions cut-10 .. cut+15 (0-based cut-11 .. cut+14) share one price,
    distinct cheaper prices before them and distinct dearer ones after. Which of the group survive is the name's."""
    its = fresh(lib)
    us = usable(its)
    ts = [us[i] for i in np.random.default_rng(11).permutation(len(us))[:n]]
    lo, hi = cut - 11, cut + 15
    prices = {}
    for j, t in enumerate(ts):
        prices[t] = 0.25 + j / 1024 if j < lo else 1.0 if j < hi else 2.0 + j / 1024
    set_prices(its, prices)
    return [its], [claim(sorted(ts))]


def ulp_keys(real):
    """Prices one ulp apart: chains of nine around 1.0 and around a real on-demand price, interleaved so that the
    catalogue order is not the price order and neighbours in it come from the two chains."""
    def chain(x):
        down, up = [x], [x]
        for _ in range(4):
            down.append(math.nextafter(down[-1], 0.0))
            up.append(math.nextafter(up[-1], math.inf))
        return down[:0:-1] + up
    a, b = chain(1.0), chain(real)
    order = [3, 7, 0, 5, 8, 1, 6, 2, 4]
    return [x for i in order for x in (a[i], b[i])]


def build_ulp(lib):
    its = fresh(lib)
    us = usable(its)
    real = next(o.price for o in its[us[0]].offerings if o.capacity_type == "on-demand" and o.zone == ZA)
    keys = ulp_keys(real)
    ts = us[5:5 + len(keys)]
    set_prices(its, dict(zip(ts, keys)))
    return [its], [claim(ts)], keys


N_RESERVED = 12


def build_extremes(lib):
    """0.0, the two smallest subnormals, 1e300 and the reserved-offering scale in one on-demand list (the prices
    createOfferings gives the reserved offerings, on-demand / 1e7, copied onto on-demand offerings); and a second claim
    that admits reserved capacity alone over types with capacity reservations, so that its keys are the reserved
    offerings' own prices. (A claim admitting reserved next to other capacity types orders by what it can reserve: not
    a plain price sort, and not pinned here.)"""
    from kpamd import catalog as cmod
    base = _base(lib, 1100, 3)
    us0 = usable(base)
    reserved = us0[40:40 + N_RESERVED]
    crs = tuple(cmod.CapacityReservation(f"cr-{base[t].name}", base[t].name, ZA, "default", 3) for t in reserved)
    its = copy.deepcopy(sized_catalog(lib, 1100, capacity_reservations=crs))
    scale = [o.price for t in reserved for o in its[t].offerings if o.reservation_id is not None]
    ts = us0[:120]
    values = [0.0, SUBNORMAL, 1e300, 1.0, 2 * SUBNORMAL] + scale
    set_prices(its, {t: values[(7 * j) % len(values)] for j, t in enumerate(ts)})
    return [its], [claim(ts), claim(us0[30:60], capacity_types=("reserved",))]


def build_zone_reversal(lib, n=100):
    """n types whose on-demand price order in zone A is the reverse of that in zone B, and both differ from the order
    by the cheapest offering over all zones (zone C holds that minimum, in yet another order). Type 0 of the set is
    unavailable in A; a pod pinned to A and one pinned to B."""
    its = fresh(lib)
    ts = usable(its)[:n]
    perm = np.random.default_rng(5).permutation(n)
    for j, t in enumerate(ts):
        for o in its[t].offerings:
            if o.capacity_type != "on-demand":
                o.price = 0.0
            elif o.zone == ZA:
                o.price = 1.0 + j / 256
            elif o.zone == ZB:
                o.price = 1.0 + (n - 1 - j) / 256
            else:
                o.price = 0.5 + int(perm[j]) / 1024
    for o in its[ts[0]].offerings:
        if o.zone == ZA:
            o.available = False
    return [its], [claim(ts, zone=ZA), claim(ts, zone=ZB)]


MIN_FAMILIES_CUT = 100


def build_min_values_tie(lib, swapped):
    """101 types: 99 cheap ones and Y from k - 1 families, X from a k-th family; X and Y tie on price at sorted
    positions 100 and 101. The NodePool asks for k families. X's name sorts first: the cut keeps X and k families.
    swapped: X and Y trade names (each keeps its family), the cut keeps Y and k - 1 families."""
    its = fresh(lib)
    us = usable(its)
    fam = {t: next(r[2][0] for r in its[t].requirements if r[0] == FAMILY and r[2]) for t in us
           if any(r[0] == FAMILY and r[1] == "In" and r[2] for r in its[t].requirements) and "-clone" not in its[t].name}
    chosen, fams = [], []
    for t in us:
        if t in fam and len(chosen) < MIN_FAMILIES_CUT:
            if fam[t] not in fams:
                if len(chosen) + sum(1 for u in fam if fam[u] == fam[t]) > MIN_FAMILIES_CUT:
                    continue  # (whole families only, so that the k - 1 are exactly those of the cheap hundred)
                fams.append(fam[t])
            chosen.append(t)
    assert len(chosen) == MIN_FAMILIES_CUT, len(chosen)
    y = chosen[-1]
    x = next(t for t in us if t in fam and fam[t] not in fams)
    k = len(fams) + 1
    if (its[x].name.encode() < its[y].name.encode()) == bool(swapped):
        nx, ny = its[x].name, its[y].name
        rename(its[x], ny)
        rename(its[y], nx)
    prices = {t: 0.25 + j / 1024 for j, t in enumerate(chosen[:-1])}
    prices[x] = prices[y] = 1.0
    set_prices(its, prices)
    return [its], [claim(sorted(chosen + [x]), extra=[(FAMILY, "Exists", [], k)])], k, x, y


# ---- C. consolidation clusters -------------------------------------------------------------------------------------
P = 1.0  # the candidates' price
POD = (500, 1024)  # a cluster pod: 500m / 1Gi
HOLES = (10, 50, 62, 66, 98)  # sorted positions whose zone-B offering costs P: cheap, yet their worst launch is not < P
LENGTHS = [513, 1, 129, 63, 128, 64, 127, 65, 100]  # one node each, in this order (a long list, then the shortest)


def holds(it, cpu, mem_mi, pods=1):
    a = it.allocatable()
    return all(v >= 0 for v in a.values()) and a.get("cpu", 0) >= cpu * pods \
        and a.get("memory", 0) >= mem_mi * (1 << 20) * 1000 * pods and a.get("pods", 0) >= 1000 * pods


def position_prices(n, down_from, at_from, up_from):
    """Prices by intended sorted position: distinct and rising, but for a tie group over positions 60-69 (it straddles
    the 64-lane halves), one at P - ulp over [down_from, at_from), one at P over [at_from, up_from) and one at P + ulp
    from there on."""
    out = []
    for j in range(n):
        if j >= up_from:
            out.append(ULP_UP)
        elif j >= at_from:
            out.append(P)
        elif j >= down_from:
            out.append(ULP_DOWN)
        elif 60 <= j < 70:
            out.append(0.5)
        else:
            out.append((0.25 if j < 60 else 0.75) + j / 4096)
    return out


def price_everywhere(its, ts, prices, holes=()):
    """On-demand price prices[j] of type ts[j] in every zone (zone B: P at the hole positions); every spot offering
    and every other type's on-demand offering at 0.0 (cheaper: the pool admits on-demand, the lists name ts)."""
    at = {t: j for j, t in enumerate(ts)}
    for t, it in enumerate(its):
        for o in it.offerings:
            if o.reservation_id is not None:
                continue
            j = at.get(t)
            if o.capacity_type != "on-demand" or j is None:
                o.price = 0.0
            else:
                o.price = P if (j in holes and o.zone == ZB) else prices[j]


def shuffled_usable(its, n, seed, cpu=POD[0], mem_mi=POD[1], pods=1, skip=()):
    us = [t for t in usable(its) if holds(its[t], cpu, mem_mi, pods) and t not in set(skip)]
    return [us[i] for i in np.random.default_rng(seed).permutation(len(us))[:n]]


def candidate_type(its):
    """The type of the candidate nodes where they are not options themselves."""
    return next(t for t in usable(its) if its[t].name == "m5.2xlarge")


def price_on_demand(it, price):
    for o in it.offerings:
        if o.capacity_type == "on-demand":
            o.price = price


def make_cluster(its, nodes, shapes, pool_reqs, name, zone_of=None):
    """nodes: (type index, [shape index per pod]); one NodePool admitting on-demand capacity plus pool_reqs; every
    node is full (nothing else lands on it), on demand, in zone A (zone_of: per node)."""
    from kpamd import catalog as cmod, synth
    from kpamd.model import Cluster, ClusterNode, ExistingNode, NodePool
    cnodes, pod_shape = [], []
    for i, (t, shs) in enumerate(nodes):
        z = cmod.ZONES.index(zone_of[i]) if zone_of else 0
        labels = synth.node_labels(its[t], z, "on-demand", "default", f"node-{i:05d}")
        pods = list(range(len(pod_shape), len(pod_shape) + len(shs)))
        pod_shape += shs
        cnodes.append(ClusterNode(ExistingNode(f"node-{i:05d}", labels, {"cpu": 0, "memory": 0, "pods": 0}, {}, [], True),
                                  0, t, pods))
    n = len(pod_shape)
    pool = NodePool("default", 0, 0, [(CT, "In", ["on-demand"])] + list(pool_reqs))
    return Cluster([its], [pool], cnodes, shapes, np.asarray(pod_shape, dtype=np.uint32),
                   (1_750_000_000 + np.arange(n)).astype(np.int64), np.arange(1, n + 1, dtype=np.uint64),
                   candidates=list(range(len(cnodes))), name=name)


def _pod_shape(res=POD, **kw):
    from kpamd import synth
    from kpamd.model import PodShape
    return PodShape(synth.req_res(*res), **kw)


def _spread(shapes):
    """A hostname topology spread over the shape's own label on every shape: the plan takes the general path. (One
    pod per new NodeClaim or existing node keeps maxSkew 1 wherever it lands; nothing else changes.)"""
    from kpamd.model import LabelSelector, TopologySpread
    for i, sh in enumerate(shapes):
        sh.labels = {"app": f"app-{i}"}
        sh.topology_spread = [TopologySpread("kubernetes.io/hostname", 1, LabelSelector({"app": f"app-{i}"}),
                                             "DoNotSchedule")]


def build_price_boundary(lib, spread=False):
    """One candidate at P whose pod may go to 140 types (the NodePool's instance-type In): the sorted list holds
    P - ulp at positions 80-89, P at 90-96 and P + ulp from 97, all inside the cut at 100; HOLES cost P in zone B."""
    its = fresh(lib)
    cand = candidate_type(its)
    ts = shuffled_usable(its, 140, 21, skip=[cand])
    price_everywhere(its, ts, position_prices(140, 80, 90, 97), HOLES)
    price_on_demand(its[cand], P)
    shapes = [_pod_shape()]
    if spread:
        _spread(shapes)
    cl = make_cluster(its, [(cand, [0])], shapes, [(IT, "In", [its[t].name for t in ts])], "order-price-boundary")
    return cl, [[0]], ts


def build_same_type(lib, spread=False):
    """Two candidates, an X at P and a Y at 2: together 3, so filterByPrice keeps the whole cut; X is among the kept
    options, so filterOutSameType caps the price at P exactly: the options at P (X and its ties) go, P - ulp stays."""
    its = fresh(lib)
    ts = shuffled_usable(its, 140, 22, pods=2)
    price_everywhere(its, ts, position_prices(140, 80, 90, 97))
    x, y = ts[92], ts[120]
    price_on_demand(its[y], 2.0)
    shapes = [_pod_shape(), _pod_shape()]
    if spread:
        _spread(shapes)
    cl = make_cluster(its, [(x, [0]), (y, [1])], shapes, [(IT, "In", [its[t].name for t in ts])], "order-same-type")
    return cl, [[0, 1], [0], [1]], ts


def build_lengths(lib, spread=False):
    """One candidate per list length n (LENGTHS): its pod's node affinity names the first n positions of one price
    layout (ties over positions 60-69 and, at P - ulp, over 95-110, straddling the cut; HOLES in both lane halves)."""
    its = fresh(lib)
    cand = candidate_type(its)
    ts = shuffled_usable(its, max(LENGTHS), 23, skip=[cand])
    price_everywhere(its, ts, position_prices(len(ts), 95, 111, 121), HOLES)
    price_on_demand(its[cand], P)
    shapes = [_pod_shape(required_terms=[[(IT, "In", [its[t].name for t in ts[:n]])]]) for n in LENGTHS]
    if spread:
        _spread(shapes)
    cl = make_cluster(its, [(cand, [i]) for i in range(len(LENGTHS))], shapes, [], "order-lengths")
    return cl, [[i] for i in range(len(LENGTHS))], ts


def plain_kept(cl, ts, n, cand_price, pods=1):
    """What the plain reference keeps for a replacement over the first n of ts: its sort cut to 100, then the options
    whose dearest on-demand offering is strictly below the price."""
    its = cl.catalogs[0]
    zones = sorted({o.zone for it in its for o in it.offerings})
    opts = plain_options(its, [t for t in ts[:n] if holds(its[t], *POD, pods)], zones, OD, 100)
    worst = {t: max(o.price for o in its[t].offerings if o.available and o.capacity_type == "on-demand") for t in opts}
    return opts, [t for t in opts if worst[t] < cand_price], worst


# ---- E. Drift ------------------------------------------------------------------------------------------------------
def build_drift(lib):
    """One drifted node with two pods: one may go to a single type in zone A, the other to the 257 all-equal types in
    zone B: its replace-all simulation makes two NodeClaims with 1 and 257 remaining types."""
    its = fresh(lib)
    ts = equal_types(its)
    cand = candidate_type(its)
    for t in ts:
        for o in its[t].offerings:
            o.price = P if o.capacity_type == "on-demand" else 0.0
    names = [its[t].name for t in ts]
    shapes = [_pod_shape(TINY, node_selector={ZONE: ZA}, required_terms=[[(IT, "In", names[128:129])]]),
              _pod_shape(TINY, node_selector={ZONE: ZB}, required_terms=[[(IT, "In", names)]])]
    return make_cluster(its, [(cand, [0, 1])], shapes, [], "order-drift"), [[0]], ts


# ---- F. launch selection -------------------------------------------------------------------------------------------
LAUNCH_M = [63, 64, 65, 128, 129]


def is_exotic(it):
    """ExoticInstanceTypeFilter's notion: a metal size, or an accelerator in the capacity."""
    size = next((r[2][0] for r in it.requirements if r[0] == "karpenter.k8s.aws/instance-size" and r[2]), "")
    return "metal" in size or any(it.capacity.get(k, 0) for k in (
        "aws.amazon.com/neuron", "aws.amazon.com/neuroncore", "amd.com/gpu", "nvidia.com/gpu", "habana.ai/gaudi"))


def build_launch(lib):
    """One catalogue, three groups of launch requests (requirements, requests, type list), all pinned to zone A:
    sizes   on-demand, the first m of a generic list whose sorted positions 55-66 tie at P - ulp, across the cut at 60;
    exotic  on-demand with minValues (the exotic filter is skipped): metal and generic types, all at P;
    spot    spot or on-demand: the cheapest on-demand price is M; spot offerings below M, at M and one ulp above."""
    from kpamd import synth
    its = fresh(lib)
    us = usable(its)
    generic = [t for t in us if not is_exotic(its[t])]
    ts = [generic[i] for i in np.random.default_rng(31).permutation(len(generic))[:max(LAUNCH_M)]]
    prices = dict(zip(ts, position_prices(len(ts), 55, 67, 80)))
    metal = [t for t in us if is_exotic(its[t]) and "metal" in its[t].name and t not in prices][:8]
    plain = [t for t in generic if t not in prices][:40]
    exo = sorted(metal + plain[:12])
    prices.update({t: P for t in exo})
    spot = plain[12:40]
    M = 0.5
    prices.update({t: M + j for j, t in enumerate(spot)})  # on demand: spot[0] is the cheapest, at M
    set_prices(its, prices)
    spot_price = [M, math.nextafter(M, math.inf), math.nextafter(M, 0.0), 0.25]
    for j, t in enumerate(spot):
        for o in its[t].offerings:
            if o.capacity_type == "spot":  # zone A alone counts (the request pins it); the others stay at 0.0
                o.price = spot_price[j % 4] if o.zone == ZA else 0.0
    res = synth.req_res(*TINY)
    zone = (ZONE, "In", [ZA])
    sizes = [([(CT, "In", ["on-demand"]), zone], res, list(ts[:m])) for m in LAUNCH_M]
    exotic = [([(CT, "In", ["on-demand"], 1), zone], res, list(exo))]
    spots = [([(CT, "In", ["spot", "on-demand"]), zone], res, list(spot))]
    return its, {"sizes": sizes, "exotic": exotic, "spot": spots}, {"M": M, "spot": spot, "exo": exo, "metal": metal}
