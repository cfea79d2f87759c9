"""Inputs and plain references for the CompatibleAvailableFilter edge tests (test_feasibility_oracle.py on the CPU,
test_gpu_feasibility_edges.py on the device): Fits-threshold sweeps, sub-catalogues with a chosen number of distinct
allocatable values, catalogues of a chosen size, and a numpy statement of resources.Fits for requirement-free rows.
"""
import copy
import functools

import numpy as np

from kpamd import abi
from kpamd import catalog as cmod

K = "karpenter.k8s.aws/"
IT = "node.kubernetes.io/instance-type"
ARCH = "kubernetes.io/arch"
TEAM = "example.com/team"
FOUR_ZONES = (["test-zone-1a", "test-zone-1b", "test-zone-1c", "test-zone-1d"],
              ["tstz1-1a", "tstz1-1b", "tstz1-1c", "tstz1-1d"])
DISTINCT_COUNTS = [1, 2, 16, 17, 256, 257]  # the 16-ary lower bound's level boundaries (16, 16^2) and one past each
SIZES = [1, 63, 64, 65, 511, 512, 513, 919, 1023, 1024, 1025, 1100]


def alloc_matrix(its):
    """InstanceType.Allocatable() as int64[T, NUM_RES] (0 where the type lacks the resource) and the mask of the
    resources each type's capacity names (resources.Subtract keeps the capacity's keys)."""
    a = np.zeros((len(its), abi.NUM_RES), dtype=np.int64)
    present = np.zeros((len(its), abi.NUM_RES), dtype=bool)
    for t, it in enumerate(its):
        for k, v in it.capacity.items():
            r = abi.RES_INDEX[k]
            a[t, r] = int(v) - int(it.overhead.get(k, 0))
            present[t, r] = True
    return a, present


def numpy_filter(its, queries):
    """CompatibleAvailableFilter for rows without requirements, in numpy: resources.Fits (no negative allocatable;
    alloc[t][r] >= need for every requested r) and an available offering; the cheapest available offering's price.
    Returns (kept bool[Q,T], cheapest f64[Q,T])."""
    assert all(not reqs for reqs, _ in queries)
    a, present = alloc_matrix(its)
    nonneg = ~(present & (a < 0)).any(axis=1)
    price = np.array([min([o.price for o in it.offerings if o.available], default=np.inf) for it in its])
    avail = np.array([any(o.available for o in it.offerings) for it in its], dtype=bool)
    kept = np.zeros((len(queries), len(its)), dtype=bool)
    for q, (_, res) in enumerate(queries):
        ok = nonneg & avail
        for k, need in res.items():
            ok = ok & (a[:, abi.RES_INDEX[k]] >= int(need))
        kept[q] = ok
    return kept, np.broadcast_to(price, kept.shape).copy()


def fits_sweep(its, resources=None, n_multi=200, seed=1):
    """Requirement-free rows at the Fits thresholds of a catalogue. For every resource some type has (or those named),
    and every distinct allocatable value v: requests v - 1, v, v + 1 (positive ones), and 1, max + 1, 1 << 62; then
    n_multi rows requesting two to five resources at once, each at or next to the allocatable of one random type."""
    a, _ = alloc_matrix(its)
    rows = []
    for r in range(abi.NUM_RES):
        vals = np.unique(a[:, r])
        if resources is not None and abi.RES_NAMES[r] not in resources:
            continue
        if not (vals != 0).any():
            continue  # no type has the resource: the threshold table is the single value 0
        cand = {1, int(vals.max()) + 1, 1 << 62}
        for v in vals.tolist():
            cand |= {v - 1, v, v + 1}
        rows += [([], {abi.RES_NAMES[r]: c}) for c in sorted(cand) if c > 0]
    rng = np.random.default_rng(seed)
    for _ in range(n_multi):
        t = int(rng.integers(len(its)))
        have = np.nonzero(a[t] > 1)[0]
        pick = rng.choice(have, size=min(len(have), int(rng.integers(2, 6))), replace=False)
        rows.append(([], {abi.RES_NAMES[int(r)]: int(a[t, r]) + int(rng.integers(-1, 2)) for r in sorted(pick)}))
    return rows


def distinct_count(its, resource):
    return len(np.unique(alloc_matrix(its)[0][:, abi.RES_INDEX[resource]]))


def rows_with_distinct(rows, its, resource, n):
    """The table rows (its[i] built from rows[i]) whose allocatable `resource` is one of n values spread over the
    catalogue's distinct ones: every type with one of those values, so values repeat as they do in the table."""
    a = alloc_matrix(its)[0][:, abi.RES_INDEX[resource]]
    vals = np.unique(a)
    assert n <= len(vals), f"{resource}: {len(vals)} distinct allocatable values, {n} wanted"
    pick = vals[np.unique(np.linspace(0, len(vals) - 1, n).round().astype(int))]
    assert len(pick) == n
    return [r for r, keep in zip(rows, np.isin(a, pick)) if keep]


@functools.lru_cache(maxsize=None)
def _table():
    return cmod.load_ec2_table()


N_MEMORY_CLONES = 120


@functools.lru_cache(maxsize=None)
def _memory_pool(lib):
    """The table's rows plus N_MEMORY_CLONES clones with memory sizes the table does not have: the table alone has 168
    distinct memory allocatables (and fewer of every other resource), short of the 256 / 257 the second level of the
    16-ary lower bound needs."""
    rows = list(_table())
    for j in range(N_MEMORY_CLONES):
        src = rows[(j * 7) % len(_table())]
        r = dict(src)
        r["name"] = f"{src['name']}-mem{j}"
        r["memory_mib"] = src["memory_mib"] + 3 * (j + 1)
        rows.append(r)
    return rows, cmod.build_catalog(lib, rows=rows)


@functools.lru_cache(maxsize=None)
def distinct_memory_catalog(lib, n):
    """A catalogue with exactly n distinct memory allocatables, through build_catalog over the chosen rows."""
    rows, its = _memory_pool(lib)
    sub = cmod.build_catalog(lib, rows=rows_with_distinct(rows, its, "memory", n))
    assert distinct_count(sub, "memory") == n
    return sub


FITS_CASES = ["full-memory", "full-other"] + [f"memory-{n}" for n in DISTINCT_COUNTS]


@functools.lru_cache(maxsize=None)
def fits_case(lib, name):
    """(catalogue, rows, oracle kept, oracle cheapest) of one Fits sweep, computed once per session and shared: the
    full catalogue's memory thresholds, its other resources' thresholds, and the memory thresholds of the sub-catalogues
    with a chosen number of distinct memory allocatables."""
    from oracle import pyoracle
    if name.startswith("full"):
        its = cmod.build_catalog(lib)
        mem = name == "full-memory"
        rows = fits_sweep(its, resources=[r for r in abi.RES_NAMES if (r == "memory") == mem], n_multi=150)
    else:
        its = distinct_memory_catalog(lib, int(name.split("-")[1]))
        rows = fits_sweep(its, resources=["memory"], n_multi=150)
    kept, cheapest = pyoracle.compatible_available_filter_many(its, rows)
    for a in (kept, cheapest):
        a.setflags(write=False)
    return its, rows, kept, cheapest


def sized_catalog(lib, n, **kw):
    """A catalogue of n types (kw: build_catalog's, such as zones). Up to the table's size: table rows spread evenly
    over the table. Past it: the whole table and clones of spread rows under a new name with a perturbed on-demand
    price; a clone keeps its source's other requirements (family, size, ...), so only the instance-type key grows."""
    rows = _table()
    if n <= len(rows):
        idx = np.unique(np.linspace(0, len(rows) - 1, n).round().astype(int))
        if n == 1:  # the type with the most memory: some rows keep it
            idx = [int(np.argmax([r["memory_mib"] for r in rows]))]
        assert len(idx) == n
        return cmod.build_catalog(lib, rows=[rows[i] for i in idx], **kw)
    extra = n - len(rows)
    src = np.linspace(0, len(rows) - 1, extra).round().astype(int).tolist()
    clones = []
    for j, i in enumerate(src):
        r = dict(rows[i])
        r["name"] = f"{rows[i]['name']}-clone{j}"
        if r["od_price"] >= 0:
            r["od_price"] = r["od_price"] * (1.0 + 0.001 * (j + 1))
        clones.append(r)
    its = cmod.build_catalog(lib, rows=rows + clones, **kw)
    for j, i in enumerate(src):
        c = its[len(rows) + j]
        c.requirements = [(IT, "In", [c.name]) if r[0] == IT else copy.deepcopy(r) for r in its[i].requirements]
    return its


def with_team_labels(its):
    """A copy in which about a third of the types carry the non-well-known label example.com/team In {a} or {b}."""
    out = copy.deepcopy(its)
    for t, it in enumerate(out):
        if t % 3 == 1:
            it.requirements.append((TEAM, "In", ["a" if t % 2 else "b"]))
    return out


def all_unavailable(its):
    out = copy.deepcopy(its)
    for it in out:
        for o in it.offerings:
            o.available = False
    return out


def dict_words(its, queries):
    """The word count W of the filter plan's label dictionary for (catalogue, rows): one word per key plus one more
    for every further 64 values of a key (the device supports W <= 64)."""
    vals = {}
    for k in (K + "capacity-reservation-id", K + "capacity-reservation-type"):
        vals.setdefault(k, set())
    for it in its:
        for r in it.requirements:
            s = vals.setdefault(r[0], set())
            if r[1] in ("In", "NotIn"):
                s.update(r[2])
        for o in it.offerings:
            vals.setdefault("karpenter.sh/capacity-type", set()).add(o.capacity_type)
            vals.setdefault("topology.kubernetes.io/zone", set()).add(o.zone)
            if o.zone_id:
                vals.setdefault("topology.k8s.aws/zone-id", set()).add(o.zone_id)
            if o.reservation_id:
                vals[K + "capacity-reservation-id"].add(o.reservation_id)
            if o.reservation_type:
                vals[K + "capacity-reservation-type"].add(o.reservation_type)
    for reqs, _ in queries:
        for r in reqs:
            s = vals.setdefault(r[0], set())
            if r[1] in ("In", "NotIn"):
                s.update(r[2])
    return len(vals) + sum(max(1, (len(s) + 63) // 64) - 1 for s in vals.values())


def requirement_edge_queries(its):
    """Rows at the requirement edges of a catalogue (with or without the example.com/team label): the custom key
    omitted / In / NotIn / Exists / DoesNotExist; the arch tie of the complement walk; instance-type In / NotIn with 1,
    half and all-but-one of its values (a multi-word key past 64 types); instance-cpu Gt / Lt around its minimum and
    maximum and an empty range; Exists / DoesNotExist on a key only some types define."""
    names = [it.name for it in its]
    cpus = sorted({int(r[2][0]) for it in its for r in it.requirements if r[0] == K + "instance-cpu"})
    lo, hi = cpus[0], cpus[-1]
    small = {"cpu": 100, "memory": 128 * (1 << 20) * 1000}
    q = [[], [(TEAM, "In", ["a"])], [(TEAM, "In", ["b"])], [(TEAM, "In", ["a", "b"])], [(TEAM, "In", ["c"])],
         [(TEAM, "NotIn", ["a"])], [(TEAM, "NotIn", ["a", "b"])], [(TEAM, "Exists", [])], [(TEAM, "DoesNotExist", [])],
         [(ARCH, "In", ["amd64"])], [(ARCH, "In", ["arm64"])], [(ARCH, "NotIn", ["amd64"])],
         [(ARCH, "In", ["amd64", "arm64"])], [(TEAM, "Exists", []), (ARCH, "In", ["amd64"])]]
    half, rest = names[::2], names[1:]
    for sel in ([names[0]], [names[-1]], half, rest):
        if not sel:
            continue
        q.append([(IT, "In", list(sel))])
        q.append([(IT, "NotIn", list(sel))])
    for b in (lo - 1, lo, hi, hi + 1):
        if b >= 0:
            q.append([(K + "instance-cpu", "Gt", [str(b)])])
            q.append([(K + "instance-cpu", "Lt", [str(b)])])
    q.append([(K + "instance-cpu", "Gt", [str(lo)]), (K + "instance-cpu", "Lt", [str(lo + 1)])])  # empty range
    q.append([(K + "instance-cpu", "Gt", [str(hi)]), (K + "instance-cpu", "Lt", [str(lo)])])
    q.append([(K + "instance-cpu", "Gt", [str(lo)]), (K + "instance-cpu", "Lt", [str(hi)])])
    q.append([(K + "instance-gpu-manufacturer", "DoesNotExist", [])])
    q.append([(K + "instance-gpu-manufacturer", "Exists", [])])
    q.append([(K + "instance-gpu-manufacturer", "Exists", []), (TEAM, "NotIn", ["b"])])
    return [(reqs, dict(small)) for reqs in q]
