"""Plain-Python reference of kp_scheduler_inputs (the rule: include/kp/kp_abi.h) over the model objects -
TEST INFRASTRUCTURE. Requirement algebra through the oracle (pyoracle.requirements_compatible), a ten-line tolerates,
dict arithmetic."""
from oracle import pyoracle

POOL = "karpenter.sh/nodepool"
PNS = "PreferNoSchedule"


def tolerates(tolerations, taint):
    """Some toleration (key, op, value, effect) tolerates the taint (key, value, effect): Toleration.ToleratesTaint"""
    key, value, effect = taint
    for tk, op, tv, te in tolerations:
        if te and te != effect:
            continue
        if tk and tk != key:
            continue
        if op == "Exists" or (op in ("Equal", "") and (tv or "") == (value or "")):
            return True
    return False


def strict(d, i=0):
    """the node selector + the i-th required term + the volume requirements (NewStrictPodRequirements: i = 0)"""
    reqs = [(k, "In", [v]) for k, v in d.node_selector.items()]
    if i < len(d.required_terms):
        reqs += list(d.required_terms[i])
    return reqs + list(d.volume_requirements)


def node_compatible(d, labels, taints):
    return all(tolerates(d.tolerations, t) for t in taints) and \
        pyoracle.requirements_compatible([(k, "In", [v]) for k, v in labels.items()], strict(d), allow_wellknown=False)


def template_requirements(np_):
    return list(np_.requirements) + [(k, "In", [v]) for k, v in np_.labels.items()] + [(POOL, "In", [np_.name])]


def template_compatible(d, np_):
    """upstream isDaemonPodCompatible: PreferNoSchedule tolerated, the first required term dropped on each failure"""
    if not all(tolerates(list(d.tolerations) + [("", "Exists", "", PNS)], t) for t in np_.taints):
        return False
    tmpl = template_requirements(np_)
    return any(pyoracle.requirements_compatible(tmpl, strict(d, i), allow_wellknown=True)
               for i in range(max(1, len(d.required_terms))))


def _sum(lists):
    out = {}
    for l in lists:
        for k, v in l.items():
            out[k] = out.get(k, 0) + v
    return out


def words(bits):
    """[bool per template] -> the uint64 words, template d at bit d % 64 of word d // 64 (at least one word)"""
    out = [0] * max(1, (len(bits) + 63) // 64)
    for d, b in enumerate(bits):
        if b:
            out[d // 64] |= 1 << (d % 64)
    return out


def compute(state):
    """-> dict of the tables Context.scheduler_inputs returns (kpamd.SchedulerInputs attribute names)"""
    ds = state.daemonsets
    out = {"available": [], "requests": [], "node_compatible": [], "compat": [], "matrix": [],
           "daemon_requests": [], "remaining": [], "pool_compatible": [], "pool_matrix": [], "clamped": []}
    cache = {}
    for n in state.nodes:
        key = (tuple(sorted(n.labels.items())), tuple(n.taints))
        bits = cache.get(key)
        if bits is None:
            bits = cache[key] = [node_compatible(d, n.labels, n.taints) for d in ds]
        bound = _sum(r for r, _ in n.pods)
        daemon = _sum(r for r, is_daemon in n.pods if is_daemon)
        expect = _sum(d.requests for d, b in zip(ds, bits) if b)
        out["available"].append({k: v - bound.get(k, 0) for k, v in n.allocatable.items()})
        out["requests"].append({k: max(0, v - daemon.get(k, 0)) for k, v in expect.items()})
        out["clamped"].append(any(v < daemon.get(k, 0) for k, v in expect.items()))
        out["node_compatible"].append(sum(bits))
        out["compat"].append(words(bits))
        out["matrix"].append(bits)
    names = {}
    for p, np_ in enumerate(state.nodepools):
        names.setdefault(np_.name, p)
    used = [{} for _ in state.nodepools]
    for n in state.nodes:
        p = names.get(n.labels.get(POOL))
        if p is not None:
            used[p] = _sum([used[p], n.capacity])
    for p, np_ in enumerate(state.nodepools):
        bits = [template_compatible(d, np_) for d in ds]
        out["daemon_requests"].append(_sum(d.requests for d, b in zip(ds, bits) if b))
        out["pool_compatible"].append(sum(bits))
        out["pool_matrix"].append(bits)
        out["remaining"].append({k: v - used[p].get(k, 0) for k, v in np_.limits.items()} if np_.limits else None)
    return out


def apply(state, target):
    """what kpamd.SchedulerInputs.apply writes, from the reference"""
    ref = compute(state)
    nodes = target.existing if hasattr(target, "existing") else [n.node for n in target.nodes]
    for np_, dr, rem in zip(target.nodepools, ref["daemon_requests"], ref["remaining"]):
        np_.daemon_requests = dict(dr)
        np_.limits = dict(rem) if rem is not None else {}
    for n, av, rq in zip(nodes, ref["available"], ref["requests"]):
        n.available = dict(av)
        n.requests = dict(rq)
    return target


TABLES = ("available", "requests", "node_compatible", "daemon_requests", "remaining", "pool_compatible")


def assert_equal(got, want, name=""):
    """a kpamd.SchedulerInputs against compute()'s dict: == on every table, the present masks (the dicts' keys) and the
    compatibility words included"""
    for t in TABLES:
        g, w = getattr(got, t), want[t]
        assert len(g) == len(w), (name, t, len(g), len(w))
        for i, (x, y) in enumerate(zip(g, w)):
            assert x == y, (name, t, i, x, y)
    assert [[int(x) for x in row] for row in got.compat] == want["compat"], (name, "compat")
