"""The expected kp_validation record (kp_cluster_validate), composed from what the oracle already gives - TEST
INFRASTRUCTURE.

  simulation   command_ref.simulate(cluster, subset): the oracle Solve of SimulateScheduling's Problem (whole: it does
               not stop at a second NodeClaim; Truncate(100) and its minValues check applied - a NodeClaim whose
               truncated options break minValues is listed without options and its pods are unplaced)
  rule         restated here from include/kp/kp_abi.h (upstream disruption/validation.go is not among the references):
                 more than one NodeClaim            MULTIPLE, n_nodeclaims 2, n_unscheduled 0 (the library's simulation
                                                    stops there: the pods it had not reached are in no state)
                 a non-pending pod unscheduled, or a candidate pod on an uninitialized node      UNSCHEDULED
                 no NodeClaim                       VALID without a replacement, else NO_REPLACEMENT_NEEDED
                 one NodeClaim, no replacement      NEEDS_REPLACEMENT
                 one NodeClaim, a replacement       the command's names a subset of the NodeClaim's option names (the
                                                    whole truncated list): VALID, else NOT_SUBSET with n_missing
  budgets      a subset kpamd.disruption.admissible rejects is not simulated: BUDGET, blocked 1

cases() builds the inputs of tests/test_gpu_validate*.py - per named cluster of command_ref.case(): its recorded
commands turned into checks (self-validation), crafted checks for every verdict, and the recorded commands of snapshot
A carried by name onto changed snapshots B - and computed() their expected records; write_golden() records both under
tests/golden/validate_*.json.gz so that GPU time goes to the device, and tests/test_validate_ref.py holds every
recorded file to the recomputation on the CPU."""
import copy
import functools
import gzip
import json
import os

import numpy as np

import command_ref

(VALID, UNSCHEDULED, NO_REPLACEMENT_NEEDED, MULTIPLE, NEEDS_REPLACEMENT, NOT_SUBSET, BUDGET) = range(7)
DELETE, REPLACE = 1, 2
NO_SUCH = "no-such.type"  # a name no catalogue holds
BLOCKED = {"verdict": BUDGET, "n_nodeclaims": 0, "n_pods": 0, "n_unscheduled": 0, "n_missing": 0, "blocked": 1}


def nodeclaim_names(cluster, nc):
    """The option names of a Solve's NodeClaim (its truncated, price-ordered list), in order."""
    cat = cluster.catalogs[cluster.nodepools[nc["nodepool"]].catalog]
    return [cat[int(t)].name for t in nc["options"]]


def record(cluster, check, verdict, solve):
    """The kp_validation dict of one check from its subset's oracle simulation (command_ref.simulate's pair)."""
    ncs = solve["nodeclaims"]
    rec = {"verdict": VALID, "n_nodeclaims": min(len(ncs), 2), "n_pods": int(verdict["n_pods"]), "n_unscheduled": 0,
           "n_missing": 0, "blocked": 0}
    repl = check["decision"] == REPLACE
    if len(ncs) > 1:
        rec["verdict"] = MULTIPLE
    elif verdict["n_unscheduled"]:
        rec.update(verdict=UNSCHEDULED, n_unscheduled=int(verdict["n_unscheduled"]))
    elif not ncs:
        rec["verdict"] = NO_REPLACEMENT_NEEDED if repl else VALID
    elif not repl:
        rec["verdict"] = NEEDS_REPLACEMENT
    else:
        have = set(nodeclaim_names(cluster, ncs[0]))
        missing = len(set(check["options"]) - have)
        if missing:
            rec.update(verdict=NOT_SUBSET, n_missing=missing)
    return rec


def reference(cluster, subsets, checks, allowed=None, solves=None):
    """What ClusterPlan.validate(subsets, checks, allowed) must return (without stats). solves: a dict that keeps each
    subset's oracle simulation."""
    from kpamd import disruption
    adm = [True] * len(subsets)
    if allowed is not None:
        offs = np.zeros(len(subsets) + 1, dtype=np.uint32)
        offs[1:] = np.cumsum([len(s) for s in subsets])
        flat = np.concatenate([np.asarray(s, dtype=np.uint32) for s in subsets] + [np.zeros(0, dtype=np.uint32)])
        adm = list(disruption.admissible(cluster, offs, flat, allowed))
    out = []
    for s, c, ok in zip(subsets, checks, adm):
        if not ok:
            out.append(dict(BLOCKED))
            continue
        out.append(record(cluster, c, *_simulate(cluster, s, solves)))
    return out


def _simulate(cluster, subset, solves):
    key = tuple(int(c) for c in subset)
    if solves is None:
        return command_ref.simulate(cluster, subset)
    if key not in solves:
        solves[key] = command_ref.simulate(cluster, subset)
    return solves[key]


class OracleValidatePlan(command_ref.OracleCommandPlan):
    """The oracle behind ClusterPlan's simulate(), command() and validate()."""

    def validate(self, subsets, checks, allowed=None, cancel=None):
        self.calls.append("validate")
        return reference(self.cluster, subsets, checks, allowed), {}


# ---- checks ----------------------------------------------------------------------------------------------------------
def check_of(cluster, cmd):
    """The check a command of `cluster` (command_ref's dict form) asks for."""
    if not cmd["nodeclaims"]:
        return {"decision": DELETE}
    return {"decision": REPLACE, "options": nodeclaim_names(cluster, cmd["nodeclaims"][0])}


def self_checks(cluster, subsets, name):
    """[(subset, check)] of the case's recorded commands, both multi_node values (their kept options differ)."""
    out, seen = [], set()
    for mn in command_ref.case(name)[2]:
        _, cmds, _ = command_ref.expected(name, mn)
        for s, c in zip(subsets, cmds):
            if c is None:
                continue
            chk = check_of(cluster, c)
            key = (tuple(s), chk["decision"], tuple(chk.get("options", ())))
            if key not in seen:
                seen.add(key)
                out.append((list(s), chk))
    return out


def crafted_checks(cluster, subsets, solves, per_class=4, scan=100):
    """[(subset, check, label)] reaching every verdict on the cluster's own simulations: per class of simulation (no
    NodeClaim, one, several, infeasible) the first per_class of the first `scan` subsets, each with the checks
    kp_abi.h's rule separates."""
    out = []
    count = {"none": 0, "one": 0, "multi": 0, "infeasible": 0, "infeasible-one": 0}
    for s in subsets[:scan]:
        if min(count.values()) >= per_class:
            break
        verdict, solve = _simulate(cluster, s, solves)
        ncs = solve["nodeclaims"]
        cls = ("multi" if len(ncs) > 1 else ("infeasible-one" if ncs else "infeasible") if verdict["n_unscheduled"]
               else "one" if ncs else "none")
        if count[cls] >= per_class:
            continue
        count[cls] += 1
        s = list(s)
        if cls == "one":
            cat = cluster.catalogs[cluster.nodepools[ncs[0]["nodepool"]].catalog]
            names = nodeclaim_names(cluster, ncs[0])
            have = set(names)
            # a type outside the truncated list: the last of the catalogue (index >= 64 in any real catalogue)
            outside = next(cat[t].name for t in range(len(cat) - 1, -1, -1) if cat[t].name not in have)
            out += [(s, {"decision": DELETE}, "delete-claimed"),
                    (s, {"decision": REPLACE, "options": names}, "whole-truncated-list"),
                    (s, {"decision": REPLACE, "options": names + [outside]}, "one-outside"),
                    (s, {"decision": REPLACE, "options": names[:1] + [NO_SUCH]}, "unknown-name"),
                    (s, {"decision": REPLACE, "options": names[:3] + names[:3] + [outside, outside]}, "duplicates"),
                    (s, {"decision": REPLACE, "options": names[-1:]}, "last-of-the-list")]
        else:
            some = cluster.catalogs[0][0].name
            out += [(s, {"decision": DELETE}, f"{cls}-delete"),
                    (s, {"decision": REPLACE, "options": [some]}, f"{cls}-replace")]
    return out


# ---- changed snapshots -----------------------------------------------------------------------------------------------
def _drop_pods(cluster, frac, seed):
    """About frac of every node's pods gone (their requests leave the node)."""
    cl = copy.deepcopy(cluster)
    rng = np.random.default_rng(seed)
    for n in cl.nodes:
        keep = []
        for p in n.pods:
            if rng.random() < frac:
                for k, v in cl.shapes[int(cl.pod_shape[p])].requests.items():
                    n.node.requests[k] = n.node.requests.get(k, 0) - v
            else:
                keep.append(p)
        n.pods = keep
    cl.name = f"{cluster.name}-pods-removed"
    return cl


def _add_pending(cluster, n, seed):
    """n pending pods of the cluster's own shapes (a scale-up between compute and apply)."""
    cl = copy.deepcopy(cluster)
    rng = np.random.default_rng(seed)
    n0 = len(cl.pod_shape)
    cl.pod_shape = np.concatenate([cl.pod_shape, rng.integers(0, len(cl.shapes), size=n).astype(cl.pod_shape.dtype)])
    cl.pod_creation = np.concatenate([cl.pod_creation, (1_750_000_000 + rng.integers(0, 600, size=n)).astype(np.int64)])
    cl.pod_uid = np.concatenate([cl.pod_uid, rng.integers(0, np.iinfo(np.int64).max, size=n, dtype=np.int64).astype(np.uint64)])
    cl.pending = list(cl.pending) + list(range(n0, n0 + n))
    cl.name = f"{cluster.name}-pending-added"
    return cl


def _remove_node(cluster, index):
    """One node gone (with its pods): every later node's index shifts."""
    cl = copy.deepcopy(cluster)
    del cl.nodes[index]
    cl.candidates = [c - (c > index) for c in cl.candidates if c != index]
    cl.name = f"{cluster.name}-node-removed"
    return cl


def ice_marks(cluster, pairs, n_marks=6):
    """[(type index, capacity type, zone)] ICE marks: every offering of the cheapest option of the first n_marks
    REPLACE checks among pairs (catalogue 0)."""
    by_name = {it.name: t for t, it in enumerate(cluster.catalogs[0])}
    marks, seen = [], set()
    for _, chk in pairs:
        if chk["decision"] != REPLACE or chk["options"][0] in seen:
            continue
        seen.add(chk["options"][0])
        t = by_name[chk["options"][0]]
        marks += [(t, o.capacity_type, o.zone) for o in cluster.catalogs[0][t].offerings if o.available]
        if len(seen) >= n_marks:
            break
    return marks


def _iced(cluster, marks):
    cl = copy.deepcopy(cluster)
    gone = set(marks)
    for t, it in enumerate(cl.catalogs[0]):
        for o in it.offerings:
            if (t, o.capacity_type, o.zone) in gone:
                o.available = False
    cl.name = f"{cluster.name}-iced"
    return cl


def carry(old, new, pairs):
    """The (subset, check) pairs of `old` on `new`, candidates mapped by node name; a pair with a candidate that is
    gone is dropped (kpamd.disruption.Validation.validate_candidates fails it before any device call)."""
    index = {n.node.name: i for i, n in enumerate(new.nodes)}
    out = []
    for s, chk in pairs:
        m = [index.get(old.nodes[c].node.name) for c in s]
        if all(i is not None for i in m):
            out.append((m, chk))
    return out


CHANGED = ("pods-removed", "pending-added", "node-removed", "iced")
N_CARRIED = 48  # recorded commands of A carried onto each changed snapshot


@functools.lru_cache(maxsize=None)
def changed(kind):
    """(cluster B, [(subset on B, check)]) for a change of config4's snapshot A."""
    a, subs, _, _ = command_ref.case("config4")
    pairs = self_checks(a, subs, "config4")
    step = max(1, len(pairs) // N_CARRIED)
    pairs = pairs[::step][:N_CARRIED]
    if kind == "pods-removed":
        b = _drop_pods(a, 0.3, 11)
    elif kind == "pending-added":
        b = _add_pending(a, 3, 12)
    elif kind == "node-removed":
        used = {c for s, _ in pairs for c in s}
        b = _remove_node(a, next(i for i in range(len(a.nodes)) if i not in used and any(c > i for c in used)))
    elif kind == "iced":
        b = _iced(a, ice_marks(a, pairs))
    else:
        raise KeyError(kind)
    return b, carry(a, b, pairs)


# ---- the named inputs and their expected records ---------------------------------------------------------------------
BATCHED = ("config4", "config4-limits", "config4-tight-limits", "disruption-state", "min-values", "min-values-broken", "spot-to-spot", "host-ports", "budgets")
GENERAL = ("spread", "anti-affinity", "reservations", "spread-min-values", "spread-min-values-broken", "two-catalogues")
ALL = BATCHED + tuple(f"config4-{k}" for k in CHANGED) + GENERAL
_SOLVES = {}


@functools.lru_cache(maxsize=None)
def min_values_broken():
    """The min-values cluster with instance-type minValues 101 on its NodePools: a NodeClaim starts with more types
    than that, and Truncate(100) leaves too few, so its pods fail (UNSCHEDULED)."""
    from kpamd.model import NodePool
    cl, subs, _, _ = command_ref.case("min-values")
    cl = copy.deepcopy(cl)
    cl.nodepools = [NodePool(p.name, p.weight, p.catalog, list(p.requirements) + [("node.kubernetes.io/instance-type", "Exists", [], 101)])
                    for p in cl.nodepools]
    return cl, subs, None


def _with_min_values(name, req):
    """A named cluster of command_ref with one more requirement (carrying minValues) on every NodePool."""
    from kpamd.model import NodePool
    cl, subs, _, _ = command_ref.case(name)
    cl = copy.deepcopy(cl)
    cl.nodepools = [NodePool(p.name, p.weight, p.catalog, list(p.requirements) + [req], p.labels, p.taints, p.limits,
                             p.daemon_requests, p.budgets) for p in cl.nodepools]
    return cl, subs, None


@functools.lru_cache(maxsize=None)
def own(name):
    """(cluster, subsets, allowed) of the inputs that are no case of command_ref (no recorded commands)."""
    if name == "min-values-broken":
        return min_values_broken()
    if name in ("config4-limits", "config4-tight-limits"):
        # config4's nodes and subsets under remaining NodePool cpu limits: a pod that fits no existing node and no
        # type the limits still admit stays unplaced, with no NodeClaim or next to the one the limits allowed
        cl, subs, _, _ = command_ref.case("config4")
        cl = copy.deepcopy(cl)
        # (tight: no type is left for most pods under the limits the pass begins with, so they fail without any
        # NodeClaim being tried - the batched kernel's own unplaced-pod path, not the settle after a second NodeClaim)
        for p, lim in zip(cl.nodepools, (4000, 1000) if name == "config4-limits" else (1000, 1000)):
            p.limits = {"cpu": lim}
        singles = [[c] for c in cl.candidates[:12] + cl.candidates[-28:]]  # full nodes alone: more than the limits admit
        return cl, singles + list(subs), None
    if name == "spread-min-values":  # the general path's minValues check on the device, holding ...
        return _with_min_values("spread", (command_ref.K + "instance-family", "Exists", [], 5))
    if name == "spread-min-values-broken":  # ... and broken by Truncate(100)
        return _with_min_values("spread", ("node.kubernetes.io/instance-type", "Exists", [], 101))
    if name == "two-catalogues":
        # the spread cluster with a second catalogue - the same types in reverse order - read by every NodePool: a
        # new NodeClaim lands on catalogue 1, while the nodes and the commands' names come from catalogue 0
        cl, subs, _, _ = command_ref.case("spread")
        cl = copy.deepcopy(cl)
        cl.catalogs = [cl.catalogs[0], list(reversed(cl.catalogs[0]))]
        for p in cl.nodepools:
            p.catalog = 1
        return cl, subs, None
    raise KeyError(name)


OWN = ("config4-limits", "config4-tight-limits", "min-values-broken", "spread-min-values", "spread-min-values-broken", "two-catalogues")


@functools.lru_cache(maxsize=None)
def cases(name):
    """(cluster, subsets, checks, labels, allowed) of a named input. Every subset appears once per check."""
    if name.startswith("config4-") and name not in OWN:
        b, pairs = changed(name[len("config4-"):])
        return b, [s for s, _ in pairs], [c for _, c in pairs], ["carried"] * len(pairs), None
    solves = _SOLVES.setdefault(name, {})
    if name == "two-catalogues":  # the spread cluster's own inputs, on the changed cluster
        cl, _, allowed = own(name)
        _, subs, checks, labels, _ = cases("spread")
        return cl, subs, checks, labels, allowed
    if name in OWN:
        cl, subs, allowed = own(name)
        pairs = []
    else:
        cl, subs, _, allowed = command_ref.case(name)
        pairs = [(s, c, "self") for s, c in self_checks(cl, subs, name)]
    pairs += crafted_checks(cl, subs, solves, per_class=6 if name == "config4" else 3, scan=240 if name in ("config4-limits", "config4-tight-limits") else 100)
    if name == "anti-affinity":  # every subset once more: the ones compiled on their own are among them
        pairs += [(list(s), {"decision": DELETE}, "every-subset") for s in subs]
    return cl, [p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs], allowed


def cluster_of(name):
    """(cluster, allowed) of a named input without touching the oracle (the GPU tests read the rest from golden/)."""
    if name.startswith("config4-") and name not in OWN:
        return changed(name[len("config4-"):])[0], None
    if name in OWN:
        return own(name)[0], None
    cl, _, _, allowed = command_ref.case(name)
    return cl, allowed


def iced_marks():
    """The ICE marks of the "iced" snapshot, for kp_catalog_update_offerings on snapshot A's own catalogue."""
    a, subs, _, _ = command_ref.case("config4")
    pairs = self_checks(a, subs, "config4")
    return ice_marks(a, pairs[::max(1, len(pairs) // N_CARRIED)][:N_CARRIED])


@functools.lru_cache(maxsize=None)
def computed(name):
    cl, subs, checks, _, allowed = cases(name)
    return reference(cl, subs, checks, allowed, solves=_SOLVES.setdefault(name, {}))


GOLDEN = command_ref.GOLDEN


def _golden_path(name):
    return os.path.join(GOLDEN, f"validate_{name}.json.gz")


def _doc(name):
    _, subs, checks, labels, _ = cases(name)
    return {"subsets": [[int(c) for c in s] for s in subs], "checks": checks, "labels": labels, "records": computed(name)}


def write_golden(name):
    os.makedirs(GOLDEN, exist_ok=True)
    with gzip.GzipFile(_golden_path(name), "wb", mtime=0) as f:
        f.write(json.dumps(_doc(name), sort_keys=True).encode())


@functools.lru_cache(maxsize=None)
def expected(name):
    """The recorded document of a named input: subsets, checks, labels, records."""
    with gzip.open(_golden_path(name), "rb") as f:
        return json.loads(f.read().decode())


if __name__ == "__main__":
    import sys
    for nm in sys.argv[1:] or ALL:
        write_golden(nm)
        print(nm, len(expected.__wrapped__(nm)["records"]), os.path.getsize(_golden_path(nm)))
