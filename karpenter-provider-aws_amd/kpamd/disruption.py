"""Disruption-side callers of the batched simulation (kp_cluster_simulate), mirroring upstream
pkg/controllers/disruption (sigs.k8s.io/karpenter v1.5.1, absent from the container; behaviour per SURVEY §3
CS3 and R:website/content/en/preview/concepts/disruption.md:89-128):

  SingleNodeConsolidation.compute_command   the first candidate (disruption-cost order) whose
                                            computeConsolidation is not a no-op
  MultiNodeConsolidation.first_n_option     firstNConsolidationOption's binary search over prefixes
                                            candidates[0:mid+1], lo=1, hi = len-1 if len <= 100 else 100
                                            (ComputeCommand passes max = Clamp(len, 0, MaxParallel=100) and
                                            firstN lowers it to len-1 only when len <= max); every prefix
                                            the search can touch is simulated in ONE batch, then the
                                            search is replayed exactly over those results
  sweep(...)                                the config-4 sweep: this rank's contiguous share of the subsets
                                            through kp_consolidate_argmin (simulation, device argmax, one
                                            RCCL all-gather of the ranks' records inside libkp)
  local_choice(...)                         a rank's kp_choice record from per-subset results on the host
                                            (what the device argmax produces; CPU tests and other transports)
  Emptiness.compute_command                 the candidates without reschedulable pods, deleted in one command
  candidate_order(cluster)                  the consolidatable nodes in disruption-cost order (ReschedulingCost of
                                            default-priority pods = their count; ties by node name)
  Drift.compute_command(cluster, plan)      the drifted nodes (ClusterNode.drifted, oldest first): the empty ones
                                            deleted in one command, else the first whose SimulateScheduling
                                            reschedules every non-pending pod, replaced by that Solve's NodeClaims
                                            (R:website/content/en/preview/concepts/disruption.md:131-175; every
                                            candidate is one simulation of ONE plan.drift batch)
  Controller.compute_command(cluster, plan) one disruption pass in upstream order ("first Drift then Consolidation",
                                            disruption.md:16-27; Emptiness, Drift, MultiNodeConsolidation,
                                            SingleNodeConsolidation): the first method that returns a command wins
  candidates(cluster, plan, method, now)    GetCandidates on the device (kp_cluster_candidates) when the cluster carries
                                            DisruptionControls: per node the reason it is no candidate (do-not-disrupt,
                                            PDBs, consolidateAfter, ...), the costs, and the candidates in disruption
                                            order; Controller.compute_command takes its lists from it then
  detect_drift(cluster, plan, now)          IsDrifted for every node on the device (kp_cluster_detect_drift) when the
                                            cluster carries DriftInputs, and the Drifted condition's life applied to
                                            ClusterNode.drifted; Controller.compute_command calls it first then
  Validation(cluster, plan)                 Validation.IsValid of a computed command against a FRESH snapshot (upstream
  Controller.validate(cmd, old, new, plan)  disruption/validation.go, restated in DESIGN §12): the candidates mapped by
                                            node name (gone, deleting, nominated, the budget walk), then one
                                            plan.validate (kp_cluster_validate) of the command's decision and options.
                                            Nothing validates unless asked; Drift commands are not validated.
  unconsolidatable(cluster, plan, now)      why each managed node stays, for the single-node pass: the candidate reason
  unconsolidatable_message(entry)           where it is no candidate, else the exit of its singleton's simulation
                                            (plan.simulate_explained, kp_cluster_simulate_explained) under the budget
                                            walk; the message renders the Unconsolidatable event's text

NodePool disruption budgets (R:website/content/en/preview/concepts/disruption.md:274-333,
R:pkg/apis/crds/karpenter.sh_nodepools.yaml:95-135), modelled when a NodePool carries `budgets`:

  allowed_disruptions(cluster, reason)      per NodePool: max(0, min over the active budgets that list the reason (or
                                            none) of value(budget, total) - deleting - not_ready); UNLIMITED without one
  budget_active(budget, now)                schedule + duration: the schedule's first fire time strictly after
                                            now - duration is <= now (five-field cron or @macro, UTC)
  budget_walk(cluster, candidates, allowed) upstream's construction for every method: the candidates in disruption-cost
                                            order, one allowance taken from its pool per candidate kept
  admissible(cluster, offsets, nodes, allowed)  the sweep's generalisation: a subset is admissible iff no NodePool owns
                                            more of its members than allowed[pool] (what the device gate computes)

Emptiness asks with the reason Empty, single- and multi-node consolidation with Underutilized, Drift with Drifted. NodePool.budgets None is
"not modelled": unlimited, and nothing above runs.

Decisions are kp_decision values: 0 no-op, 1 delete, 2 replace.
"""
import calendar
import datetime
import re

import numpy as np

from . import abi

NOOP, DELETE, REPLACE = 0, 1, 2
UNLIMITED = 2**32 - 1  # KP_BUDGET_UNLIMITED
POOL_LABEL = "karpenter.sh/nodepool"
EMPTY, UNDERUTILIZED, DRIFTED = "Empty", "Underutilized", "Drifted"


class Command:
    """A disruption command: the method that produced it, its candidates (cluster node indices, candidate order), the
    decision (DELETE / REPLACE) and the computeConsolidation result (savings, replacement NodePool and price, ...)."""

    def __init__(self, method, candidates, decision, result=None):
        self.method = method
        self.candidates = list(candidates)
        self.decision = decision
        self.result = result or {}

    def __repr__(self):
        return f"Command({self.method}, {self.candidates}, {('noop', 'delete', 'replace')[self.decision]})"


def candidate_order(cluster, nodes=None):
    """Consolidation candidates in disruption-cost order (R:website/content/en/preview/concepts/disruption.md:101-103:
    the candidates that are cheapest to disrupt first). Every pod here has the default priority and deletion cost, so
    ReschedulingCost is the pod count; nodes marked for deletion are never candidates; ties go by node name (upstream
    sorts a slice built from a map: parity unpinned)."""
    idx = [i for i in (range(len(cluster.nodes)) if nodes is None else nodes) if not cluster.nodes[i].deleting]
    return sorted(idx, key=lambda i: (len(cluster.nodes[i].pods), cluster.nodes[i].node.name))


METHODS = {"emptiness": 0, "single": 1, "multi": 2, "drift": 3}  # enum kp_disruption_method


def candidates(cluster, plan, method, now):
    """GetCandidates for one method ("emptiness" / "single" / "multi" / "drift", or its kp_disruption_method value) at
    unix time `now`, from cluster.controls (DisruptionControls): (records, order). records[i] is node i's
    kp_candidate (reason 0: a candidate, else why not, with the reason's detail; ReschedulingCost in units of 2^-27;
    DisruptionCost); order lists the candidates by DisruptionCost (Drift: by the Drifted transition time), ties by node
    name. plan: the resident snapshot (ClusterPlan, or any object with the same candidates(method, now))."""
    if cluster.controls is None:
        raise ValueError("the cluster carries no DisruptionControls (candidate_order / drift_order apply)")
    res = plan.candidates(METHODS.get(method, method), int(now))
    return res[0], list(res[1])


# ---- NodePool disruption budgets -----------------------------------------------------------------------------------
_NODES_RE = re.compile(r"^((100|[0-9]{1,2})%|[0-9]+)$")  # the CRD's pattern
_MACROS = {"@yearly": "0 0 1 1 *", "@annually": "0 0 1 1 *", "@monthly": "0 0 1 * *", "@weekly": "0 0 * * 0",
           "@daily": "0 0 * * *", "@midnight": "0 0 * * *", "@hourly": "0 * * * *"}
_FIELDS = ((0, 59), (0, 23), (1, 31), (1, 12), (0, 7))  # minute, hour, day of month, month, day of week (7 = Sunday)


def budget_value(nodes, total):
    """value(budget, total): ceil(total * p / 100) for "p%", else the integer."""
    if not isinstance(nodes, str) or not _NODES_RE.match(nodes):
        raise ValueError(f"budget nodes {nodes!r}")
    if nodes.endswith("%"):
        return (total * int(nodes[:-1]) + 99) // 100
    return int(nodes)


def _cron_field(text, lo, hi):
    """One cron field (`*`, lists, ranges, /step) -> (set of values, restricted?). Names are rejected."""
    out = set()
    for part in text.split(","):
        rng, _, step = part.partition("/")
        if ("/" in part and not step.isdigit()) or (step and int(step) < 1):
            raise ValueError(f"cron step in {text!r}")
        st = int(step) if step else 1
        if rng == "*":
            a, b = lo, hi
        elif "-" in rng:
            x, _, y = rng.partition("-")
            if not (x.isdigit() and y.isdigit()):
                raise ValueError(f"cron range {rng!r}")
            a, b = int(x), int(y)
        else:
            if not rng.isdigit():
                raise ValueError(f"cron value {rng!r}")
            a = int(rng)
            b = hi if step else a  # "a/step": from a to the field's end
        if a < lo or b > hi or a > b:
            raise ValueError(f"cron field {text!r} outside {lo}-{hi}")
        out.update(range(a, b + 1, st))
    star = text == "*" or text.startswith("*/")
    return out, not star


def parse_schedule(schedule):
    """Five-field cron or @macro -> (minutes, hours, days of month, months, days of week (0-6), dom restricted, dow
    restricted). ValueError on anything else (month and day names included)."""
    if not isinstance(schedule, str):
        raise ValueError(f"schedule {schedule!r}")
    text = schedule.strip()
    if text.startswith("@"):
        if text not in _MACROS:
            raise ValueError(f"schedule macro {schedule!r}")
        text = _MACROS[text]
    parts = text.split()
    if len(parts) != 5:
        raise ValueError(f"schedule {schedule!r}: five fields expected")
    sets, restricted = [], []
    for p, (lo, hi) in zip(parts, _FIELDS):
        s, r = _cron_field(p, lo, hi)
        sets.append(s)
        restricted.append(r)
    dow = {d % 7 for d in sets[4]}
    return sets[0], sets[1], sets[2], sets[3], dow, restricted[2], restricted[4]


def _ts(now):
    if now is None:
        return datetime.datetime.now(datetime.timezone.utc).timestamp()
    if isinstance(now, datetime.datetime):
        if now.tzinfo is None:
            now = now.replace(tzinfo=datetime.timezone.utc)
        return now.timestamp()
    return now


def schedule_next(schedule, after):
    """The schedule's first fire time (unix seconds, UTC) strictly after `after`; None if none within eight years."""
    mins, hours, doms, months, dows, dom_r, dow_r = parse_schedule(schedule)
    t = (int(after // 60) + 1) * 60
    end = t + 8 * 366 * 86400
    while t < end:
        y, mo, d, h, mi = datetime.datetime.fromtimestamp(t, datetime.timezone.utc).timetuple()[:5]
        if mo not in months:
            t = calendar.timegm((y + (mo == 12), mo % 12 + 1, 1, 0, 0, 0))
            continue
        wd = (calendar.weekday(y, mo, d) + 1) % 7  # 0 = Sunday
        # both day fields restricted: either one matching suffices; otherwise both must match
        day = (d in doms or wd in dows) if (dom_r and dow_r) else (d in doms and wd in dows)
        if not day:
            t = calendar.timegm((y, mo, d, 0, 0, 0)) + 86400
        elif h not in hours:
            t = calendar.timegm((y, mo, d, h, 0, 0)) + 3600
        elif mi not in mins:
            t += 60
        else:
            return t
    return None


def budget_active(budget, now=None):
    """A budget without schedule and duration is always active; with both, iff the schedule's first fire time strictly
    after now - duration is <= now (UTC). One without the other is a ValueError."""
    if (budget.schedule is None) != (budget.duration_s is None):
        raise ValueError("budget schedule and duration must be set together")
    if budget.schedule is None:
        return True
    now = _ts(now)
    nxt = schedule_next(budget.schedule, now - budget.duration_s)
    return nxt is not None and nxt <= now


def _pool_index(cluster):
    return {p.name: i for i, p in enumerate(cluster.nodepools)}


def node_pools(cluster):
    """Per node: the index of the NodePool its karpenter.sh/nodepool label names, -1 if missing or unknown."""
    idx = _pool_index(cluster)
    return np.array([idx.get(n.node.labels.get(POOL_LABEL), -1) for n in cluster.nodes], dtype=np.int64)


def allowed_disruptions(cluster, reason, now=None, not_ready=(), extra_deleting=None):
    """Allowed disruptions per NodePool for `reason` (list, UNLIMITED where no active budget applies). total = the
    pool's nodes, deleting ones included; not_ready: node indices that are NotReady; extra_deleting[pool index or
    name]: nodes still terminating but no longer in the snapshot (they add to total and to deleting)."""
    pools = node_pools(cluster)
    P = len(cluster.nodepools)
    total, busy = [0] * P, [0] * P
    nr = set(not_ready)
    for i, n in enumerate(cluster.nodes):
        p = int(pools[i])
        if p < 0:
            continue
        total[p] += 1
        if n.deleting or i in nr:
            busy[p] += 1
    for k, v in (extra_deleting or {}).items():
        p = k if isinstance(k, int) else _pool_index(cluster)[k]
        total[p] += int(v)
        busy[p] += int(v)
    out = []
    for p, pool in enumerate(cluster.nodepools):
        vals = [budget_value(b.nodes, total[p]) for b in (pool.budgets or [])
                if (b.reasons is None or reason in b.reasons) and budget_active(b, now)]
        out.append(min(UNLIMITED, max(0, min(vals) - busy[p])) if vals else UNLIMITED)
    return out


def budgets_modelled(cluster):
    return any(p.budgets is not None for p in cluster.nodepools)


def budget_walk(cluster, candidates, allowed):
    """Upstream's candidate construction under budgets: the candidates in the given (disruption-cost) order; one whose
    pool has no allowance left is skipped, otherwise it is kept and takes one from its pool."""
    pools = node_pools(cluster)
    left = list(allowed)
    out = []
    for c in candidates:
        p = int(pools[c])
        if p < 0:
            raise ValueError(f"node {c}: no NodePool for its {POOL_LABEL} label")
        if left[p] == 0:
            continue
        if left[p] != UNLIMITED:
            left[p] -= 1
        out.append(c)
    return out


def admissible(cluster, offsets, nodes, allowed):
    """numpy bool per CSR subset: for every NodePool, the subset's members owned by it number <= allowed[pool]."""
    offsets = np.asarray(offsets, dtype=np.int64)
    nodes = np.asarray(nodes, dtype=np.int64)
    n, P = len(offsets) - 1, len(cluster.nodepools)
    if len(allowed) != P:
        raise ValueError(f"allowed has {len(allowed)} entries for {P} NodePools")
    pool = node_pools(cluster)[nodes] if len(nodes) else np.zeros(0, dtype=np.int64)
    if (pool < 0).any():
        raise ValueError(f"node {int(nodes[np.argmax(pool < 0)])}: no NodePool for its {POOL_LABEL} label")
    sub = np.repeat(np.arange(n), np.diff(offsets))
    cnt = np.zeros((n, max(P, 1)), dtype=np.int64)
    np.add.at(cnt, (sub, pool), 1)
    return (cnt[:, :P] <= np.asarray(allowed, dtype=np.int64)[None, :]).all(axis=1)


class Emptiness:
    """Emptiness (WhenEmptyOrUnderutilized with consolidateAfter elapsed): every candidate node without reschedulable
    pods is deleted, all in one command; under budgets, as many as the reason Empty allows per NodePool (the walk)."""

    def compute_command(self, cluster, candidates, now=None, not_ready=(), extra_deleting=None):
        empty = [c for c in candidates if not cluster.nodes[c].pods]
        if empty and budgets_modelled(cluster):
            empty = budget_walk(cluster, empty, allowed_disruptions(cluster, EMPTY, now, not_ready, extra_deleting))
        return Command("emptiness", empty, DELETE, {"decision": DELETE}) if empty else None


def drift_order(cluster):
    """Drift candidates: the nodes carrying a Drifted condition (ClusterNode.drifted, its transition time) and not
    marked for deletion, oldest condition first, ties by node name."""
    idx = [i for i, n in enumerate(cluster.nodes) if getattr(n, "drifted", None) is not None and not n.deleting]
    return sorted(idx, key=lambda i: (cluster.nodes[i].drifted, cluster.nodes[i].node.name))


def detect_drift(cluster, plan, now):
    """Drift detection for every node of the snapshot (cluster.drift_inputs) and the life of the Drifted
    condition (R:website/content/en/preview/concepts/disruption.md:162-164), applied to ClusterNode.drifted and, when
    the cluster has controls, to controls.nodes[i].drifted: a newly drifted node gets `now`, a node still drifted keeps
    its time, a node no longer drifted loses it; a node whose status is an error keeps what it had (upstream returns
    the error and does not touch the condition). plan: the resident snapshot (ClusterPlan, or any object with the same
    detect_drift()). Returns (records, counts)."""
    if cluster.drift_inputs is None:
        raise ValueError("the cluster carries no DriftInputs")
    records, counts = plan.detect_drift()[:2]
    controls = getattr(cluster, "controls", None)
    at = _ts(now)
    for i, node in enumerate(cluster.nodes):
        if int(records[i]["status"]) >= abi.DRIFT_ERR_INSTANCE:
            continue
        if int(records[i]["reason"]) == abi.DRIFT_NONE:
            node.drifted = None
        elif node.drifted is None:
            node.drifted = at
        if controls is not None:
            controls.nodes[i].drifted = None if node.drifted is None else int(node.drifted)
    return records, counts


class Drift:
    """Drift (upstream disruption/drift.go v1.5.1, restated in DESIGN §10). Budgets are asked with the reason Drifted.
    Drifted candidates without reschedulable pods come first: each whose pool still has allowance is kept (one
    allowance each) and, if any are kept, they form one DELETE command with no simulation. Otherwise the candidates are
    tried in order, one whose pool's allowance is 0 skipped; the first whose simulation schedules every non-pending pod
    wins, with every new NodeClaim of that Solve as its replacements (none: a plain delete). All candidates are one
    plan.drift batch of singletons: the device answers which is first."""

    def compute_command(self, cluster, plan, now=None, not_ready=(), extra_deleting=None, cands=None):
        cands = drift_order(cluster) if cands is None else list(cands)
        if not cands:
            return None
        allowed = None
        if budgets_modelled(cluster):
            allowed = allowed_disruptions(cluster, DRIFTED, now, not_ready, extra_deleting)
        empty = [c for c in cands if not cluster.nodes[c].pods]
        if empty and allowed is not None:
            empty = budget_walk(cluster, empty, allowed)
        if empty:
            return Command("drift", empty, DELETE, {"decision": DELETE, "replacements": [], "blocked": []})
        if allowed is not None:  # a candidate whose pool's allowance is 0 is skipped (nothing is consumed before a command)
            pools = node_pools(cluster)
            cands = [c for c in cands if allowed[int(pools[c])] != 0]
        if not cands:
            return None
        r = plan.drift([[c] for c in cands], allowed=allowed)
        if r["first"] < 0:
            return None
        repl = r["replacements"]["nodeclaims"]
        decision = REPLACE if repl else DELETE
        return Command("drift", [cands[r["first"]]], decision,
                       {"decision": decision, "replacements": repl, "placement": r["replacements"]["placement"],
                        "blocked": cands[:r["first"]]})


class Controller:
    """One pass of the disruption controller over its methods, in upstream order: Emptiness, then Drift (only when some
    node carries `drifted`; the plan is not touched otherwise), then
    MultiNodeConsolidation (firstNConsolidationOption over the disruption-cost order), then SingleNodeConsolidation
    (the first candidate whose computeConsolidation is not a no-op). plan: the resident snapshot of `cluster`
    (ClusterPlan, or any object with the same simulate(subsets, multi_node)). When some NodePool has budgets, each
    method's candidates go through the budget walk first (Emptiness: reason Empty, the others: Underutilized); now,
    not_ready and extra_deleting are allowed_disruptions' arguments.

    materialize=True: the multi-node and single-node winners are passed once more through plan.command([winner],
    multi_node) (kp_cluster_command), and their Command.result gains "replacements" (the replacement NodeClaim, its
    options the ones the price filters kept; none for a DELETE) and "placement" (where every rescheduled pod went) -
    Drift's keys. The command call must decide what simulate decided. The default leaves plans without .command
    working as before."""

    def __init__(self, materialize=False):
        self.materialize = materialize

    def _materialized(self, plan, method, candidates, r):
        if not self.materialize:
            return Command(method, candidates, r["decision"], r)
        res, cmds, _ = plan.command([list(candidates)], multi_node=method == "multi")
        if res[0] != r or cmds[0] is None:
            raise RuntimeError(f"command({candidates}) decided {res[0]}, simulate {r}")
        out = dict(r, replacements=cmds[0]["nodeclaims"], placement=cmds[0]["placement"])
        return Command(method, candidates, r["decision"], out)

    def compute_command(self, cluster, plan, now=None, not_ready=(), extra_deleting=None):
        if getattr(cluster, "drift_inputs", None) is not None:  # which nodes are drifted is computed, not given
            detect_drift(cluster, plan, now)
        if getattr(cluster, "controls", None) is not None:
            return self._compute_with_controls(cluster, plan, now, not_ready, extra_deleting)
        cands = candidate_order(cluster)
        cmd = Emptiness().compute_command(cluster, cands, now, not_ready, extra_deleting)
        if cmd is not None:
            return cmd
        cmd = Drift().compute_command(cluster, plan, now, not_ready, extra_deleting)
        if cmd is not None:
            return cmd
        cands = [c for c in cands if cluster.nodes[c].pods]
        return self._consolidate(cluster, plan, cands, cands, now, not_ready, extra_deleting)

    def _compute_with_controls(self, cluster, plan, now, not_ready, extra_deleting):
        """The pass with each method's candidates from candidates() (cluster.controls set): the same methods in the
        same order, every list the device's for that method at `now`."""
        at = int(_ts(now))
        cmd = Emptiness().compute_command(cluster, candidates(cluster, plan, "emptiness", at)[1], now, not_ready,
                                          extra_deleting)
        if cmd is not None:
            return cmd
        cmd = Drift().compute_command(cluster, plan, now, not_ready, extra_deleting,
                                      cands=candidates(cluster, plan, "drift", at)[1])
        if cmd is not None:
            return cmd
        multi = [c for c in candidates(cluster, plan, "multi", at)[1] if cluster.nodes[c].pods]
        single = [c for c in candidates(cluster, plan, "single", at)[1] if cluster.nodes[c].pods]
        return self._consolidate(cluster, plan, multi, single, now, not_ready, extra_deleting)

    def _consolidate(self, cluster, plan, cands, single_cands, now, not_ready, extra_deleting):
        allowed = None
        if budgets_modelled(cluster):
            allowed = allowed_disruptions(cluster, UNDERUTILIZED, now, not_ready, extra_deleting)
        multi = MultiNodeConsolidation(plan, cluster, allowed)
        hit = multi.first_n_option(cands)
        if hit is not None:
            n, r = hit
            return self._materialized(plan, "multi", multi.candidates(cands)[:n], r)
        hit = SingleNodeConsolidation(plan, cluster, allowed).compute_command(single_cands)
        if hit is not None:
            c, r = hit
            return self._materialized(plan, "single", [c], r)
        return None

    def validate(self, cmd, old_cluster, cluster, plan, now=None, not_ready=(), extra_deleting=None):
        """Validation.IsValid of a command computed on old_cluster against the current cluster and its plan: (ok,
        reason). Nothing calls this unless asked; a Drift command is not validated (upstream runs none on it)."""
        if cmd.method == "drift":
            return True, None
        ok, why, _ = Validation(cluster, plan).validate_command(cmd, old_cluster, now, not_ready, extra_deleting)
        return ok, why


VERDICTS = ("valid", "unscheduled", "no-replacement-needed", "multiple", "needs-replacement", "not-subset", "budget")
_REASON = {"emptiness": EMPTY, "drift": DRIFTED, "single": UNDERUTILIZED, "multi": UNDERUTILIZED}


# ---- Unconsolidatable events (kp_cluster_simulate_explained) -------------------------------------------------
# Reason texts. Only the two strings R:website/content/en/preview/concepts/disruption.md:105-113 prints are pinned:
# "pdb <ns>/<name> prevents pod evictions" and "can't replace with a lower-priced node". The rest are restated and
# UNPINNED (disruption/consolidation.go is not among the references).
_UNCONS_TEXT = {
    abi.UNCONS_BUDGET: "disruption budget allows no more disruptions of its NodePool",                       # unpinned
    abi.UNCONS_MULTIPLE_NODECLAIMS: "can't remove without creating {n_nodeclaims} candidates",                # unpinned
    abi.UNCONS_UNSCHEDULABLE: "not all pods would schedule",                                                  # unpinned
    abi.UNCONS_UNPRICED: "can't determine the price of the candidate's instance type",                       # unpinned
    abi.UNCONS_SPOT_TO_SPOT_DISABLED: "SpotToSpotConsolidation is disabled, can't replace a spot node with a spot node",  # unpinned
    abi.UNCONS_NOT_CHEAPER: "can't replace with a lower-priced node",                                         # pinned
    abi.UNCONS_SAME_TYPE: "can't replace with a lower-priced node of another instance type",                  # unpinned
    abi.UNCONS_SPOT_FLEXIBILITY: "SpotToSpotConsolidation requires 15 cheaper instance type options than the current "
                                 "candidate to consolidate, got {n_same_type}",                               # unpinned
    abi.UNCONS_MIN_VALUES: "minValues requirement is not met for the cheaper instance type options",          # unpinned
}
PDB_BLOCKED = abi.REASON_NAMES.index("PDB_BLOCKED")  # enum kp_candidate_reason
_CAND_TEXT = {1: "not managed by a NodePool", 2: "node has the karpenter.sh/do-not-disrupt annotation",
              3: "node is not initialized", 4: "node is deleting", 5: "node is nominated for a pending pod",
              6: "pod has the karpenter.sh/do-not-disrupt annotation", 8: "consolidation is disabled (consolidateAfter Never)",
              9: "NodePool consolidates only when empty", 10: "consolidateAfter has not elapsed", 11: "node is not empty",
              12: "node is not drifted"}  # unpinned, all of them


def unconsolidatable(cluster, plan, now=None, not_ready=(), extra_deleting=None):
    """Why each managed node stays, for the single-node pass: one entry per node that carries a NodePool of the
    cluster, in node order: {"node", "candidate_reason", "detail", "pdb", "why", "sim"}.
      * With cluster.controls: a node that is no SingleNodeConsolidation candidate carries its kp_candidate reason and
        detail ("pdb": (namespace, name) of the blocking PDB for KP_PDB_BLOCKED), and no simulation. Without controls
        only the nodes being deleted are no candidates (candidate_order).
      * Every other node carries "why", the kp_sim_why of its singleton's simulation (plan.simulate_explained, multi_node
        False), and "sim"; under modelled budgets the candidates go through the budget walk first (reason
        Underutilized) and one the walk skips carries the KP_UNCONS_BUDGET record without a simulation.
    plan: the resident snapshot (ClusterPlan, or any object with the same candidates / simulate_explained)."""
    pools = node_pools(cluster)
    entries = {}
    if getattr(cluster, "controls", None) is not None:
        recs, order = candidates(cluster, plan, "single", int(_ts(now)))
        for i in range(len(cluster.nodes)):
            # (a kp_candidate record of the device, or the (reason, detail, ...) tuple a reference plan returns)
            r, d = (int(recs[i]["reason"]), int(recs[i]["detail"])) if hasattr(recs[i], "dtype") else \
                (int(recs[i][0]), int(recs[i][1]))
            if pools[i] >= 0 and r != 0:
                pdb = cluster.controls.pdbs[d] if r == PDB_BLOCKED else None
                entries[i] = {"node": i, "candidate_reason": r, "detail": d, "why": None, "sim": None,
                              "pdb": (pdb.namespace, pdb.name) if pdb is not None else None}
        cands = [c for c in order if pools[c] >= 0]
    else:
        for i, n in enumerate(cluster.nodes):
            if pools[i] >= 0 and n.deleting:
                entries[i] = {"node": i, "candidate_reason": 4, "detail": 0, "why": None, "sim": None, "pdb": None}
        cands = [c for c in candidate_order(cluster) if pools[c] >= 0]
    kept = cands
    if budgets_modelled(cluster):
        kept = budget_walk(cluster, cands, allowed_disruptions(cluster, UNDERUTILIZED, now, not_ready, extra_deleting))
    blocked = dict.fromkeys(abi.WHY_FIELDS, 0)
    blocked.update(reason=abi.UNCONS_BUDGET, first_unscheduled=-1, unpriced=-1, cheapest_launch=0.0)
    for c in set(cands) - set(kept):
        entries[c] = {"node": c, "candidate_reason": 0, "detail": 0, "why": dict(blocked), "sim": None, "pdb": None}
    if kept:
        sims, whys = plan.simulate_explained([[c] for c in kept], multi_node=False)[:2]
        for c, s, w in zip(kept, sims, whys):
            entries[c] = {"node": c, "candidate_reason": 0, "detail": 0, "why": w, "sim": s, "pdb": None}
    return [entries[i] for i in sorted(entries)]


def unconsolidatable_message(entry):
    """The Unconsolidatable event's text for an entry of unconsolidatable(), None for a node that can be consolidated
    (reason KP_UNCONS_NONE). Pinned: "pdb <ns>/<name> prevents pod evictions" and "can't replace with a lower-priced
    node" (disruption.md:105-113); every other text is a restatement and unpinned."""
    r = entry["candidate_reason"]
    if r == PDB_BLOCKED:
        return "pdb {}/{} prevents pod evictions".format(*entry["pdb"])
    if r:
        return _CAND_TEXT[r]
    w = entry["why"]
    if w["reason"] == abi.UNCONS_NONE:
        return None
    return _UNCONS_TEXT[w["reason"]].format(**w)


class Validation:
    """Validation.IsValid of a consolidation command against a fresh snapshot (upstream disruption/validation.go v1.5.1,
    restated in DESIGN §12 and include/kp/kp_abi.h: the file is not among the references). cluster / plan: the CURRENT
    state and its resident snapshot (ClusterPlan, or any object with the same validate(subsets, checks, allowed)).
    Waiting the consolidation TTL is the caller's; nomination is read from ClusterNode.nominated when present."""

    def __init__(self, cluster, plan):
        self.cluster, self.plan = cluster, plan

    def allowed(self, cmd, now=None, not_ready=(), extra_deleting=None):
        """allowed_disruptions for the command's reason, None when no NodePool models budgets."""
        if not budgets_modelled(self.cluster):
            return None
        return allowed_disruptions(self.cluster, _REASON[cmd.method], now, not_ready, extra_deleting)

    def validate_candidates(self, cmd, old_cluster, now=None, not_ready=(), extra_deleting=None):
        """The command's candidates (indices of old_cluster) mapped by node name into the current cluster: (indices,
        None), or (None, reason) when one is gone, marked for deletion or nominated, or - with budgets modelled - when
        the walk over them meets a pool whose allowance for the command's reason is used up."""
        index = {n.node.name: i for i, n in enumerate(self.cluster.nodes)}
        mapped = []
        for c in cmd.candidates:
            name = old_cluster.nodes[c].node.name
            i = index.get(name)
            if i is None:
                return None, f"candidate {name} is gone"
            node = self.cluster.nodes[i]
            if node.deleting:
                return None, f"candidate {name} is marked for deletion"
            if getattr(node, "nominated", False):
                return None, f"candidate {name} is nominated for pending pods"
            mapped.append(i)
        allowed = self.allowed(cmd, now, not_ready, extra_deleting)
        if allowed is not None and len(budget_walk(self.cluster, mapped, allowed)) != len(mapped):
            return None, f"the {_REASON[cmd.method]} budget no longer allows the command's candidates"
        return mapped, None

    @staticmethod
    def option_names(cmd, old_cluster):
        """The instance-type names of the command's replacement (Command.result["replacements"], a materialized
        command: Controller(materialize=True)), through the catalogue of the replacement's NodePool in old_cluster."""
        if cmd.decision != REPLACE:
            return None
        repl = cmd.result.get("replacements")
        if not repl:
            raise ValueError("a REPLACE command without its replacement: compute it with Controller(materialize=True)")
        cat = old_cluster.catalogs[old_cluster.nodepools[repl[0]["nodepool"]].catalog]
        return [cat[int(t)].name for t in repl[0]["options"]]

    def validate_command(self, cmd, old_cluster, now=None, not_ready=(), extra_deleting=None):
        """(ok, reason, kp_validation dict or None). Emptiness: the candidates pass the candidate check and still
        carry no reschedulable pods. Single- and multi-node consolidation: the candidate check, then one
        plan.validate of the mapped candidates with the replacement's options by name."""
        if cmd.method == "drift":
            raise ValueError("Drift commands are not validated")
        mapped, why = self.validate_candidates(cmd, old_cluster, now, not_ready, extra_deleting)
        if mapped is None:
            return False, why, None
        if cmd.method == "emptiness":
            busy = [self.cluster.nodes[i].node.name for i in mapped if self.cluster.nodes[i].pods]
            return (False, f"candidate {busy[0]} is no longer empty", None) if busy else (True, None, None)
        names = self.option_names(cmd, old_cluster)
        check = {"decision": DELETE} if names is None else {"decision": REPLACE, "options": names}
        recs, _ = self.plan.validate([mapped], [check], allowed=self.allowed(cmd, now, not_ready, extra_deleting))
        rec = recs[0]
        return rec["verdict"] == 0, None if rec["verdict"] == 0 else VERDICTS[rec["verdict"]], rec


class _Budgeted:
    """A consolidation method over plan; with allowed (allowed_disruptions of cluster) its candidates are the budget
    walk's."""

    def __init__(self, plan, cluster=None, allowed=None):
        self.plan, self.cluster, self.allowed = plan, cluster, allowed

    def candidates(self, candidates):
        if self.allowed is None:
            return list(candidates)
        return budget_walk(self.cluster, candidates, self.allowed)


class SingleNodeConsolidation(_Budgeted):
    def compute_command(self, candidates):
        """Returns (candidate, result) of the first candidate whose simulation is not a no-op, or None."""
        candidates = self.candidates(candidates)
        if not candidates:
            return None
        res, _ = self.plan.simulate([[c] for c in candidates], multi_node=False)
        for c, r in zip(candidates, res):
            if r["decision"] != NOOP:
                return c, r
        return None


class MultiNodeConsolidation(_Budgeted):
    MAX_PARALLEL = 100  # upstream MultiNodeConsolidation MaxParallel

    @staticmethod
    def search_hi(n):
        """firstNConsolidationOption's initial max: ComputeCommand passes Clamp(n, 0, 100); if n <= max it becomes
        n - 1 (so with more than 100 candidates the search can reach the 101-candidate prefix)."""
        mx = min(max(n, 0), MultiNodeConsolidation.MAX_PARALLEL)
        return n - 1 if n <= mx else mx

    @staticmethod
    def search_prefixes(n):
        """Every mid the binary search can evaluate (prefix length mid+1)."""
        if n < 2:
            return []
        return list(range(1, MultiNodeConsolidation.search_hi(n) + 1))

    @staticmethod
    def replay(n, results_by_mid):
        """firstNConsolidationOption over precomputed computeConsolidation(candidates[0:mid+1]) results."""
        if n < 2:
            return None
        lo, hi = 1, MultiNodeConsolidation.search_hi(n)
        best = None
        while lo <= hi:
            mid = (lo + hi) // 2
            r = results_by_mid[mid]
            if r["decision"] == DELETE or (r["decision"] == REPLACE and r["n_options"] > 0):
                best = (mid, r)
                lo = mid + 1
            else:
                hi = mid - 1
        return best

    def first_n_option(self, candidates):
        """Returns (prefix length, result) of the command firstNConsolidationOption picks, or None; the prefix is of
        self.candidates(candidates), the budget walk's list."""
        candidates = self.candidates(candidates)
        mids = self.search_prefixes(len(candidates))
        if not mids:
            return None
        res, _ = self.plan.simulate([candidates[:m + 1] for m in mids], multi_node=True)
        by_mid = dict(zip(mids, res))
        hit = self.replay(len(candidates), by_mid)
        return None if hit is None else (hit[0] + 1, hit[1])


def random_subsets_csr(n_candidates, n_subsets, seed, max_size=100, min_size=2):
    """n_subsets random subsets of candidate POSITIONS (2..max_size each, distinct, ascending), CSR."""
    rng = np.random.default_rng(seed)
    k = rng.integers(min_size, min(max_size, n_candidates) + 1, size=n_subsets)
    picks = rng.integers(0, n_candidates, size=(n_subsets, int(k.max())))
    picks = np.sort(np.where(np.arange(picks.shape[1])[None, :] < k[:, None], picks, np.iinfo(np.int64).max), axis=1)
    valid = picks != np.iinfo(np.int64).max
    valid[:, 1:] &= picks[:, 1:] != picks[:, :-1]  # drop repeats: subsets stay sets
    sizes = valid.sum(axis=1)
    offs = np.zeros(n_subsets + 1, dtype=np.uint32)
    offs[1:] = np.cumsum(sizes)
    return offs, picks[valid].astype(np.uint32)


SWEEP_CHUNK = 1 << 16  # subsets per generation chunk of the config-4 sweep (chunk c uses seed 1000 + c)


def sweep_subsets(candidates, n_subsets, chunk_lo=0, chunk_hi=None):
    """The config-4 sweep's random candidate subsets (2..100 candidates each), chunks [chunk_lo, chunk_hi) of
    SWEEP_CHUNK subsets concatenated into one CSR over cluster node indices; the set does not depend on how the
    chunks are split over ranks. Returns (offsets, nodes, global index of the first subset)."""
    cands = np.asarray(candidates, dtype=np.uint32)
    n_chunks = (n_subsets + SWEEP_CHUNK - 1) // SWEEP_CHUNK
    chunk_hi = n_chunks if chunk_hi is None else chunk_hi
    offs_l, nodes_l, base = [], [], 0
    for c in range(chunk_lo, chunk_hi):
        n = min(SWEEP_CHUNK, n_subsets - c * SWEEP_CHUNK)
        offs, pos = random_subsets_csr(len(cands), n, seed=1000 + c)
        offs_l.append(offs[:-1] + base)
        nodes_l.append(cands[pos])
        base += int(offs[-1])
    offs_l.append(np.array([base], dtype=np.uint32))
    return (np.concatenate(offs_l).astype(np.uint32),
            np.concatenate(nodes_l) if nodes_l else np.zeros(0, dtype=np.uint32), chunk_lo * SWEEP_CHUNK)


def best_local(results, base_index=0):
    """(savings, global subset index) of the best non-no-op decision in this shard; (-inf, -1) if none."""
    dec = np.array([int(r.decision) for r in results], dtype=np.int32) if not isinstance(results, np.ndarray) else results["decision"]
    sav = np.array([r.savings for r in results], dtype=np.float64) if not isinstance(results, np.ndarray) else results["savings"]
    sav = np.where(dec != NOOP, sav, -np.inf)
    if len(sav) == 0 or not np.isfinite(sav.max()):
        return -np.inf, -1
    i = int(np.argmax(sav))  # first index of the max: ties -> lowest subset index
    return float(sav[i]), base_index + i


def reduce_best(savings, index, dist=None, device=None):
    """Cross-rank argmax of (savings, -index) as two scalar all-reduces (RCCL over xGMI on the GPU path):
    MAX of the savings, then MIN of the subset index among the ranks holding that maximum. Exact (no packing of
    the f64 savings into a key) and deterministic: ties go to the lowest global subset index."""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return savings, index
    import torch
    s = torch.tensor([savings if index >= 0 else -np.inf], dtype=torch.float64, device=device)
    dist.all_reduce(s, op=dist.ReduceOp.MAX)
    best_s = float(s.item())
    if not np.isfinite(best_s):
        return -np.inf, -1
    mine = index >= 0 and savings == best_s
    i = torch.tensor([index if mine else np.iinfo(np.int64).max], dtype=torch.int64, device=device)
    dist.all_reduce(i, op=dist.ReduceOp.MIN)
    return best_s, int(i.item())


def shard(n, rank, world):
    """Contiguous block of [0, n) for this rank."""
    per = (n + world - 1) // world
    lo = min(n, rank * per)
    return lo, min(n, lo + per)


def local_choice(results, base_index=0):
    """kp_choice record of one rank from its per-subset results (dicts or the simulate_csr structured array): the
    best non-no-op decision (savings desc, global subset index asc) and the decision counts."""
    from . import abi
    ch = abi.Choice()
    ch.subset = -1
    dec = [int(r["decision"]) for r in results]
    for k in range(3):
        ch.counts[k] = sum(1 for d in dec if d == k)
    s, i = best_local(results if isinstance(results, np.ndarray) else _as_struct(results), base_index)
    if i >= 0:
        r = results[i - base_index]
        ch.subset = i
        ch.result = abi.SimResult(int(r["decision"]), int(r["nodepool"]), float(r["candidate_price"]),
                                  float(r["replacement_price"]), float(r["savings"]), int(r["n_options"]),
                                  int(r["n_pods"]))
    return ch


def _as_struct(results):
    from . import abi
    out = np.zeros(len(results), dtype=abi.sim_dtype())
    for j, r in enumerate(results):
        out[j]["decision"] = r["decision"]
        out[j]["savings"] = r["savings"]
    return out


def sweep(plan, offsets, nodes, base_index=0, comm=None, multi_node=True, allowed=None):
    """The config-4 sweep step of one rank: kp_consolidate_argmin over this rank's CSR subsets (global indices
    base_index + i); with a Comm the best decision is reduced across ranks inside libkp (RCCL all-gather).
    allowed (allowed_disruptions): the subsets that exceed a NodePool's allowance are gated out on the device
    (kp_consolidate_argmin_budgeted; stats["budget_blocked"]). Returns (choice, stats)."""
    if allowed is None:
        ch, _, st = plan.argmin(offsets, nodes, base_index=base_index, comm=comm, multi_node=multi_node)
    else:
        ch, _, st = plan.argmin(offsets, nodes, base_index=base_index, comm=comm, multi_node=multi_node, allowed=allowed)
    return ch, st
