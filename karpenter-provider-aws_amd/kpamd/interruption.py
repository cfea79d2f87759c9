"""The interruption controller around kp_cluster_interruptions — the caller model, next to kpamd.disruption.

The reference's controller (R:pkg/controllers/interruption/controller.go) receives a batch of SQS messages, parses each
(EventParser.Parse, parser.go:74-93, and the four parsers under messages/), looks up the NodeClaims of every instance id
one List at a time, marks the spot offering of an interrupted NodeClaim unavailable and deletes the NodeClaim. Here:

  parse(body)                 EventParser.Parse with the four parsers: (kind, instance ids), or ParseError
  instance_id(provider_id)    utils.ParseInstanceID: the last path segment, None when the id has not the known format
  Controller.reconcile(...)   parses the batch, resolves it on the device in one call (ClusterPlan.interruptions) and
                              turns the marks into Catalog.update_offerings records

Stays with the Go caller: SQS receive and delete, events, latency metrics and the API delete of each NodeClaim."""
import json
import re
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

from . import abi

ITYPE = "node.kubernetes.io/instance-type"
ZONE = "topology.kubernetes.io/zone"
NODEPOOL = "karpenter.sh/nodepool"
CAPACITY_TYPE = "karpenter.sh/capacity-type"

# the parser map's keys: (version, source, detail-type)
STATE_CHANGE = ("0", "aws.ec2", "EC2 Instance State-change Notification")
SPOT_INTERRUPTION = ("0", "aws.ec2", "EC2 Spot Instance Interruption Warning")
SCHEDULED_CHANGE = ("0", "aws.health", "AWS Health Event")
REBALANCE = ("0", "aws.ec2", "EC2 Instance Rebalance Recommendation")
ACCEPTED_STATES = frozenset(("stopping", "stopped", "shutting-down", "terminated"))

_PROVIDER_ID = re.compile(r"(.*):///(.*)/(.*)")
_RFC3339 = re.compile(r"\d{4}-\d{2}-\d{2}T\d{2}:\d{2}:\d{2}(\.\d+)?(Z|[+-]\d{2}:\d{2})")


class ParseError(ValueError):
    """The body is not the JSON its parser expects. The controller logs it, counts it and deletes the message."""


def _str(obj, key):
    """A string field as encoding/json leaves it in a struct: absent or null is the zero value, another type an error"""
    v = obj.get(key)
    if v is None:
        return ""
    if not isinstance(v, str):
        raise ParseError(f"{key}: a {type(v).__name__} where a string is expected")
    return v


def _detail(msg):
    d = msg.get("detail")
    if d is None:
        return {}
    if not isinstance(d, dict):
        raise ParseError("detail: not an object")
    return d


def parse(body):
    """EventParser.Parse: (kind, [instance id]) with kind an abi.MSG_* value. An empty body and a (version, source,
    detail-type) no parser is registered for are no_op; so is a state change to a state outside ACCEPTED_STATES
    (compared lower-cased, statechange/parser.go:38) and a health event that is not EC2 / scheduledChange. A state change's kind
    compares the state as written (statechange/model.go:40-45): "STOPPED" is accepted and is instance_terminated."""
    if body == "":
        return abi.MSG_NO_OP, []
    try:
        msg = json.loads(body)
    except (ValueError, TypeError) as e:
        raise ParseError(f"unmarshalling the message as Metadata, {e}") from None
    if msg is None:  # JSON null unmarshals into the zero Metadata: no parser has the empty key
        return abi.MSG_NO_OP, []
    if not isinstance(msg, dict):
        raise ParseError("unmarshalling the message as Metadata, not an object")
    for k in ("account", "id", "region"):
        _str(msg, k)
    res = msg.get("resources")
    if res is not None and (not isinstance(res, list) or not all(r is None or isinstance(r, str) for r in res)):
        raise ParseError("resources: not an array of strings")
    when = msg.get("time")
    if when is not None and (not isinstance(when, str) or not _RFC3339.fullmatch(when)):
        raise ParseError("time: not an RFC 3339 time")  # (Metadata.Time is a time.Time)
    key = (_str(msg, "version"), _str(msg, "source"), _str(msg, "detail-type"))
    if key == STATE_CHANGE:
        d = _detail(msg)
        state = _str(d, "state")
        if state.lower() not in ACCEPTED_STATES:
            return abi.MSG_NO_OP, []
        kind = abi.MSG_INSTANCE_STOPPED if state in ("stopping", "stopped") else abi.MSG_INSTANCE_TERMINATED
        return kind, [_str(d, "instance-id")]
    if key == SPOT_INTERRUPTION:
        return abi.MSG_SPOT_INTERRUPTED, [_str(_detail(msg), "instance-id")]
    if key == REBALANCE:
        return abi.MSG_REBALANCE_RECOMMENDATION, [_str(_detail(msg), "instance-id")]
    if key == SCHEDULED_CHANGE:
        d = _detail(msg)
        if _str(d, "service") != "EC2" or _str(d, "eventTypeCategory") != "scheduledChange":
            return abi.MSG_NO_OP, []
        entities = d.get("affectedEntities") or []
        if not isinstance(entities, list):
            raise ParseError("affectedEntities: not an array")
        ids = []
        for e in entities:
            if e is not None and not isinstance(e, dict):
                raise ParseError("affectedEntities: an entry is not an object")
            ids.append(_str(e or {}, "entityValue"))
        return abi.MSG_SCHEDULED_CHANGE, ids
    return abi.MSG_NO_OP, []


def instance_id(provider_id):
    """utils.ParseInstanceID (R:pkg/utils/utils.go:36-52): the last path segment of provider:///zone/id; None when the
    provider id is absent or has not that format (such a NodeClaim is not indexed under any instance id)."""
    if not provider_id:
        return None
    m = _PROVIDER_ID.search(provider_id)
    return m.group(3) if m else None


@dataclass
class Reconciled:
    """What one Reconcile decided. deletes: (node index, message index, kind) in node order, the NodeClaims the caller
    deletes. marks: (instance type name, zone, nodes that carry it). updates: per catalogue index the records handed to
    Catalog.update_offerings. disrupted: NodeClaimsDisruptedTotal's increments by (kind name, NodePool, capacity type).
    received: messages per kind name (ReceivedMessages). parse_errors: bodies that did not parse (their messages are
    deleted from the queue like every other). nodes / matches: the device's records."""
    deletes: List[Tuple[int, int, int]] = field(default_factory=list)
    marks: List[Tuple[str, str, int]] = field(default_factory=list)
    updates: Dict[int, list] = field(default_factory=dict)
    disrupted: Dict[Tuple[str, str, str], int] = field(default_factory=dict)
    received: Dict[str, int] = field(default_factory=dict)
    parse_errors: int = 0
    nodes: list = field(default_factory=list)
    matches: list = field(default_factory=list)
    stats: dict = field(default_factory=dict)


def mark_updates(instance_types, marks):
    """The Catalog.update_offerings records of marks [(type name, zone)] for one catalogue: (type index, "spot", zone,
    False) wherever a type of that name has a spot offering in that zone. A mark the catalogue has no such offering for
    yields nothing: the reference's cache is keyed by name and a catalogue without the offering never reads the key."""
    by_name = {}
    for t, it in enumerate(instance_types):
        by_name.setdefault(it.name, []).append(t)
    ups = []
    for name, zone in marks:
        for t in by_name.get(name, ()):
            if any(o.capacity_type == "spot" and o.zone == zone for o in instance_types[t].offerings):
                ups.append((t, "spot", zone, False))
    return ups


class Controller:
    """One Reconcile of the interruption controller over a batch of message bodies."""

    def reconcile(self, bodies, cluster, plan, catalogs, seqnum, table_log2=0):
        """bodies: the SQS message bodies (None: a message without a body, a parse error). cluster / plan: the snapshot
        and its ClusterPlan (or any object with its interruptions()); a node's instance id is instance_id() of its
        ClusterNode.provider_id. catalogs: the plan's kpamd.Catalog objects; each one that has an offering some mark
        names is updated with seqnum, all or nothing, and the caller then refreshes what is resident on them
        (ClusterPlan.refresh, SolvePlan.refresh). Returns a Reconciled."""
        out = Reconciled(received={n: 0 for n in abi.MESSAGE_KIND_NAMES})
        messages = []
        for body in bodies:
            try:
                if body is None:
                    raise ParseError("message or message body is nil")
                kind, ids = parse(body)
            except ParseError:
                out.parse_errors += 1
                continue
            out.received[abi.MESSAGE_KIND_NAMES[kind]] += 1
            messages.append((kind, ids))
        node_ids = [instance_id(n.provider_id) for n in cluster.nodes]
        res = plan.interruptions(messages, node_ids, table_log2=table_log2)
        out.nodes, out.matches, out.stats = res["nodes"], res["matches"], res.get("stats", {})
        for d in res["deletes"]:
            labels = cluster.nodes[d["node"]].node.labels
            out.deletes.append((d["node"], d["message"], d["kind"]))
            key = (abi.MESSAGE_KIND_NAMES[d["kind"]], labels.get(NODEPOOL, ""), labels.get(CAPACITY_TYPE, ""))
            out.disrupted[key] = out.disrupted.get(key, 0) + 1
        for m in res["marks"]:
            labels = cluster.nodes[m["node"]].node.labels
            out.marks.append((labels[ITYPE], labels[ZONE], m["n_nodes"]))
        pairs = [(name, zone) for name, zone, _ in out.marks]
        for c, cat in enumerate(catalogs):
            ups = mark_updates(cat.instance_types, pairs)
            if ups:
                cat.update_offerings(ups, seqnum)
                out.updates[c] = ups
        return out
