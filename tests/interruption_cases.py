"""Inputs of tests/test_interruption_ref.py and tests/test_gpu_interruption.py: clusters, instance ids and message
batches built for one edge of kp_cluster_interruptions each - TEST INFRASTRUCTURE. A case is
(cluster, node_ids, messages, table_log2); messages are (kind, [instance id]) with interruption_ref's kinds."""
import numpy as np

import interruption_ref as ref
from kpamd import synth
from kpamd.model import Cluster, ClusterNode, ExistingNode, NodePool, PodShape

TYPES = ("m5.large", "m5.2xlarge", "c5.large", "t3.large", "r5.large")
ZONES = synth.ZONES
CT = "karpenter.sh/capacity-type"


def types_named(catalog, names=TYPES):
    by = {it.name: it for it in catalog}
    return [by[n] for n in names]


def iid(n, width=17):
    """An EC2 instance id: i- and 17 hex digits, 19 bytes"""
    return "i-" + format(n, "x").rjust(width, "0")


def provider_id(instance_id, zone="test-zone-1a"):
    return f"aws:///{zone}/{instance_id}"


class Build:
    """A cluster node by node; every node a spot m5.large in zone 0 of pool `default` unless said otherwise"""

    def __init__(self, catalogs):
        self.catalogs = catalogs
        self.nodes, self.ids = [], []

    def node(self, instance_id, type_name="m5.large", zone=0, ct="spot", catalog=0, deleting=False, labels=None,
             pool="default"):
        """labels: added to the launched node's; a value of None removes the label. instance_id None: no provider id"""
        cat = self.catalogs[catalog]
        t = next(i for i, it in enumerate(cat) if it.name == type_name)
        name = f"node-{len(self.nodes)}"
        lab = synth.node_labels(cat[t], zone, ct, pool, name)
        for k, v in (labels or {}).items():
            if v is None:
                lab.pop(k, None)
            else:
                lab[k] = v
        node = ClusterNode(ExistingNode(name, lab, {"cpu": 1000, "memory": 1 << 30, "pods": 100}), catalog, t,
                           deleting=deleting,
                           provider_id=None if instance_id is None else provider_id(instance_id, ZONES[zone]))
        self.nodes.append(node)
        self.ids.append(instance_id)
        return len(self.nodes) - 1

    def build(self, name, messages, table_log2=0):
        empty = np.zeros(0, dtype=np.uint32)
        pools = [NodePool("default", 0, 0, []), NodePool("other", 0, len(self.catalogs) - 1, [])]
        cl = Cluster(self.catalogs, pools, self.nodes, [PodShape(synth.req_res(100, 128))], empty,
                     np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint64), name=name)
        return cl, list(self.ids), messages, table_log2


def reference_suite_node(catalog, labels=None):
    """The suite's BeforeEach NodeClaim (R:pkg/controllers/interruption/suite_test.go:95-127): one NodeClaim of pool
    `default` with a provider id"""
    b = Build([types_named(catalog)])
    b.node(iid(0xabc), "t3.large", labels=labels)
    return b


def sized(catalog, n_nodes, n_messages, seed=0):
    """n_nodes nodes with distinct ids over the types and zones, n_messages messages of every kind: two thirds name a
    node, the rest nobody; every fifth scheduled change carries three ids"""
    rng = np.random.default_rng(1000 * n_nodes + n_messages + seed)
    b = Build([types_named(catalog)])
    for i in range(n_nodes):
        b.node(iid(0x5000 + i), TYPES[i % len(TYPES)], zone=i % 3, ct="spot" if i % 4 else "on-demand",
               deleting=(i % 7 == 3))
    msgs = []
    for m in range(n_messages):
        kind = int(rng.integers(0, 6))
        pick = lambda: iid(0x5000 + int(rng.integers(0, n_nodes))) if n_nodes and rng.random() < 0.67 else iid(0x900000 + m)
        ids = [pick() for _ in range(3)] if kind == ref.SCHEDULED_CHANGE and m % 5 == 0 else [pick()]
        msgs.append((kind, ids))
    return b.build(f"interruption-{n_nodes}-nodes-{n_messages}-messages", msgs)


def shared_id(catalog, copies, home=None, slots_log2=0):
    """`copies` nodes sharing one instance id among three others. home / slots_log2: the id is chosen so that its home
    slot in a forced table of 1 << slots_log2 slots is `home`; with home the last slot the duplicates' run wraps."""
    b = Build([types_named(catalog)])
    k = 0
    if slots_log2:
        while ref.table_hash(iid(0x77000 + k)) & ((1 << slots_log2) - 1) != home:
            k += 1
    dup = iid(0x77000 + k)
    b.node(iid(1))
    for c in range(copies):
        b.node(dup, TYPES[c % len(TYPES)], zone=c % 3, deleting=(c == 1))
    b.node(iid(2))
    b.node(iid(3), deleting=True)
    msgs = [(ref.REBALANCE, [dup]), (ref.SPOT, [dup]), (ref.TERMINATED, [iid(2)]), (ref.SCHEDULED_CHANGE, [iid(9), dup, iid(3)])]
    return b.build(f"interruption-shared-id-{copies}", msgs, slots_log2)


def smallest_table(catalog, copies, home):
    """copies duplicates alone in the smallest legal table (the least power of two above the node count), their run
    starting at slot `home`"""
    log2 = max(1, int(copies).bit_length())  # 1 << log2 > copies
    b = Build([types_named(catalog)])
    k = 0
    while ref.table_hash(iid(0x88000 + k)) & ((1 << log2) - 1) != home:
        k += 1
    dup = iid(0x88000 + k)
    for c in range(copies):
        b.node(dup, zone=c % 3)
    return b.build(f"interruption-smallest-table-{copies}-home-{home}",
                   [(ref.SPOT, [dup]), (ref.STOPPED, [iid(5)]), (ref.SCHEDULED_CHANGE, [dup, dup])], log2)


def forced_load(catalog, n_nodes, quarter):
    """n_nodes distinct ids in a forced table: the smallest legal one (long runs), or one at a quarter load"""
    cl, ids, msgs, _ = sized(catalog, n_nodes, 65, seed=3)
    log2 = int(n_nodes).bit_length() + (2 if quarter else 0)
    if quarter:
        assert n_nodes * 4 <= (1 << log2) < n_nodes * 8
    return cl, ids, msgs, log2


def scheduled_changes(catalog):
    """Scheduled changes with 0, 1 and 3 ids, and one id twice; ids that match nothing first, in the middle and last"""
    b = Build([types_named(catalog)])
    for i in range(6):
        b.node(iid(0x10 + i), zone=i % 3)
    a = [iid(0x10 + i) for i in range(6)]
    gone = [iid(0xdead0 + i) for i in range(4)]
    msgs = [(ref.SCHEDULED_CHANGE, []), (ref.SCHEDULED_CHANGE, [a[0]]), (ref.SCHEDULED_CHANGE, [a[1], a[2], a[3]]),
            (ref.SCHEDULED_CHANGE, [a[4], a[4]]), (ref.SCHEDULED_CHANGE, [gone[0], a[5], a[0]]),
            (ref.SCHEDULED_CHANGE, [a[1], gone[1], a[2]]), (ref.SCHEDULED_CHANGE, [a[3], a[4], gone[2]]),
            (ref.SCHEDULED_CHANGE, [gone[3]]), (ref.SCHEDULED_CHANGE, [])]
    return b.build("interruption-scheduled-changes", msgs)


def long_and_close_ids(catalog):
    """An id of 31 bytes, two ids equal in their first 16 bytes, an id that is a prefix of another, an empty id"""
    b = Build([types_named(catalog)])
    long_id = "i-" + "f" * 29
    left, right = "i-0123456789abcdeX", "i-0123456789abcdeY"   # they differ at byte 17
    assert len(long_id) == 31 and left[:16] == right[:16]
    for x in (long_id, left, right, "i-0123456789abcde", long_id[:-1], ""):
        b.node(x)
    msgs = [(ref.SPOT, [long_id]), (ref.STOPPED, [right]), (ref.TERMINATED, ["i-0123456789abcde"]),
            (ref.SCHEDULED_CHANGE, [left, long_id[:-2], ""]), (ref.REBALANCE, [long_id[:-1]])]
    return b.build("interruption-long-and-close-ids", msgs)


def kind_orders(catalog):
    """One node hit by kinds 1, 3 and 5 in each of the six orders (first_message skips the rebalance message), nodes
    hit only by rebalance and no_op messages, and a no_op that carries ids"""
    import itertools
    b = Build([types_named(catalog)])
    msgs = []
    for o, order in enumerate(itertools.permutations((ref.REBALANCE, ref.SPOT, ref.TERMINATED))):
        b.node(iid(0x100 + o), zone=o % 3)
        msgs += [(k, [iid(0x100 + o)]) for k in order]
    b.node(iid(0x200))
    b.node(iid(0x201))
    msgs += [(ref.REBALANCE, [iid(0x200)]), (ref.NO_OP, [iid(0x201), iid(0x200)]), (ref.NO_OP, []), (ref.REBALANCE, [iid(0x200)])]
    return b.build("interruption-kind-orders", msgs)


def only_notifications(catalog):
    b = Build([types_named(catalog)])
    for i in range(5):
        b.node(iid(0x300 + i))
    msgs = [(ref.REBALANCE, [iid(0x300)]), (ref.NO_OP, [iid(0x301)]), (ref.REBALANCE, [iid(0x302)]), (ref.NO_OP, [])]
    return b.build("interruption-only-notifications", msgs)


def ice_marks(catalog):
    """Deleting nodes hit by spot messages (a mark, no delete), an on-demand node hit by one (marked), nodes missing
    either label or carrying an empty one, a node without an id, many nodes under one (type, zone), a pair hit by a
    state change only (no mark), and one type name in two catalogues"""
    b = Build([types_named(catalog), types_named(catalog, ("m5.large", "c5.large"))])
    spot = []

    def hit(*a, **kw):
        n = b.node(iid(0x400 + len(b.nodes)), *a, **kw)
        spot.append(b.ids[n])
        return n
    hit("m5.large", zone=0, deleting=True)
    hit("m5.2xlarge", zone=1, ct="on-demand")
    hit("c5.large", zone=2, labels={ref.ITYPE: None})
    hit("c5.large", zone=2, labels={ref.ZONE: None})
    hit("c5.large", zone=2, labels={ref.ITYPE: ""})
    hit("c5.large", zone=2, labels={ref.ZONE: ""})
    b.node(None, "t3.large", zone=0)
    for i in range(70):                                  # one mark for 70 nodes, its lowest node in the first wave
        hit("t3.large", zone=1, deleting=(i % 9 == 0))
    stopped = b.node(iid(0x999), "m5.2xlarge", zone=2)
    hit("m5.large", zone=0, catalog=1, pool="other")    # the pair of node 0, through another catalogue
    hit("c5.large", zone=0, catalog=1, pool="other")
    hit("m5.large", zone=0, labels={ref.ITYPE: "m5.large ", CT: "spot"})  # another string: another mark
    msgs = [(ref.SPOT, [x]) for x in spot] + [(ref.STOPPED, [b.ids[stopped]])]
    return b.build("interruption-ice-marks", msgs)


def compaction(catalog, n_nodes, pattern):
    """n_nodes nodes of which all, none or every other one are hit by a spot message. With `all` the first 17 nodes
    share a (type, zone) pair and every later node has one of its own, so that marks are emitted up to the last node
    and compact beside the deletes across the block boundary (49 zone values: a plan takes at most 64 per key);
    otherwise the pairs repeat every 12 nodes"""
    b = Build([types_named(catalog)])
    msgs = []
    for i in range(n_nodes):
        if pattern == "all":
            k = max(0, i - 16)
            b.node(iid(0x6000 + i), TYPES[k % len(TYPES)], zone=i % 3, labels={ref.ZONE: f"zone-{k // len(TYPES)}"})
        else:
            b.node(iid(0x6000 + i), TYPES[i % len(TYPES)], zone=(i // 4) % 3)
        if pattern == "all" or (pattern == "alternate" and i % 2 == 0):
            msgs.append((ref.SPOT, [iid(0x6000 + i)]))
    if pattern == "none":
        msgs.append((ref.SPOT, [iid(0x1)]))
    return b.build(f"interruption-compaction-{n_nodes}-{pattern}", msgs)


def storm(catalog, n_messages, n_nodes=None, seed=9):
    """The reference benchmark's mix (makeDiverseMessagesAndNodes, R:pkg/controllers/interruption/
    interruption_benchmark_test.go): a third scheduled_change, a third spot, the rest state changes, each naming a node
    of its own, over a cluster of n_nodes (default: as many) spot nodes"""
    n_nodes = n_messages if n_nodes is None else n_nodes
    rng = np.random.default_rng(seed)
    b = Build([types_named(catalog)])
    for i in range(n_nodes):
        b.node(iid(0xa00000 + i), TYPES[i % 4], zone=i % 3)
    targets = rng.permutation(n_nodes)[:n_messages] if n_nodes >= n_messages else rng.integers(0, max(n_nodes, 1), n_messages)
    msgs = []
    for m in range(n_messages):
        x = iid(0xa00000 + int(targets[m]))
        kind = (ref.SCHEDULED_CHANGE, ref.SPOT, ref.STOPPED if m % 2 else ref.TERMINATED)[m % 3]
        msgs.append((kind, [x]))
    return b.build(f"interruption-storm-{n_messages}-{n_nodes}", msgs)
