"""The plain-Python reference of kp_cluster_interruptions (the rule: include/kp/kp_abi.h) - TEST
INFRASTRUCTURE. Dicts and loops: handleMessage's one lookup per instance id (R:pkg/controllers/interruption/
controller.go:160-248), restated for a whole batch. It reads the model objects, never the library."""
NO_OP, REBALANCE, SCHEDULED_CHANGE, SPOT, STOPPED, TERMINATED = range(6)
KIND_NAMES = ("no_op", "rebalance_recommendation", "scheduled_change", "spot_interrupted", "instance_stopped",
              "instance_terminated")
DELETE, ALREADY_DELETING, ICE = 1, 2, 4
ITYPE = "node.kubernetes.io/instance-type"
ZONE = "topology.kubernetes.io/zone"


def acts(kind):
    """actionForMessage is CordonAndDrain (:272-279)"""
    return kind in (SCHEDULED_CHANGE, SPOT, STOPPED, TERMINATED)


def resolve(cluster, messages, node_ids):
    """messages [(kind, [instance id])], node_ids [id or None] per node of cluster.nodes -> the dict
    ClusterPlan.interruptions returns, without stats."""
    assert len(node_ids) == len(cluster.nodes)
    by_id = {}
    for n, nid in enumerate(node_ids):
        if nid is not None:
            by_id.setdefault(nid, []).append(n)
    recs = [{"first_message": -1, "kinds": 0, "n_messages": 0, "flags": 0} for _ in cluster.nodes]
    spot_hit = [False] * len(cluster.nodes)
    matches = []
    for m, (kind, ids) in enumerate(messages):
        for iid in ids:
            if kind == NO_OP:            # returned before EC2InstanceIDs() is read (:164-166)
                matches.append(0)
                continue
            hit = by_id.get(iid, [])
            matches.append(len(hit))
            for n in hit:
                r = recs[n]
                r["kinds"] |= 1 << kind
                r["n_messages"] += 1
                if acts(kind) and (r["first_message"] < 0 or m < r["first_message"]):
                    r["first_message"] = m
                if kind == SPOT:
                    spot_hit[n] = True
    deletes, counts = [], [0] * 6
    carriers = {}                        # (type label, zone label) -> the nodes that carry the mark, ascending
    for n, node in enumerate(cluster.nodes):
        r = recs[n]
        if r["first_message"] >= 0:
            if node.deleting:            # deleteNodeClaim returns early (:234-236)
                r["flags"] |= ALREADY_DELETING
            else:
                r["flags"] |= DELETE
                kind = messages[r["first_message"]][0]
                deletes.append({"node": n, "message": r["first_message"], "kind": kind})
                counts[kind] += 1
        labels = node.node.labels
        if spot_hit[n] and labels.get(ITYPE, "") != "" and labels.get(ZONE, "") != "":   # (:218-225)
            r["flags"] |= ICE
            carriers.setdefault((labels[ITYPE], labels[ZONE]), []).append(n)
    marks = sorted(({"node": ns[0], "n_nodes": len(ns)} for ns in carriers.values()), key=lambda m: m["node"])
    return {"nodes": recs, "matches": matches, "deletes": deletes, "marks": marks, "counts": counts}


class RefPlan:
    """resolve() behind ClusterPlan.interruptions' signature, for kpamd.interruption.Controller on the CPU"""

    def __init__(self, cluster):
        self.cluster = cluster

    def interruptions(self, messages, node_ids, table_log2=0):
        return resolve(self.cluster, messages, node_ids)


def table_hash(iid):
    """The hash the join's kernels give an id's zero-padded 32-byte slot (csrc/kp_interrupt.hip ir_hash): only the
    case builders use it, to aim a probe run at the end of a forced table. If the two ever differ the cases still
    compare equal; they merely stop wrapping."""
    b = iid.encode().ljust(32, b"\0")
    h = 0x811C9DC5
    for i in range(8):
        h = ((h ^ int.from_bytes(b[4 * i:4 * i + 4], "little")) * 0x01000193) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
    h ^= h >> 12
    return h
