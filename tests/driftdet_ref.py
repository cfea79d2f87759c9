"""Plain-Python reference of drift detection (kp_cluster_detect_drift; the rule: include/kp/kp_abi.h). It
shares only the model dataclasses with kpamd: dict and set logic for the ladder, the oracle's Requirements.Compatible
for requirement drift and for the AMI map. Records are (reason, status, detail) tuples."""
from oracle import pyoracle

(OK, SKIP_NOT_MANAGED, SKIP_NO_NODECLASS, ERR_INSTANCE, ERR_INSTANCE_TYPE, ERR_NO_AMIS, ERR_NO_SECURITY_GROUPS,
 ERR_NO_SUBNETS) = range(8)
(NONE, NODEPOOL, REQUIREMENTS, NODECLASS, AMI, SECURITY_GROUP, SUBNET, CAPACITY_RESERVATION) = range(8)
REASON_COUNT = 8
NO_AMI = 0xFFFFFFFF
POOL_LABEL = "karpenter.sh/nodepool"

# karpv1.NormalizedLabels
NORMALIZED = {"failure-domain.beta.kubernetes.io/zone": "topology.kubernetes.io/zone",
              "beta.kubernetes.io/arch": "kubernetes.io/arch", "beta.kubernetes.io/os": "kubernetes.io/os",
              "beta.kubernetes.io/instance-type": "node.kubernetes.io/instance-type",
              "failure-domain.beta.kubernetes.io/region": "topology.kubernetes.io/region",
              "topology.ebs.csi.aws.com/zone": "topology.kubernetes.io/zone"}


def static_drift(hash_a, version_a, hash_b, version_b):
    """areStaticFieldsDrifted: all four present, versions equal, hashes different"""
    if None in (hash_a, version_a, hash_b, version_b) or version_a != version_b:
        return False
    return hash_a != hash_b


def labels_as_requirements(labels):
    return [(k, "In", [v]) for k, v in labels.items()]


def requirement_drift(labels, requirements):
    """None when NewLabelRequirements(labels).Compatible(requirements) holds, else the index of the first requirement
    whose key fails: the key's requirements alone are incompatible with the labels."""
    as_reqs = labels_as_requirements(labels)
    if pyoracle.requirements_compatible(as_reqs, list(requirements), allow_wellknown=False):
        return None
    norm = lambda k: NORMALIZED.get(k, k)
    for i, r in enumerate(requirements):
        same_key = [q for q in requirements if norm(q[0]) == norm(r[0])]
        if not pyoracle.requirements_compatible(as_reqs, same_key, allow_wellknown=False):
            return i
    raise AssertionError("incompatible as a whole, compatible key by key")


def ami_for_type(it, amis):
    """MapToInstanceTypes for one type: the index of the first AMI, in list order, the type is compatible with"""
    for i, a in enumerate(amis):
        if pyoracle.requirements_compatible(list(it.requirements), list(a.requirements), allow_wellknown=False):
            return i
    return None


def pool_type(cluster, node, pool):
    """The node's instance type inside its pool's catalogue (by name when the node's catalogue is another), or None"""
    cat = cluster.catalogs[pool.catalog]
    if node.catalog == pool.catalog:
        return cat[node.instance_type] if node.instance_type < len(cat) else None
    name = cluster.catalogs[node.catalog][node.instance_type].name
    return next((it for it in cat if it.name == name), None)


def detect(cluster, inputs=None):
    """(records, counts) for every node of the cluster"""
    inputs = cluster.drift_inputs if inputs is None else inputs
    pool_index = {p.name: i for i, p in enumerate(cluster.nodepools)}
    ami_cache = {}
    records = []
    for node, nd in zip(cluster.nodes, inputs.nodes):
        records.append(_node(cluster, inputs, pool_index, ami_cache, node, nd))
    counts = [0] * REASON_COUNT
    for r in records:
        counts[r[0]] += 1
    return records, counts


def _node(cluster, inputs, pool_index, ami_cache, node, nd):
    p = pool_index.get(node.node.labels.get(POOL_LABEL))
    if p is None:
        return (NONE, SKIP_NOT_MANAGED, 0)
    pool, pd = cluster.nodepools[p], inputs.pools[p]
    if pd.nodeclass < 0:
        return (NONE, SKIP_NO_NODECLASS, 0)
    if static_drift(pd.hash, pd.hash_version, nd.nodepool_hash, nd.nodepool_hash_version):
        return (NODEPOOL, OK, 0)
    failing = requirement_drift(node.node.labels, pool.requirements)
    if failing is not None:
        return (REQUIREMENTS, OK, failing)
    nc = inputs.nodeclasses[pd.nodeclass]
    if static_drift(nc.hash, nc.hash_version, nd.nodeclass_hash, nd.nodeclass_hash_version):
        return (NODECLASS, OK, 0)
    inst = nd.instance
    if inst is None:
        return (NONE, ERR_INSTANCE, 0)
    it = pool_type(cluster, node, pool)
    if it is None:
        return (NONE, ERR_INSTANCE_TYPE, 0)
    if not nc.amis:
        return (NONE, ERR_NO_AMIS, 0)
    key = (pd.nodeclass, pool.catalog, it.name)
    if key not in ami_cache:
        ami_cache[key] = ami_for_type(it, nc.amis)
    mapped = ami_cache[key]
    if not nc.security_groups:
        return (NONE, ERR_NO_SECURITY_GROUPS, 0)
    if not nc.subnets:
        return (NONE, ERR_NO_SUBNETS, 0)
    if mapped is None or nc.amis[mapped].id != inst.image_id:
        return (AMI, OK, NO_AMI if mapped is None else mapped)
    if set(nc.security_groups) != set(inst.security_groups):
        return (SECURITY_GROUP, OK, 0)
    if inst.subnet_id not in nc.subnets:
        return (SUBNET, OK, 0)
    if inst.capacity_reservation_id is not None and inst.capacity_reservation_id not in nc.capacity_reservations:
        return (CAPACITY_RESERVATION, OK, 0)
    return (NONE, OK, 0)
