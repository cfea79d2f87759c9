"""Small catalogues, AMI lists and launch requests for the launch-template grouping (kp_launch_templates),
shared by tests/test_ltgroup_ref.py (the reference against hand-written expectations, CPU) and
tests/test_gpu_ltgroup.py (the device against the reference). A case is (instance types, requests, subnet zones, amis,
max_types). Prices rise with the type's number, so OrderByPrice leaves the types in the order they are built."""
from kpamd.model import AMI, InstanceType, Offering

CT = "karpenter.sh/capacity-type"
ARCH = "kubernetes.io/arch"
ITYPE = "node.kubernetes.io/instance-type"
ZONE = "topology.kubernetes.io/zone"
K = "karpenter.k8s.aws/"
EFA = "vpc.amazonaws.com/efa"
ZONES = ["test-zone-1a", "test-zone-1b", "test-zone-1c"]
GIB = 1024 * 1024 * 1024 * 1000  # milli-bytes

AMD = AMI("ami-123", [(ARCH, "In", ["amd64"])])
ARM = AMI("ami-456", [(ARCH, "In", ["arm64"])])
REQUESTS = {"cpu": 1000, "pods": 1000}


def od(zone, price, available=True):
    return Offering("on-demand", zone, None, float(price), bool(available))


def reserved(zone, rid, capacity, rtype="default", available=True, price=1e-8):
    return Offering("reserved", zone, None, float(price), bool(available), rid, rtype, int(capacity))


def typ(i, arch="amd64", pods=110, efa=None, zones=ZONES, extra=(), offerings=None, name=None):
    """Type number i: on-demand in `zones` at a price that rises with i, or the given offerings"""
    name = name or f"t{i:04d}.large"
    offs = list(offerings) if offerings is not None else [od(z, 1.0 + i / 1024.0) for z in zones]
    cts = ["on-demand", "spot"] + (["reserved"] if any(o.capacity_type == "reserved" for o in offs) else [])
    reqs = [(ITYPE, "In", [name]), (ARCH, "In", [arch]), (CT, "In", cts),
            (ZONE, "In", sorted({o.zone for o in offs}))] + list(extra)
    rids = sorted({o.reservation_id for o in offs if o.reservation_id})
    if rids:
        reqs += [(K + "capacity-reservation-id", "In", rids),
                 (K + "capacity-reservation-type", "In", sorted({o.reservation_type for o in offs if o.reservation_type}))]
    else:
        reqs += [(K + "capacity-reservation-id", "DoesNotExist", []), (K + "capacity-reservation-type", "DoesNotExist", [])]
    cap = {"cpu": 4000, "memory": 16 * GIB, "pods": pods * 1000}
    if efa is not None:
        cap[EFA] = efa * 1000
    return InstanceType(name, reqs, cap, {}, offs)


def request(types, reqs=(), resources=None):
    return (list(reqs), dict(REQUESTS if resources is None else resources), list(range(types)) if isinstance(types, int) else list(types))


def uniform(n, max_types=60, amis=(AMD,), zones=ZONES, **kw):
    """n amd64 types alike but for price: one group"""
    return [typ(i, **kw) for i in range(n)], [request(n)], list(zones), list(amis), max_types


def distinct_pods(n, max_types=60):
    """every type its own pod capacity: every type its own group"""
    return [typ(i, pods=10 + i) for i in range(n)], [request(n)], list(ZONES), [AMD], max_types


def unmapped_at(n, where):
    """n types, the ones at the positions `where` arm64 with an amd64 AMI alone: no AMI takes them"""
    types = [typ(i, arch="arm64" if i in where else "amd64") for i in range(n)]
    return types, [request(n)], list(ZONES), [AMD], 60


def ami_lists():
    """(name, amis) over mixed(): 0, 1, 2 and 9 AMIs; an empty requirement list; a value and a key no type carries under
    positive and negative operators"""
    nine = [AMI(f"ami-{i}", [(K + "instance-family", "In", [f"fam{i}"])]) for i in range(7)] + [ARM, AMD]
    return [("none", []), ("one", [AMD]), ("two", [AMD, ARM]), ("nine", nine),
            ("empty-requirements", [AMI("ami-any", []), AMD]),
            ("unknown-value-in", [AMI("ami-x", [(ARCH, "In", ["riscv"])]), AMD, ARM]),
            ("unknown-value-notin", [AMI("ami-x", [(ARCH, "NotIn", ["riscv"])]), AMD]),
            ("unknown-key-in", [AMI("ami-x", [("example.com/none", "In", ["a"])]), ARM, AMD]),
            ("unknown-key-exists", [AMI("ami-x", [("example.com/none", "Exists", [])]), AMD]),
            ("unknown-key-notin", [AMI("ami-x", [("example.com/none", "NotIn", ["a"])]), AMD]),
            ("unknown-key-dne", [AMI("ami-x", [("example.com/none", "DoesNotExist", [])]), AMD]),
            ("known-key-dne", [AMI("ami-x", [(K + "instance-family", "DoesNotExist", [])]), AMD, ARM]),
            ("gt", [AMI("ami-big", [(K + "instance-cpu", "Gt", ["8"])]), AMD, ARM]),
            ("two-keys", [AMI("ami-x", [(ARCH, "In", ["arm64"]), (K + "instance-family", "In", ["fam1"])]), AMD, ARM])]


def mixed(n=12):
    """amd64 and arm64 types of a few families, cpu sizes and pod capacities; every other arm64 type has no family"""
    types = []
    for i in range(n):
        arm = i % 3 == 2
        extra = [(K + "instance-cpu", "In", [str(4 << (i % 3))])]
        if not (arm and i % 2):
            extra.append((K + "instance-family", "In", [f"fam{i % 4}"]))
        types.append(typ(i, arch="arm64" if arm else "amd64", pods=[29, 58, 110][i % 3 if i < 6 else 0], extra=extra))
    return types


def efa_types():
    """EFA counts 0 (key absent), 0 (key present), 1, 1, 4"""
    return [typ(0), typ(1, efa=0), typ(2, efa=1), typ(3, efa=1), typ(4, efa=4)]


def reservation_suite():
    """R:pkg/providers/launchtemplate/suite_test.go:2461: m5.large reserved twice in 1a (10 and 15 instances) and once
    in 1b, m5.xlarge once in 1b; the request asks for reserved capacity"""
    large = typ(0, name="m5.large", offerings=[od(z, 0.096) for z in ZONES] + [
        reserved("test-zone-1a", "cr-m5.large-1a-1", 10), reserved("test-zone-1a", "cr-m5.large-1a-2", 15),
        reserved("test-zone-1b", "cr-m5.large-1b-1", 10)])
    xlarge = typ(1, name="m5.xlarge", offerings=[od(z, 0.192) for z in ZONES] + [
        reserved("test-zone-1b", "cr-m5.xlarge-1b-1", 15, price=2e-8)])
    return [large, xlarge], [request(2, [(CT, "In", ["reserved"])])], list(ZONES), [AMD], 60


def reserved_edges():
    """Reserved launches at the slice's edges, one request each over its own types: a reservation in a zone without a
    subnet (its config is dropped), an unavailable reservation beside an available one, a capacity block, a type no
    AMI takes, and a request that pins one of two reservations by id"""
    rq = [(CT, "In", ["reserved", "on-demand"])]
    types = [
        typ(0, offerings=[od("test-zone-1a", 1.0), reserved("test-zone-1a", "cr-a", 3), reserved("test-zone-1c", "cr-c", 5)]),
        typ(1, offerings=[od("test-zone-1a", 1.1), reserved("test-zone-1a", "cr-gone", 0, available=False),
                          reserved("test-zone-1b", "cr-b", 2)]),
        typ(2, offerings=[reserved("test-zone-1a", "cr-block-1", 1, "capacity-block", price=3e-8),
                          reserved("test-zone-1b", "cr-block-2", 1, "capacity-block", price=2e-8), od("test-zone-1a", 1.2)]),
        typ(3, arch="arm64", offerings=[od("test-zone-1a", 1.3), reserved("test-zone-1a", "cr-arm", 4)]),
        typ(4, offerings=[od("test-zone-1b", 1.4), reserved("test-zone-1b", "cr-p1", 9), reserved("test-zone-1b", "cr-p2", 1)]),
        typ(5, offerings=[od("test-zone-1c", 1.5), reserved("test-zone-1c", "cr-only-c", 2)]),
    ]
    requests = [request([0], rq), request([1], rq), request([2], rq), request([3], rq),
                request([4], rq + [(K + "capacity-reservation-id", "In", ["cr-p2"])]), request([5], rq),
                request([0, 1, 3, 4], rq), request([0, 1], [(CT, "In", ["on-demand"])])]
    return types, requests, ["test-zone-1a", "test-zone-1b"], [AMD], 60


def statuses():
    """OK, insufficient capacity (no type fits) and minValues (two families asked of one) in one call"""
    types = [typ(i, pods=[29, 110][i % 2], extra=[(K + "instance-family", "In", ["fam0"])]) for i in range(6)]
    requests = [request(6), request(6, resources={"cpu": 64000}),
                request(6, [(K + "instance-family", "Exists", [], 2)]), request([]), request([4, 1])]
    return types, requests, list(ZONES), [AMD], 60
