"""Inputs of tests/test_driftdet.py and tests/test_gpu_driftdet.py: clusters with DriftInputs built for one edge of
drift detection each, every node with the expectation written out by hand from the rule, so that the CPU
half shows the reference (tests/driftdet_ref.py) lands on the edge the builder claims and the GPU half compares the
device with the reference. R: is the reference project, line numbers as of its pkg/cloudprovider/suite_test.go.

A record is (reason, status, detail); the names are driftdet_ref's."""
import numpy as np

import driftdet_ref as ref
from kpamd import catalog as kcatalog
from kpamd import synth
from kpamd.model import (AMI, Cluster, ClusterNode, DriftInputs, ExistingNode, InstanceInfo, NodeClassStatus, NodeDrift,
                         NodePool, PodShape, PoolDrift)

K = "karpenter.k8s.aws/"
ARCH, OS, BUILD, ITYPE = ("kubernetes.io/arch", "kubernetes.io/os", "node.kubernetes.io/windows-build",
                          "node.kubernetes.io/instance-type")
ZONE = "topology.kubernetes.io/zone"
TYPES = ("m5.large", "m5.2xlarge", "c5.large", "g4dn.xlarge", "inf2.xlarge", "m6g.large")
AMD = AMI("ami-amd64", [(ARCH, "In", ["amd64"])])
ARM = AMI("ami-arm64", [(ARCH, "In", ["arm64"])])
STANDARD = AMI("ami-standard", [(K + "instance-accelerator-count", "DoesNotExist", []),
                                (K + "instance-gpu-count", "DoesNotExist", [])])   # R:pkg/providers/amifamily/types.go:88-92
NVIDIA = AMI("ami-nvidia", [(K + "instance-gpu-count", "Exists", [])])               # :93-94
NEURON = AMI("ami-neuron", [(K + "instance-accelerator-count", "Exists", [])])       # :95-96
WIN2019 = AMI("ami-win2019", [(OS, "In", ["windows"]), (BUILD, "In", ["10.0.17763"])])
WIN2022 = AMI("ami-win2022", [(OS, "In", ["windows"]), (BUILD, "In", ["10.0.20348"])])

NOT_DRIFTED = (ref.NONE, ref.OK, 0)


def types_named(catalog, names=TYPES):
    by = {it.name: it for it in catalog}
    return [by[n] for n in names]


class Suite:
    """A cluster node by node, each with its expectation. Every nodeclass starts as the suite's BeforeEach leaves it
    (R::661-805): an amd64 and an arm64 AMI, three subnets, one security group, equal hashes; every node as an
    m5.large instance launched from it."""

    def __init__(self, catalogs):
        self.catalogs = catalogs
        self.pools, self.pdrift, self.classes = [], [], []
        self.nodes, self.ndrift, self.want = [], [], {}

    def nodeclass(self, **kw):
        base = dict(amis=[AMD, ARM], subnets=["subnet-1", "subnet-2", "subnet-3"], security_groups=["sg-valid"],
                    capacity_reservations=[], hash="class-hash", hash_version="v1")
        base.update(kw)
        self.classes.append(NodeClassStatus(**base))
        return len(self.classes) - 1

    def pool(self, name, nodeclass=None, requirements=(), catalog=0, pool_hash="pool-hash", pool_hash_version="v1", **nc):
        """A NodePool with a nodeclass of its own (nc: what differs from the base), unless one is given"""
        if nodeclass is None:
            nodeclass = self.nodeclass(**nc)
        self.pools.append(NodePool(name, 0, catalog, list(requirements)))
        self.pdrift.append(PoolDrift(nodeclass, pool_hash, pool_hash_version))
        return name

    def node(self, name, pool, want, type_name="m5.large", catalog=0, labels=None, instance="default", **ann):
        """labels: added to the launched node's; a value of None removes the label. instance: InstanceInfo fields
        that differ from a clean launch, or None for no instance. ann: NodeDrift annotations that differ."""
        cat = self.catalogs[catalog]
        t = next(i for i, it in enumerate(cat) if it.name == type_name)
        lab = synth.node_labels(cat[t], 0, "on-demand", pool, name)
        for k, v in (labels or {}).items():
            if v is None:
                lab.pop(k, None)
            else:
                lab[k] = v
        self.nodes.append(ClusterNode(ExistingNode(name, lab, {"cpu": 1000, "memory": 1 << 30, "pods": 100}), catalog, t))
        inst = None
        if instance is not None:
            f = dict(image_id="ami-amd64", subnet_id="subnet-1", security_groups=["sg-valid"], capacity_reservation_id=None)
            f.update({} if instance == "default" else instance)
            inst = InstanceInfo(**f)
        a = dict(nodepool_hash="pool-hash", nodepool_hash_version="v1", nodeclass_hash="class-hash",
                 nodeclass_hash_version="v1")
        a.update(ann)
        self.ndrift.append(NodeDrift(instance=inst, **a))
        assert name not in self.want
        self.want[name] = want

    def case(self, name, want, requirements=(), type_name="m5.large", labels=None, instance="default", ann=None, **nc):
        """one pool, one nodeclass and one node for one case"""
        self.pool("pool-" + name, requirements=requirements, **nc)
        self.node(name, "pool-" + name, want, type_name, labels=labels, instance=instance, **(ann or {}))

    def build(self, name):
        empty = np.zeros(0, dtype=np.uint32)
        cl = Cluster(self.catalogs, self.pools, self.nodes, [PodShape(synth.req_res(100, 128))], empty,
                     np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint64), name=name)
        cl.drift_inputs = DriftInputs(self.classes, self.pdrift, self.ndrift)
        return cl, self.want


def reference_suite(lib, catalog):
    """(cluster, want): the reference's own cases, one node each, named by the line of their `It`."""
    cat = types_named(catalog)
    small = types_named(catalog, ("m5.2xlarge", "c5.large"))  # a second catalogue that lacks m5.large
    rows = [r for r in kcatalog.load_ec2_table() if r["name"] in ("m5.large", "m6g.large")]
    windows = kcatalog.build_catalog(lib, rows=rows, ami_family="Windows2022")
    s = Suite([cat, small, windows])
    fake = dict(image_id="ami-fake")
    drift = lambda r, detail=0: (r, ref.OK, detail)
    err = lambda st: (ref.NONE, st, 0)
    # ---- R::806-983 ----
    s.pool("pool-806", nodeclass=-1)
    s.node("L806-no-nodeclass", "pool-806", err(ref.SKIP_NO_NODECLASS))
    s.node("L812-no-nodepool", "pool-gone", err(ref.SKIP_NOT_MANAGED))
    s.node("L812-no-label", "pool-806", err(ref.SKIP_NOT_MANAGED), labels={"karpenter.sh/nodepool": None})
    s.case("L818-ami-invalid", drift(ref.AMI, 0), instance=fake)
    s.case("L828-multiple", drift(ref.NODECLASS), hash="abcdefghijkl",
           instance=dict(image_id="ami-fake", subnet_id="subnet-fake", security_groups=["sg-fake"]))
    s.case("L845-subnet-invalid", drift(ref.SUBNET), instance=dict(subnet_id="subnet-fake"))
    s.case("L854-subnets-empty", err(ref.ERR_NO_SUBNETS), subnets=[])
    s.case("L861-valid", NOT_DRIFTED)
    s.case("L866-sgs-empty", err(ref.ERR_NO_SECURITY_GROUPS), security_groups=[], instance=dict(security_groups=["sg-fake"]))
    s.case("L874-sg-different", drift(ref.SECURITY_GROUP), instance=dict(security_groups=["sg-fake"]))
    s.case("L884-sg-superset", drift(ref.SECURITY_GROUP), instance=dict(security_groups=["sg-fake", "sg-valid"]))
    s.case("L894-sg-subset", drift(ref.SECURITY_GROUP), security_groups=["sg-valid", "sg-fake"])
    s.pool("pool-910", capacity_reservations=["cr-foo"])
    s.node("L910-reservation-selected", "pool-910", NOT_DRIFTED, instance=dict(capacity_reservation_id="cr-foo"))
    s.node("L910-reservation-gone", "pool-910", drift(ref.CAPACITY_RESERVATION), instance=dict(capacity_reservation_id="cr-bar"))
    s.node("L910-no-reservation", "pool-910", NOT_DRIFTED)
    s.case("L941-sgs-match", NOT_DRIFTED, security_groups=["sg-b", "sg-a", "sg-b"],
           instance=dict(security_groups=["sg-a", "sg-a", "sg-b"]))
    # :946 the NodeClaim names no type of the pool: here a type that the pool's catalogue lacks
    s.pool("pool-946", catalog=1)
    s.node("L946-type-unknown", "pool-946", err(ref.ERR_INSTANCE_TYPE))
    s.node("L946-type-by-name", "pool-946", NOT_DRIFTED, type_name="c5.large")
    s.case("L951-no-provider-id", err(ref.ERR_INSTANCE), instance=None)
    s.case("L957-no-instance", err(ref.ERR_INSTANCE), instance=None)
    s.case("L964-ami-other-arch", drift(ref.AMI, 0), amis=[AMD], instance=dict(image_id="ami-arm64"))
    s.case("L964-ami-none", drift(ref.AMI, ref.NO_AMI), amis=[AMD], type_name="m6g.large", instance=dict(image_id="ami-arm64"))
    s.case("drift-go-88-no-amis", err(ref.ERR_NO_AMIS), amis=[])  # R:pkg/cloudprovider/drift.go:88-90, no `It` of its own
    # ---- R::984-1190 static drift: the hashes are inputs, so every entry of the first table is "the hash changed" ----
    s.case("L1063-static-changed", drift(ref.NODECLASS), hash="class-hash-2")
    for entry in ("ami", "subnet", "sg"):  # :1109-1130 only the spec's dynamic fields change: the hash does not
        s.case("L1109-dynamic-" + entry, NOT_DRIFTED)
    s.case("L1131-claim-hash-absent", NOT_DRIFTED, hash="class-hash-2", ann=dict(nodeclass_hash=None))
    s.case("L1143-version-mismatch", NOT_DRIFTED, hash="class-hash-2", hash_version="v2")
    s.case("L1157-class-version-absent", NOT_DRIFTED, hash="class-hash-2", hash_version=None)
    s.case("L1174-claim-version-absent", NOT_DRIFTED, hash="class-hash-2", ann=dict(nodeclass_hash_version=None))
    s.case("static-class-hash-absent", NOT_DRIFTED, hash=None)
    # ---- R:website/content/en/preview/concepts/disruption.md:135 ----
    s.case("docs-widened", NOT_DRIFTED, requirements=[(ITYPE, "In", ["m5.large", "m5.2xlarge"])])
    s.case("docs-narrowed", drift(ref.REQUIREMENTS, 0), requirements=[(ITYPE, "In", ["m5.2xlarge"])])
    # ---- the AMI variants on real types, both list orders: the first compatible wins ----
    for order, amis in (("special-first", [NVIDIA, NEURON, STANDARD]), ("standard-first", [STANDARD, NEURON, NVIDIA])):
        p = s.pool("pool-variants-" + order, amis=amis)
        for type_name in ("m5.large", "g4dn.xlarge", "inf2.xlarge"):
            variant = {"m5.large": STANDARD, "g4dn.xlarge": NVIDIA, "inf2.xlarge": NEURON}[type_name]
            i = amis.index(variant)
            s.node(f"variant-{order}-{type_name}", p, NOT_DRIFTED, type_name, instance=dict(image_id=variant.id))
            s.node(f"variant-{order}-{type_name}-stale", p, drift(ref.AMI, i), type_name, instance=dict(image_id="ami-amd64"))
    p = s.pool("pool-no-standard", amis=[NVIDIA, NEURON])
    s.node("variant-none-for-m5", p, drift(ref.AMI, ref.NO_AMI), instance=dict(image_id="ami-nvidia"))
    # ---- the Windows pair: types of a Windows2022 catalogue ----
    p = s.pool("pool-windows", catalog=2, amis=[WIN2019, WIN2022])
    s.node("windows-2022", p, NOT_DRIFTED, catalog=2, instance=dict(image_id="ami-win2022"))
    s.node("windows-2019-image", p, drift(ref.AMI, 1), catalog=2, instance=dict(image_id="ami-win2019"))
    s.node("windows-arm64-no-os", p, drift(ref.AMI, ref.NO_AMI), "m6g.large", catalog=2, instance=dict(image_id="ami-win2022"))
    p = s.pool("pool-linux-amis-windows-types", catalog=2)
    s.node("windows-type-linux-ami", p, NOT_DRIFTED, catalog=2)  # the base AMIs constrain the architecture only
    return s.build("driftdet-reference-suite")


def precedence(catalog):
    """(cluster, want): one node per adjacent pair of the ladder carrying both, and the errors against the reasons."""
    s = Suite([types_named(catalog), types_named(catalog, ("m5.2xlarge", "c5.large"))])
    drift = lambda r, detail=0: (r, ref.OK, detail)
    err = lambda st: (ref.NONE, st, 0)
    narrowed = [(ZONE, "Exists", []), (ITYPE, "In", ["m5.2xlarge"])]
    s.case("nodepool-over-requirements", drift(ref.NODEPOOL), requirements=narrowed, ann=dict(nodepool_hash="old"))
    s.case("requirements-over-nodeclass", drift(ref.REQUIREMENTS, 1), requirements=narrowed, hash="class-hash-2")
    s.case("nodeclass-over-ami", drift(ref.NODECLASS), hash="class-hash-2", instance=dict(image_id="ami-fake"))
    s.case("ami-over-sg", drift(ref.AMI, 0), instance=dict(image_id="ami-fake", security_groups=["sg-fake"]))
    s.case("sg-over-subnet", drift(ref.SECURITY_GROUP), instance=dict(security_groups=["sg-fake"], subnet_id="subnet-fake"))
    s.case("subnet-over-reservation", drift(ref.SUBNET), instance=dict(subnet_id="subnet-fake", capacity_reservation_id="cr-x"))
    s.case("reservation-alone", drift(ref.CAPACITY_RESERVATION), instance=dict(capacity_reservation_id="cr-x"))
    # an error wins over an earlier dynamic reason, not over the static ones
    s.case("no-subnets-over-ami", err(ref.ERR_NO_SUBNETS), subnets=[], instance=dict(image_id="ami-fake"))
    s.case("no-sgs-over-ami", err(ref.ERR_NO_SECURITY_GROUPS), security_groups=[], instance=dict(image_id="ami-fake"))
    s.case("nodeclass-over-no-subnets", drift(ref.NODECLASS), subnets=[], hash="class-hash-2")
    s.case("nodepool-over-no-instance", drift(ref.NODEPOOL), instance=None, ann=dict(nodepool_hash="old"))
    s.case("requirements-over-no-instance", drift(ref.REQUIREMENTS, 1), requirements=narrowed, instance=None)
    s.case("nodeclass-over-no-amis", drift(ref.NODECLASS), amis=[], hash="class-hash-2")
    # the errors among themselves, in the order isNodeClassDrifted meets them
    s.pool("pool-small", catalog=1, amis=[])
    s.node("no-instance-over-type", "pool-small", err(ref.ERR_INSTANCE), instance=None)
    s.node("type-over-no-amis", "pool-small", err(ref.ERR_INSTANCE_TYPE))
    s.case("no-amis-over-no-sgs", err(ref.ERR_NO_AMIS), amis=[], security_groups=[])
    s.case("no-sgs-over-no-subnets", err(ref.ERR_NO_SECURITY_GROUPS), security_groups=[], subnets=[])
    # the skips come before everything
    s.pool("pool-unresolved", nodeclass=-1)
    s.node("no-nodeclass-over-nodepool", "pool-unresolved", err(ref.SKIP_NO_NODECLASS), nodepool_hash="old")
    s.node("not-managed-over-all", "pool-gone", err(ref.SKIP_NOT_MANAGED), nodepool_hash="old", instance=None)
    # NodePool hash: as areStaticFieldsDrifted
    s.case("nodepool-claim-hash-absent", NOT_DRIFTED, ann=dict(nodepool_hash=None))
    s.case("nodepool-version-mismatch", NOT_DRIFTED, ann=dict(nodepool_hash="old", nodepool_hash_version="v0"))
    s.pool("pool-no-hash", pool_hash=None)
    s.node("nodepool-pool-hash-absent", "pool-no-hash", NOT_DRIFTED, nodepool_hash="old")
    return s.build("driftdet-precedence")


def requirement_edges(catalog):
    """(cluster, want): requirement drift where a key is listed twice, on Exists / DoesNotExist, on Gt / Lt against a
    label that is no integer, and on a key no node carries. Each pool leads with a requirement every node passes, so
    that detail is not 0 by default."""
    s = Suite([types_named(catalog)])
    bad = lambda i: (ref.REQUIREMENTS, ref.OK, i)
    lead = (ZONE, "Exists", [])

    def pool(name, *reqs):
        return s.pool(name, nodeclass=0 if s.classes else None, requirements=[lead, *reqs])

    p = pool("in-ab-notin-a", ("team", "In", ["a", "b"]), ("team", "NotIn", ["a"]))
    s.node("twice-a", p, bad(1), labels={"team": "a"})
    s.node("twice-b", p, NOT_DRIFTED, labels={"team": "b"})
    s.node("twice-c", p, bad(1), labels={"team": "c"})
    s.node("twice-absent", p, bad(1))                       # In {b} is left: an undefined key is not allowed
    p = pool("gt2-lt8", (ARCH, "In", ["amd64"]), ("example.com/n", "Gt", ["2"]), ("example.com/n", "Lt", ["8"]))
    s.node("bounds-5", p, NOT_DRIFTED, labels={"example.com/n": "5"})
    s.node("bounds-2", p, bad(2), labels={"example.com/n": "2"})
    s.node("bounds-3", p, NOT_DRIFTED, labels={"example.com/n": "3"})
    s.node("bounds-7", p, NOT_DRIFTED, labels={"example.com/n": "7"})
    s.node("bounds-8", p, bad(2), labels={"example.com/n": "8"})
    s.node("bounds-word", p, bad(2), labels={"example.com/n": "five"})
    s.node("bounds-absent", p, bad(2))
    p = pool("gt8-lt2", ("example.com/n", "Gt", ["8"]), ("example.com/n", "Lt", ["2"]))  # empty range: DoesNotExist
    s.node("empty-range-5", p, bad(1), labels={"example.com/n": "5"})
    s.node("empty-range-absent", p, NOT_DRIFTED)
    p = pool("in-a-notin-a", ("team", "In", ["a"]), ("team", "NotIn", ["a"]))            # nothing is left: DoesNotExist
    s.node("nothing-present", p, bad(1), labels={"team": "a"})
    s.node("nothing-other", p, bad(1), labels={"team": "b"})
    s.node("nothing-absent", p, NOT_DRIFTED)
    p = pool("exists", ("team", "Exists", []))
    s.node("exists-has", p, NOT_DRIFTED, labels={"team": ""})
    s.node("exists-lacks", p, bad(1))
    p = pool("does-not-exist", ("team", "DoesNotExist", []))
    s.node("dne-has", p, bad(1), labels={"team": "a"})
    s.node("dne-lacks", p, NOT_DRIFTED)
    p = pool("gt-word", (K + "instance-cpu", "Gt", ["1"]))
    s.node("gt-integer", p, NOT_DRIFTED)                                                  # m5.large: instance-cpu 2
    s.node("gt-not-integer", p, bad(1), labels={K + "instance-cpu": "two"})
    p = pool("custom-in", ("example.com/nobody", "In", ["x"]))
    s.node("custom-in-absent", p, bad(1))
    p = pool("custom-notin", ("example.com/nobody", "NotIn", ["x"]))
    s.node("custom-notin-absent", p, NOT_DRIFTED)
    p = pool("well-known-absent", (K + "instance-gpu-name", "In", ["t4"]))                # well-known, still not allowed
    s.node("well-known-undefined", p, bad(1))
    p = pool("old-key", ("beta.kubernetes.io/arch", "In", ["arm64"]))                     # normalized to kubernetes.io/arch
    s.node("normalized-key", p, bad(1))
    p = pool("two-failing", ("team", "In", ["a"]), (ARCH, "In", ["arm64"]))
    s.node("first-failing-wins", p, bad(1))
    s.node("second-failing", p, bad(2), labels={"team": "a"})
    return s.build("driftdet-requirement-edges")


# ---- the device's size edges ---------------------------------------------------------------------------------------
def node_counts(catalog, n):
    """(cluster, want): n nodes of one pool, every third with a stale image, every fifth with a foreign subnet"""
    s = Suite([types_named(catalog)])
    s.pool("default")
    for i in range(n):
        inst, want = {}, NOT_DRIFTED
        if i % 5 == 4:
            inst, want = dict(subnet_id="subnet-fake"), (ref.SUBNET, ref.OK, 0)
        if i % 3 == 2:
            inst, want = dict(inst, image_id="ami-stale"), (ref.AMI, ref.OK, 0)
        s.node(f"n{i:04d}", "default", want, instance=inst)
    return s.build(f"driftdet-{n}-nodes")


def ami_lists(catalog):
    """(cluster, want): AMI lists of 1, 63, 64, 65 and 129 with the first compatible AMI (for an m5.large) at index 0,
    63, 64 and last, and with none compatible; an arm64 filler pads the list, and a second compatible AMI behind the
    first shows that the lowest wins."""
    s = Suite([types_named(catalog)])
    filler = lambda i: AMI(f"ami-filler-{i}", [(ARCH, "In", ["arm64"])])
    for n in (1, 63, 64, 65, 129):
        for at in sorted({0, 63, 64, n - 1}):
            if at >= n:
                continue
            amis = [filler(i) for i in range(n)]
            amis[at] = AMI("ami-first", [(ARCH, "In", ["amd64"])])
            if at + 1 < n:
                amis[-1] = AMI("ami-later", [(ARCH, "NotIn", ["arm64"])])
            p = s.pool(f"pool-{n}-{at}", amis=amis)
            s.node(f"amis-{n}-at-{at}", p, NOT_DRIFTED, instance=dict(image_id="ami-first"))
            s.node(f"amis-{n}-at-{at}-later", p, (ref.AMI, ref.OK, at), instance=dict(image_id="ami-later"))
            s.node(f"amis-{n}-at-{at}-arm", p, (ref.AMI, ref.OK, 0 if at else (1 if n > 1 else ref.NO_AMI)), "m6g.large",
                   instance=dict(image_id="ami-first"))
        p = s.pool(f"pool-{n}-none", amis=[filler(i) for i in range(n)])
        s.node(f"amis-{n}-none", p, (ref.AMI, ref.OK, ref.NO_AMI), instance=dict(image_id="ami-filler-0"))
    return s.build("driftdet-ami-lists")


def value_dictionaries(catalog):
    """(cluster, want): a key whose value dictionary holds 63, 64, 65 and 129 distinct values over the nodes, the
    pool admitting the value whose id sits at a word boundary (0, 63, 64, 127, 128, last) and no other."""
    s = Suite([types_named(catalog)])
    nc = s.nodeclass()
    for n in (63, 64, 65, 129):
        key = f"example.com/v{n}"
        # first the nodes that give the dictionary its size, in value order (ids follow first appearance), under a
        # pool that refuses one value
        p = s.pool(f"pool-{n}-fill", nodeclass=nc, requirements=[(key, "NotIn", [f"value-{n - 1}"])])
        for v in range(n):
            s.node(f"dict-{n}-fill-{v}", p, NOT_DRIFTED if v != n - 1 else (ref.REQUIREMENTS, ref.OK, 0),
                   labels={key: f"value-{v}"})
        for at in sorted({0, 63, 64, 127, 128, n - 1}):
            if at >= n:
                continue
            p = s.pool(f"pool-{n}-{at}", nodeclass=nc, requirements=[(ZONE, "Exists", []), (key, "In", [f"value-{at}", "unseen"])])
            for v in {0, at - 1, at, at + 1, n - 1}:
                if 0 <= v < n:
                    s.node(f"dict-{n}-{at}-v{v}", p, NOT_DRIFTED if v == at else (ref.REQUIREMENTS, ref.OK, 1),
                           labels={key: f"value-{v}"})
    return s.build("driftdet-value-dictionaries")


def id_sets(catalog):
    """(cluster, want): security-group sets of 1, 2 and 17 ids with duplicates, permuted, as a subset and as a
    superset; subnets of 1 and 65 ids with the instance's first, last and absent."""
    s = Suite([types_named(catalog)])
    sgd = (ref.SECURITY_GROUP, ref.OK, 0)
    for n in (1, 2, 17):
        ids = [f"sg-{i:02d}" for i in range(n)]
        p = s.pool(f"pool-sg-{n}", security_groups=ids + ids[:1])
        s.node(f"sg-{n}-same", p, NOT_DRIFTED, instance=dict(security_groups=list(ids)))
        s.node(f"sg-{n}-permuted-dup", p, NOT_DRIFTED, instance=dict(security_groups=ids[::-1] + ids[-1:] + ids[:1]))
        s.node(f"sg-{n}-superset", p, sgd, instance=dict(security_groups=ids + ["sg-zz"]))
        s.node(f"sg-{n}-subset", p, sgd, instance=dict(security_groups=ids[1:]))
        s.node(f"sg-{n}-one-different", p, sgd, instance=dict(security_groups=ids[:-1] + ["sg-zz"]))
    for n in (1, 65):
        ids = [f"subnet-{i:02d}" for i in range(n)]
        p = s.pool(f"pool-subnet-{n}", subnets=ids[::-1])
        s.node(f"subnet-{n}-first", p, NOT_DRIFTED, instance=dict(subnet_id=ids[0]))
        s.node(f"subnet-{n}-last", p, NOT_DRIFTED, instance=dict(subnet_id=ids[-1]))
        s.node(f"subnet-{n}-absent", p, (ref.SUBNET, ref.OK, 0), instance=dict(subnet_id="subnet-zz"))
    return s.build("driftdet-id-sets")


def pools_and_classes(catalog, n_pools, n_classes):
    """(cluster, want): n_pools pools sharing n_classes nodeclasses (class c publishes image ami-c), two nodes per pool:
    one launched from its class's image, one from the next class's."""
    s = Suite([types_named(catalog)])
    for c in range(n_classes):
        s.nodeclass(amis=[AMI(f"ami-{c}", [(ARCH, "In", ["amd64"])])], hash=f"class-hash-{c}")
    for p in range(n_pools):
        c = p % n_classes
        name = s.pool(f"pool-{p:03d}", nodeclass=c)
        s.node(f"p{p:03d}-own", name, NOT_DRIFTED, instance=dict(image_id=f"ami-{c}"), nodeclass_hash=f"class-hash-{c}")
        other = (c + 1) % n_classes
        s.node(f"p{p:03d}-other", name, NOT_DRIFTED if other == c else (ref.AMI, ref.OK, 0),
               instance=dict(image_id=f"ami-{other}"), nodeclass_hash=f"class-hash-{c}")
    return s.build(f"driftdet-{n_pools}-pools-{n_classes}-classes")


def random_cluster(catalog, seed, n_nodes=120, n_pools=12):
    """A randomized cluster with add_drift_inputs: synth.random_cluster's nodes over n_pools pools, the last of the
    regular pools moved to a second catalogue that holds every other type (its nodes keep their own catalogue: half of
    them run a type their pool does not offer), a few nodes without a NodePool, and the generator's error pools."""
    cl = synth.random_cluster(catalog, seed, n_nodes=n_nodes, n_pools=n_pools)
    cl.catalogs.append(cl.catalogs[0][::2])
    cl.nodepools[n_pools - 5].catalog = 1
    for p in cl.nodepools[::3]:   # a third of the pools constrain nothing: their nodes drift by the other reasons only
        p.requirements = []
    for i, n in enumerate(cl.nodes):  # a few nodes nothing manages
        if i % 17 == 16:
            del n.node.labels["karpenter.sh/nodepool"]
        elif i % 19 == 18:
            n.node.labels["karpenter.sh/nodepool"] = "pool-gone"
    synth.add_drift_inputs(cl, seed)
    return cl
