"""kp_catalog_compile on the device with == on every field, present masks included: against the docs'
allocatable table, against the host's kp_instance_type_resolve / kp_instance_type_overhead and the oracle over a matrix
of NodeClasses, against build_catalog, and against the plain-Python rule (tests/catcomp_ref.py, held to hand-written
cases on the CPU by tests/test_catcomp_ref.py) at the smallest shapes where the kernels can go wrong."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import catcomp_ref as ref  # noqa: E402
from kpamd import abi, catalog  # noqa: E402
from kpamd.catalog import CapacityReservation as CR  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GOLD_NAMES = ["cpu", "memory", "ephemeral-storage", "pods", "vpc.amazonaws.com/pod-eni", "vpc.amazonaws.com/efa",
              "nvidia.com/gpu", "amd.com/gpu", "aws.amazon.com/neuron", "aws.amazon.com/neuroncore", "habana.ai/gaudi"]
GI = 1 << 30

# The NodeClasses the device is held to the host on: every AMI family's flags, the pod-density knobs, the kubelet
# overrides, each eviction form, and every way ephemeralStorage picks its volume.
MATRIX = {
    "al2023": dict(),
    "al2": dict(ami_family="AL2"),
    "bottlerocket": dict(ami_family="Bottlerocket"),
    "windows2022": dict(ami_family="Windows2022"),
    "custom": dict(ami_family="Custom"),
    "max_pods_110": dict(max_pods=110),
    "pods_per_core_4": dict(pods_per_core=4),
    "pods_per_core_not_honoured": dict(pods_per_core=4, ami_family="Bottlerocket"),
    "max_pods_and_pods_per_core": dict(max_pods=110, pods_per_core=4, ami_family="Windows2022"),
    "reserved_overrides": dict(kubelet_cfg=dict(kube_reserved={"cpu": "200m", "memory": "1Gi", "pods": "3"},
                                                system_reserved={"cpu": "100m", "memory": "200Mi",
                                                                 "ephemeral-storage": "1Gi"})),
    "hard_memory_5pct": dict(kubelet_cfg=dict(eviction_hard={"memory.available": "5%"})),
    "hard_memory_12_5pct": dict(kubelet_cfg=dict(eviction_hard={"memory.available": "12.5%"})),
    "hard_memory_100pct": dict(kubelet_cfg=dict(eviction_hard={"memory.available": "100%"})),
    "hard_nodefs_10pct": dict(kubelet_cfg=dict(eviction_hard={"nodefs.available": "10%"})),
    "hard_quantities": dict(kubelet_cfg=dict(eviction_hard={"memory.available": "500Mi", "nodefs.available": "3Gi"})),
    "hard_empty_map": dict(kubelet_cfg=dict(eviction_hard={})),
    "soft_honoured": dict(kubelet_cfg=dict(eviction_hard={"memory.available": "5%"},
                                           eviction_soft={"memory.available": "12.5%", "nodefs.available": "15%"})),
    "soft_below_hard": dict(ami_family="AL2", kubelet_cfg=dict(eviction_hard={"memory.available": "1Gi"},
                                                                eviction_soft={"memory.available": "200Mi"})),
    "soft_not_honoured": dict(ami_family="Bottlerocket",
                              kubelet_cfg=dict(eviction_soft={"memory.available": "12.5%", "nodefs.available": "15%"})),
    "root_volume_bdm": dict(block_device_mappings=[("/dev/xvdb", 100 * GI, True), ("/dev/xvda", 40 * GI, False)]),
    "family_device_bdm": dict(block_device_mappings=[("/dev/sdf", 7 * GI, False), ("/dev/xvda", 40 * GI + 1, False)]),
    "bottlerocket_device_bdm": dict(ami_family="Bottlerocket",
                                    block_device_mappings=[("/dev/xvda", 4 * GI, False), ("/dev/xvdb", 33 * GI, False)]),
    "custom_bdms": dict(ami_family="Custom", block_device_mappings=[("/dev/sda", 30 * GI, False), ("/dev/sdb", 61 * GI, False)]),
    "custom_bdm_without_size": dict(ami_family="Custom", block_device_mappings=[("/dev/sda", 30 * GI, False), ("/dev/sdb", None, False)]),
    "raid0": dict(instance_store_policy="RAID0"),
    "raid0_with_root_bdm": dict(instance_store_policy="RAID0", block_device_mappings=[("/dev/xvda", 77 * GI, True)],
                                kubelet_cfg=dict(eviction_hard={"nodefs.available": "12.5%"})),
}
# reserved_enis large enough that the usable ENIs reach 0 (an option of the call, not of a NodeClass)
RESERVED_ENIS = ("al2023", "bottlerocket", "windows2022", "max_pods_110")


@pytest.fixture(scope="module")
def rows():
    rows = catalog.load_ec2_table()
    assert len(rows) == 919
    nvme = [int(r["local_nvme_gb"] or 0) > 0 for r in rows]
    assert any(nvme) and not all(nvme)  # RAID0 on types with and without an instance store
    return rows


def host_lists(lib, rows, nodeclasses, opts):
    """the five lists from kp_instance_type_resolve / kp_instance_type_overhead, one (NodeClass, type) pair per call"""
    arena = abi.Arena()
    infos = [catalog.ec2_info(arena, r) for r in rows]
    out = {k: np.zeros((len(nodeclasses), len(rows)), dtype=abi.resource_list_dtype()) for k in abi.COMPILE_LISTS}
    lists = [abi.ResourceList() for _ in abi.COMPILE_LISTS]
    for n, kw in enumerate(nodeclasses):
        nc = catalog.nodeclass(arena, **kw)
        for t, info in enumerate(infos):
            assert lib.kp_instance_type_resolve(C.byref(opts), C.byref(info), C.byref(nc), C.byref(lists[0]), C.byref(lists[1])) == 0
            assert lib.kp_instance_type_overhead(C.byref(opts), C.byref(info), C.byref(nc), *(C.byref(l) for l in lists[2:])) == 0
            for k, l in zip(abi.COMPILE_LISTS, lists):
                out[k][n, t] = np.frombuffer(bytes(l), dtype=abi.resource_list_dtype())[0]
    return out


def assert_tables_equal(got, want, keys, name=""):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (name, k)
        if got[k].dtype.names:
            for f in got[k].dtype.names:
                bad = np.argwhere(got[k][f] != want[k][f])
                assert not len(bad), (name, k, f, bad[:5].tolist())
        elif got[k].dtype.kind == "f":
            bad = np.argwhere(got[k].view(np.uint64) != want[k].view(np.uint64))  # the bits
            assert not len(bad), (name, k, bad[:5].tolist())
        else:
            bad = np.argwhere(got[k] != want[k])
            assert not len(bad), (name, k, bad[:5].tolist())


def test_allocatable_matches_the_docs(ctx, rows):
    """capacity - overhead of the default AL2023 NodeClass is the docs' allocatable table for all 919 types"""
    drift = {l.strip() for l in open(os.path.join(GOLD, "docs_pod_eni_drift.txt")) if l.strip() and not l.startswith("#")}
    gold = {}
    for line in open(os.path.join(GOLD, "docs_allocatable.tsv")):
        if not (line.startswith("#") or line.startswith("name")):
            p = line.rstrip("\n").split("\t")
            gold[p[0]] = [int(x) for x in p[1:]]
    tab = ctx.compile_catalogs(rows, [dict()], outputs=("capacity", "overhead"))
    cap, ovh = tab["capacity"][0], tab["overhead"][0]
    assert (cap["present"] == 0x7FF).all()
    assert (ovh["present"] == 0b111).all()  # cpu, memory, ephemeral-storage
    bad = []
    for t, r in enumerate(rows):
        for n in GOLD_NAMES:
            i = abi.RES_INDEX[n]
            if n == "vpc.amazonaws.com/pod-eni" and r["name"] in drift:
                continue
            have = int(cap["milli"][t, i]) - (int(ovh["milli"][t, i]) if ovh["present"][t] >> i & 1 else 0)
            if have != gold[r["name"]][GOLD_NAMES.index(n)]:
                bad.append((r["name"], n, have, gold[r["name"]][GOLD_NAMES.index(n)]))
    assert not bad, bad[:10]


@pytest.fixture(scope="module")
def matrix_tables(ctx, rows):
    return ctx.compile_catalogs(rows, list(MATRIX.values()), outputs=abi.COMPILE_LISTS)


def test_matrix_equals_the_host(ctx, lib, rows, matrix_tables):
    assert_tables_equal(matrix_tables, host_lists(lib, rows, list(MATRIX.values()), ctx.opts), abi.COMPILE_LISTS)
    # the matrix reaches what it is meant to reach
    cap, ev = matrix_tables["capacity"], matrix_tables["eviction_threshold"]
    names = list(MATRIX)
    eph, mem, pods = abi.RES_INDEX["ephemeral-storage"], abi.RES_INDEX["memory"], abi.RES_INDEX["pods"]
    nvme = np.array([int(r["local_nvme_gb"] or 0) > 0 for r in rows])
    raid, plain = cap["milli"][names.index("raid0"), :, eph], cap["milli"][names.index("al2023"), :, eph]
    assert (raid[nvme] != plain[nvme]).all() and (raid[~nvme] == plain[~nvme]).all()
    assert (cap["present"][names.index("windows2022")] != cap["present"][names.index("al2023")]).any()
    assert (ev["milli"][names.index("hard_memory_100pct"), :, mem] == 0).all()
    assert (ev["milli"][names.index("soft_honoured"), :, mem] > ev["milli"][names.index("hard_memory_5pct"), :, mem]).all()
    assert (ev["milli"][names.index("soft_not_honoured")] == ev["milli"][names.index("bottlerocket")]).all()
    assert (cap["milli"][names.index("pods_per_core_not_honoured"), :, pods] == cap["milli"][names.index("bottlerocket"), :, pods]).all()


def test_matrix_equals_the_oracle(rows, matrix_tables):
    assert_tables_equal(matrix_tables, ref.resource_lists(rows, list(MATRIX.values())), abi.COMPILE_LISTS)


def test_reserved_enis_until_no_eni_is_usable(ctx, lib, rows):
    opts = abi.Options(0.075, 100, 0)
    ncs = [MATRIX[k] for k in RESERVED_ENIS]
    got = ctx.compile_catalogs(rows, ncs, outputs=abi.COMPILE_LISTS, opts=opts)
    assert_tables_equal(got, host_lists(lib, rows, ncs, opts), abi.COMPILE_LISTS)
    assert_tables_equal(got, ref.resource_lists(rows, ncs, opts), abi.COMPILE_LISTS)
    assert (got["capacity"]["milli"][0, :, abi.RES_INDEX["pods"]] == 0).all()
    opts = abi.Options(0.075, 3, 0)  # some types keep a usable ENI, some do not
    got = ctx.compile_catalogs(rows, ncs, outputs=abi.COMPILE_LISTS, opts=opts)
    assert_tables_equal(got, host_lists(lib, rows, ncs, opts), abi.COMPILE_LISTS)
    p = got["capacity"]["milli"][0, :, abi.RES_INDEX["pods"]]
    assert (p == 0).any() and (p > 0).any()


def test_build_catalogs_equals_build_catalog(ctx, lib, rows):
    """the whole InstanceType lists: requirements, capacity, overhead and every offering"""
    crs = [CR("cr-1", rows[3]["name"], catalog.ZONES[0], "default", 3),
           CR("cr-2", rows[3]["name"], catalog.ZONES[2], "capacity-block", 0), CR("cr-3", rows[918]["name"], catalog.ZONES[1])]
    unavailable = frozenset({("spot", rows[5]["name"], catalog.ZONES[1]), ("on-demand", rows[64]["name"], catalog.ZONES[0])})
    ncs = [dict(kw) for kw in MATRIX.values()]
    ncs[1]["capacity_reservations"] = crs
    ncs[2]["capacity_reservations"] = crs[:1]
    ncs[3]["zones"], ncs[3]["zone_ids"] = catalog.ZONES[1:], catalog.ZONE_IDS[1:]
    got = catalog.build_catalogs(ctx, ncs, rows=rows, unavailable=unavailable)
    assert len(got) == len(ncs)
    for name, kw, its in zip(MATRIX, ncs, got):
        if "zones" in kw:
            continue  # build_catalog iterates the subnet zones: compared below
        want = catalog.build_catalog(lib, rows=rows, unavailable=unavailable, **kw)
        assert its == want, name
    # a NodeClass on two of the three zones: what build_catalog gives for those zones, plus, for the third zone,
    # offerings that are never available and have no zone id
    kw = dict(ncs[3])
    want = catalog.build_catalog(lib, rows=rows, unavailable=unavailable, **kw)
    spot3 = catalog.default_spot_prices(rows)
    for a, b, r in zip(got[3], want, rows):
        assert (a.name, a.requirements, a.capacity, a.overhead) == (b.name, b.requirements, b.capacity, b.overhead)
        assert [(o.capacity_type, o.zone, o.zone_id, o.available) for o in a.offerings[2:]] == \
            [(o.capacity_type, o.zone, o.zone_id, o.available) for o in b.offerings]
        od = r["od_price"] if r["od_price"] >= 0 else 0.0
        assert [(o.zone, o.zone_id, o.price, o.available) for o in a.offerings[:2]] == \
            [(catalog.ZONES[0], None, od, False), (catalog.ZONES[0], None, spot3.get((r["name"], catalog.ZONES[0]), 0.0), False)]


# ---- size edges: tests/catcomp_ref.py is the reference ---------------------------------------------------------------
def edge_rows(rows, n_types, last):
    """n_types rows whose last one is the only arm64 type, or the only type without a price"""
    plain = [r for r in rows if r["arch"] == "amd64" and r["od_price"] >= 0]
    if last == "arm64":
        odd = next(r for r in rows if r["arch"] == "arm64" and r["od_price"] >= 0)
    else:
        odd = next(r for r in rows if r["arch"] == "amd64" and r["od_price"] < 0)
    if n_types - 1 > len(plain):  # the whole table: the odd one is no longer the only one, but still in the last lane
        plain = [r for r in rows if r is not odd]
    return plain[:n_types - 1] + [odd]


def edge_case(rows, n_types, n_nodeclasses, n_zones, last):
    sub = edge_rows(rows, n_types, last)
    zones = [f"zone-{z}" for z in range(n_zones)]
    ids = [f"id-{z}" for z in range(n_zones)]
    g = catalog.SplitMix64(n_types * 1000 + n_zones)
    full = (1 << n_zones) - 1
    type_zones = [g.next() & full for _ in sub]
    type_zones[0] = full
    type_zones[-1] = full  # the last lane is offered everywhere: its arm64 / missing price is what decides
    if n_types > 2:
        type_zones[1] = 0
    ncs = []
    for n in range(n_nodeclasses):
        pick = [z for z in range(n_zones) if (z + n) % (n + 1) == 0] or [0]
        kw = dict(list(MATRIX.values())[(n * 5) % len(MATRIX)])
        kw.update(zones=[zones[z] for z in pick] + ["zone-elsewhere"], zone_ids=[ids[z] for z in pick] + ["id-elsewhere"])
        ncs.append(kw)
    if n_nodeclasses > 1:
        ncs[-1].update(zones=["zone-elsewhere"], zone_ids=["id-elsewhere"])  # shares no zone with any type
    spot = {(r["name"], z): 0.25 + 0.001 * i + 0.01 * j for i, r in enumerate(sub) for j, z in enumerate(zones)
            if r["od_price"] >= 0 and (i + j) % 5 != 4}
    last_name, first_name = sub[-1]["name"], sub[0]["name"]
    unavailable = {("spot", last_name, zones[-1]), ("on-demand", first_name, zones[0])}
    if n_zones > 1:
        unavailable.add(zones[n_zones // 2])
    if n_zones > 2:
        unavailable.add("spot" if n_types % 2 else "on-demand")
    reservations = [[] for _ in ncs]
    reservations[0] = [CR("cr-a", last_name, zones[0], "default", 2), CR("cr-b", last_name, zones[-1], "default", 0),
                       CR("cr-c", first_name, zones[0], "capacity-block", 7)]
    if n_nodeclasses > 1:
        reservations[1] = [CR("cr-a", last_name, zones[0], "default", 2)]   # two NodeClasses on one type
        reservations[-1].append(CR("cr-d", first_name, zones[0], "default", 1))
    discovered = {(n_nodeclasses - 1, last_name): 123456789012}
    return dict(rows=sub, nodeclasses=ncs, all_zones=zones, type_zones=type_zones, spot_prices=spot, unavailable=unavailable,
                reservations=reservations, discovered_memory=discovered)


EDGES = [(1, 1, 1), (63, 2, 63), (64, 7, 64), (65, 2, 1), (919, 7, 3), (65, 1, 64)]


@pytest.mark.parametrize("last", ["arm64", "unpriced"])
@pytest.mark.parametrize("n_types,n_nodeclasses,n_zones", EDGES)
def test_size_edges(ctx, rows, n_types, n_nodeclasses, n_zones, last):
    case = edge_case(rows, n_types, n_nodeclasses, n_zones, last)
    sub = case.pop("rows")
    ncs = case.pop("nodeclasses")
    assert len(sub) == n_types and len(ncs) == n_nodeclasses
    want = ref.compile_catalogs(sub, ncs, **case)
    got = ctx.compile_catalogs(sub, ncs, **case)
    assert_tables_equal(got, want, abi.COMPILE_OUTPUTS, (n_types, n_nodeclasses, n_zones, last))
    assert got["stats"]["device_ms"] >= 0 and got["stats"]["host_ms"] > 0
    if n_nodeclasses > 1:
        assert (got["it_zones"][-1] == 0).all() and (got["available"][-1] == 0).all()
    if last == "unpriced":
        assert (got["price"][-1] == 0).all() and (got["available"][:, -1] == 0).all()
        assert (got["available"][0, 0] != 0).any() or n_zones == 1
    mem = abi.RES_INDEX["memory"]
    assert got["capacity"]["milli"][-1, -1, mem] == 123456789012 * 1000
    assert len(got["reserved"]) == sum(len(x) for x in case["reservations"])


def small(rows):
    sub = edge_rows(rows, 65, "unpriced")
    ncs = [dict(), dict(zones=catalog.ZONES[:2], zone_ids=catalog.ZONE_IDS[:2], max_pods=20)]
    return sub, ncs


@pytest.mark.parametrize("unavailable", [[("spot", 64, 0)], [("on-demand", 0, 2), ("spot", 63, 1)], ["spot"], ["on-demand"],
                                         [1], [("spot", 64, 0), "on-demand", 1]],
                         ids=["triple", "triples", "spot", "on-demand", "zone", "all"])
def test_unavailable_kinds(ctx, rows, unavailable):
    sub, ncs = small(rows)
    sub[64] = next(r for r in rows if r["arch"] == "arm64" and r["od_price"] >= 0)  # (every type priced)
    unav = [(u[0], sub[u[1]]["name"], catalog.ZONES[u[2]]) if isinstance(u, tuple) else
            catalog.ZONES[u] if isinstance(u, int) else u for u in unavailable]
    keys = ("it_zones", "price", "available")
    got = ctx.compile_catalogs(sub, ncs, unavailable=unav, outputs=keys)
    assert_tables_equal(got, ref.compile_catalogs(sub, ncs, unavailable=unav, lists=False), keys)
    clear = ctx.compile_catalogs(sub, ncs, outputs=keys)
    assert (clear["available"][0] == 0b111).all() and (clear["available"][1] == 0b011).all()
    assert (got["available"] != clear["available"]).any()
    assert_tables_equal(got, clear, ("it_zones", "price"))


def test_no_reservations_and_the_feature_gate(ctx, rows):
    sub, ncs = small(rows)
    got = ctx.compile_catalogs(sub, ncs)
    assert got["reserved"].shape == (0,)
    crs = [[CR("cr-1", sub[1]["name"], catalog.ZONES[2], "default", 4)], [CR("cr-2", sub[1]["name"], catalog.ZONES[2], "default", 4)]]
    on = ctx.compile_catalogs(sub, ncs, reservations=crs)
    assert on["reserved"].tolist() == [(sub[1]["od_price"] / 10_000_000.0, 1, 4), (sub[1]["od_price"] / 10_000_000.0, 0, 4)]
    off = ctx.compile_catalogs(sub, ncs, reservations=crs, reserved_capacity=False)
    assert (off["reserved"]["capacity"] == 0).all()  # not written: the buffer as it was handed in
    assert_tables_equal(off, got, [k for k in abi.COMPILE_OUTPUTS if k != "reserved"])
    assert_tables_equal(on, got, [k for k in abi.COMPILE_OUTPUTS if k != "reserved"])


def test_discovered_memory_of_one_pair_only(ctx, rows):
    sub, ncs = small(rows)
    plain = ctx.compile_catalogs(sub, ncs)
    got = ctx.compile_catalogs(sub, ncs, discovered_memory={(1, sub[64]["name"]): 5 * GI})
    want = {k: v.copy() for k, v in plain.items() if k != "stats"}
    want["capacity"]["milli"][1, 64, abi.RES_INDEX["memory"]] = 5 * GI * 1000
    assert_tables_equal(got, want, abi.COMPILE_OUTPUTS)
    none = ctx.compile_catalogs(sub, ncs, discovered_memory={})  # the table given, every entry negative
    assert_tables_equal(none, plain, abi.COMPILE_OUTPUTS)


def test_each_output_skipped_in_turn(ctx, rows):
    sub, ncs = small(rows)
    args = dict(unavailable=["spot", (("on-demand"), sub[2]["name"], catalog.ZONES[0])],
                reservations=[[CR("cr-1", sub[1]["name"], catalog.ZONES[1], "default", 4)], []],
                discovered_memory={(0, sub[3]["name"]): GI})
    full = ctx.compile_catalogs(sub, ncs, **args)
    assert_tables_equal(full, ref.compile_catalogs(sub, ncs, **args), abi.COMPILE_OUTPUTS)
    for skip in abi.COMPILE_OUTPUTS:
        keep = tuple(k for k in abi.COMPILE_OUTPUTS if k != skip)
        got = ctx.compile_catalogs(sub, ncs, outputs=keep, **args)
        assert skip not in got
        assert_tables_equal(got, full, keep, skip)
    one = ctx.compile_catalogs(sub, ncs, outputs=("price",), **args)
    assert_tables_equal(one, full, ("price",))
