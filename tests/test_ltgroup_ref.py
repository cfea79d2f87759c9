"""The plain-Python reference of the launch-template grouping (tests/ltgroup_ref.py; kp_launch_templates)
held to hand-written expectations that restate the reference suite (R:pkg/providers/launchtemplate/suite_test.go) and
the rule of include/kp/kp_abi.h. CPU only; tests/test_gpu_ltgroup.py compares the device with this reference."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ltgroup_cases as cases  # noqa: E402
import ltgroup_ref as ref  # noqa: E402
from ltgroup_cases import AMD, ARCH, ARM, CT, EFA, K, ZONES  # noqa: E402
from kpamd.model import AMI  # noqa: E402


def one(types, requests, zones, amis, max_types=60):
    out = ref.launch_templates(types, requests, zones, amis, max_types)
    assert len(out) == len(requests)
    return out


def summary(r):
    return [(c["ami"], c["max_pods"], c["efa_count"], c["reservation_id"], c["types"]) for c in r["configs"]]


def test_several_amis_with_non_equivalent_requirements_give_several_templates():
    """suite_test.go:2146: an amd64 and an arm64 AMI, types of both architectures: both images get a template"""
    types = [cases.typ(0), cases.typ(1, arch="arm64"), cases.typ(2)]
    r, = one(types, [cases.request(3)], ZONES, [AMD, ARM])
    assert r["lt_status"] == "OK" and r["types"] == [0, 1, 2] and r["unmapped"] == 0 and r["dropped"] == 0
    assert summary(r) == [("ami-123", 110, 0, None, [0, 2]), ("ami-456", 110, 0, None, [1])]
    assert r["configs"][0]["overrides"] == [(t, z) for t in (0, 2) for z in ZONES]
    assert r["configs"][1]["overrides"] == [(1, z) for z in ZONES]


def test_the_first_compatible_ami_in_status_order_wins():
    """suite_test.go:2175: status.amis is sorted newest first; ami-456 and ami-123 both take amd64 types, ami-789 none"""
    amis = [AMI("ami-456", [(ARCH, "In", ["amd64"])]), AMI("ami-123", [(ARCH, "In", ["amd64"])]),
            AMI("ami-789", [(ARCH, "In", ["arm64"])])]
    types = [cases.typ(i) for i in range(3)]
    r, = one(types, [cases.request(3, [(ARCH, "In", ["amd64"])])], ZONES, amis)
    assert summary(r) == [("ami-456", 110, 0, None, [0, 1, 2])]
    r, = one(types, [cases.request(3)], ZONES, amis[::-1])
    assert summary(r) == [("ami-123", 110, 0, None, [0, 1, 2])]


def test_different_max_pods_values_give_different_templates():
    """suite_test.go:1164: five pod capacities under one image are five templates, not two"""
    pods = [8, 29, 58, 110, 234, 29, 8]
    types = [cases.typ(i, pods=p) for i, p in enumerate(pods)]
    r, = one(types, [cases.request(len(pods))], ZONES, [AMD])
    assert summary(r) == [("ami-123", 8, 0, None, [0, 6]), ("ami-123", 29, 0, None, [1, 5]), ("ami-123", 58, 0, None, [2]),
                          ("ami-123", 110, 0, None, [3]), ("ami-123", 234, 0, None, [4])]
    assert r["configs"][0]["overrides"] == [(t, z) for t in (0, 6) for z in ZONES]


def test_one_template_per_capacity_reservation():
    """suite_test.go:2461: three templates rather than four (of the two reservations of m5.large in 1a only the one
    with the greater capacity launches), one override each, for the reservation's type and zone"""
    r, = one(*cases.reservation_suite())
    assert r["capacity_type"] == "reserved" and r["lt_status"] == "OK" and r["dropped"] == 0
    assert [(c["reservation_id"], c["types"], c["overrides"], c["reservation_type"]) for c in r["configs"]] == [
        ("cr-m5.large-1a-2", [0], [(0, "test-zone-1a")], "default"),
        ("cr-m5.large-1b-1", [0], [(0, "test-zone-1b")], "default"),
        ("cr-m5.xlarge-1b-1", [1], [(1, "test-zone-1b")], "default")]


def test_efa_counts_split_templates_only_when_the_nodeclaim_requests_efa():
    types = cases.efa_types()
    r, = one(types, [cases.request(5)], ZONES, [AMD])
    assert summary(r) == [("ami-123", 110, 0, None, [0, 1, 2, 3, 4])]
    for amount in (1000, 0):  # a present zero counts: Go tests the key of the request list
        r, = one(types, [cases.request(5, resources={"cpu": 1000, EFA: amount})], ZONES, [AMD])
        want = [("ami-123", 110, 0, None, [0, 1]), ("ami-123", 110, 1, None, [2, 3]), ("ami-123", 110, 4, None, [4])]
        assert summary(r) == (want if amount == 0 else want[1:])  # (types without EFA cannot fit a request for one)


def test_unmapped_types_dropped_configs_and_statuses():
    r, = one(*cases.unmapped_at(5, {0, 2, 4}))
    assert r["lt_status"] == "OK" and r["unmapped"] == 3 and summary(r) == [("ami-123", 110, 0, None, [1, 3])]
    r, = one(*cases.unmapped_at(3, {0, 1, 2}))
    assert r["lt_status"] == "NO_COMPATIBLE_AMI" and r["unmapped"] == 3 and r["configs"] == []
    types, requests, zones, _, mt = cases.uniform(3)
    r, = one(types, requests, zones, [], mt)
    assert r["lt_status"] == "NO_AMIS" and r["unmapped"] == 3 and r["status"] == 0 and r["types"] == [0, 1, 2]
    r, = one(types, requests, [], [AMD], mt)
    assert r["lt_status"] == "NO_OFFERINGS" and r["dropped"] == 1 and r["configs"] == [] and r["n_overrides"] == 0
    # a pod capacity offered only in a zone without a subnet: its config is dropped, the other stays
    types = [cases.typ(0), cases.typ(1, pods=29, zones=ZONES[2:])]
    r, = one(types, [cases.request(2)], ZONES[:2], [AMD])
    assert r["lt_status"] == "OK" and r["dropped"] == 1 and summary(r) == [("ami-123", 110, 0, None, [0])]
    out = one(*cases.statuses())
    assert [(x["status"], x["lt_status"]) for x in out] == [(0, "OK"), (1, "SKIPPED"), (2, "SKIPPED"), (1, "SKIPPED"),
                                                             (0, "OK")]
    assert [len(x["configs"]) for x in out] == [2, 0, 0, 0, 2]
    assert summary(out[4]) == [("ami-123", 110, 0, None, [1]), ("ami-123", 29, 0, None, [4])]  # canonical: launch order


def test_reserved_edges():
    out = one(*cases.reserved_edges())
    got = [(x["capacity_type"], x["lt_status"], x["unmapped"], x["dropped"],
            [(c["reservation_id"], c["reservation_type"], c["overrides"]) for c in x["configs"]]) for x in out]
    assert got == [
        ("reserved", "OK", 0, 1, [("cr-a", "default", [(0, "test-zone-1a")])]),          # cr-c: no subnet in 1c
        ("reserved", "OK", 0, 0, [("cr-b", "default", [(1, "test-zone-1b")])]),          # cr-gone is not available
        ("reserved", "OK", 0, 0, [("cr-block-2", "capacity-block", [(2, "test-zone-1b")])]),  # the cheaper block
        ("reserved", "NO_COMPATIBLE_AMI", 1, 0, []),
        ("reserved", "OK", 0, 0, [("cr-p2", "default", [(4, "test-zone-1b")])]),         # pinned by id
        ("reserved", "NO_OFFERINGS", 0, 1, []),
        ("reserved", "OK", 1, 1, [("cr-a", "default", [(0, "test-zone-1a")]), ("cr-b", "default", [(1, "test-zone-1b")]),
                                  ("cr-p1", "default", [(4, "test-zone-1b")])]),
        ("on-demand", "OK", 0, 0, [(None, None, [(0, "test-zone-1a"), (1, "test-zone-1a")])])]


def test_ami_lists_over_mixed_types():
    types = cases.mixed()
    arm = [i for i in range(12) if i % 3 == 2]
    amd = [i for i in range(12) if i % 3 != 2]
    got = {}
    for name, amis in cases.ami_lists():
        r, = one(types, [cases.request(12)], ZONES, amis)
        got[name] = (r["lt_status"], r["unmapped"], {c["ami"]: sorted(t for d in r["configs"] if d["ami"] == c["ami"]
                                                                      for t in d["types"]) for c in r["configs"]})
    assert got["none"] == ("NO_AMIS", 12, {})
    assert got["one"] == ("OK", 4, {"ami-123": amd})
    assert got["two"] == ("OK", 0, {"ami-123": amd, "ami-456": arm})
    fam = lambda f: [i for i in range(12) if i % 4 == f and not (i % 3 == 2 and i % 2)]
    rest = lambda taken, of: [i for i in of if i not in taken]
    taken = [i for f in range(4) for i in fam(f)]
    assert got["nine"] == ("OK", 0, {**{f"ami-{f}": fam(f) for f in range(4)}, "ami-456": rest(taken, arm)})
    assert got["empty-requirements"] == ("OK", 0, {"ami-any": list(range(12))})
    assert got["unknown-value-in"] == ("OK", 0, {"ami-123": amd, "ami-456": arm})
    assert got["unknown-key-in"] == ("OK", 0, {"ami-123": amd, "ami-456": arm})
    assert got["unknown-key-exists"] == ("OK", 4, {"ami-123": amd})
    for name in ("unknown-value-notin", "unknown-key-notin", "unknown-key-dne"):
        assert got[name] == ("OK", 0, {"ami-x": list(range(12))}), name
    nofam = [i for i in range(12) if i % 3 == 2 and i % 2]
    assert got["known-key-dne"] == ("OK", 0, {"ami-x": nofam, "ami-123": amd, "ami-456": rest(nofam, arm)})
    big = [i for i in range(12) if i % 3 == 2]  # instance-cpu 16
    assert got["gt"] == ("OK", 0, {"ami-big": big, "ami-123": rest(big, amd)})
    x = [i for i in arm if i % 4 == 1 and not i % 2]
    assert got["two-keys"] == ("OK", 0, {**({"ami-x": x} if x else {}), "ami-123": amd, "ami-456": rest(x, arm)})


def test_full_catalogue_partitions_by_gpu_amd64_and_arm64_amis(catalog):
    """The 919-type catalogue under a GPU AMI listed first, an amd64 and an arm64 AMI: three sets of types. The request
    carries minValues, which keeps the GPU and metal types in the launch (ExoticInstanceTypeFilter stands down)."""
    amis = [AMI("ami-gpu", [(K + "instance-gpu-count", "Exists", [])]), AMD, ARM]
    reqs = [(CT, "In", ["on-demand"]), (K + "instance-family", "Exists", [], 1)]
    r, = one(catalog, [(reqs, {"cpu": 100, "pods": 1000}, list(range(len(catalog))))], ZONES, amis, max_types=1024)
    sel = set(r["types"])  # (a few types have no on-demand price: CompatibleAvailableFilter drops them)
    assert r["lt_status"] == "OK" and r["unmapped"] == 0 and len(sel) == len(r["types"]) > 900
    by_ami = {}
    for c in r["configs"]:
        by_ami.setdefault(c["ami"], set()).update(c["types"])
    have = lambda it, key: next((q for q in it.requirements if q[0] == key and q[1] == "In"), None)
    gpu = {t for t in sel if have(catalog[t], K + "instance-gpu-count")}
    arch = lambda a: {t for t in sel if have(catalog[t], ARCH)[2] == [a]} - gpu
    assert len(gpu) > 10 and len(arch("arm64")) > 100
    assert by_ami == {"ami-gpu": gpu, "ami-123": arch("amd64"), "ami-456": arch("arm64")}
    assert sum(len(c["types"]) for c in r["configs"]) == len(sel)
    assert len({(c["ami"], c["max_pods"]) for c in r["configs"]}) == len(r["configs"]) > 3
