"""The launch-template grouping on the device (kp_launch_templates, kp_ltgroup.hip) against the plain-Python
reference (tests/ltgroup_ref.py) with == on every field, at the smallest shapes where the kernels can go wrong
(tests/ltgroup_cases.py; tests/test_ltgroup_ref.py holds the reference to hand-written expectations on the CPU)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ltgroup_cases as cases  # noqa: E402
import ltgroup_ref as ref  # noqa: E402
from ltgroup_cases import AMD, ARM, CT, EFA, K, ZONES  # noqa: E402

pytestmark = pytest.mark.gpu


def check(ctx, case):
    """The prepared plan's and the one-shot entry's results equal the reference's; the launch fields equal
    kp_launch_run's on the same plan; the configs of a launch that is not reserved hold kp_launch_run's overrides of
    the types some AMI takes, each once. Returns the results."""
    import kpamd
    types, requests, zones, amis, max_types = case
    want = ref.launch_templates(types, requests, zones, amis, max_types)
    ch = kpamd.Catalog(ctx, types)
    plan = kpamd.LaunchPlan(ctx, ch, requests, zones, max_types=max_types)
    try:
        got, stats = plan.templates(amis)
        flat, _ = plan.run()
        again, _ = plan.templates(amis)  # (the plan's tables are built once; a second run reuses them)
        oneshot = ctx.launch_templates(ch, requests, zones, amis, max_types=max_types)
    finally:
        plan.close()
        ch.close()
    assert len(got) == len(want) == len(requests)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"request {i}: device {g} vs reference {w}"
    assert again == got and oneshot == got
    for i, (g, f) in enumerate(zip(got, flat)):
        assert {k: g[k] for k in f if k != "overrides"} == {k: v for k, v in f.items() if k != "overrides"}, i
        assert g["n_overrides"] == len(f["overrides"])
        if g["status"] == 0 and g["capacity_type"] != "reserved":
            mapped = {t for t in g["types"] if ref.ami_for_type(types[t], amis) is not None}
            assert sorted(o for c in g["configs"] for o in c["overrides"]) == \
                sorted(o for o in f["overrides"] if o[0] in mapped), i
    assert stats["device_ms"] >= 0 and stats["host_ms"] > 0
    return got


@pytest.mark.parametrize("n,max_types", [(1, 60), (59, 60), (60, 60), (61, 60), (130, 64), (130, 65), (130, 130),
                                         (129, 1024)])
def test_selected_type_counts_one_group(ctx, n, max_types):
    """1, 59, 60 selected types, a list one longer than the cut, and the pass boundary at 64 lanes"""
    r, = check(ctx, cases.uniform(n, max_types))
    assert len(r["types"]) == min(n, max_types) and len(r["configs"]) == 1
    assert r["configs"][0]["types"] == r["types"] and len(r["configs"][0]["overrides"]) == 3 * len(r["types"])


@pytest.mark.parametrize("n,max_types", [(1, 60), (60, 60), (130, 64), (130, 65), (130, 130)])
def test_every_type_its_own_group(ctx, n, max_types):
    r, = check(ctx, cases.distinct_pods(n, max_types))
    assert [c["types"] for c in r["configs"]] == [[t] for t in r["types"]] and len(r["types"]) == min(n, max_types)


def test_groups_that_span_passes(ctx):
    """150 types over seven pod capacities and two architectures: every group has members in all three passes"""
    types = [cases.typ(i, arch=["amd64", "arm64"][i % 2], pods=10 * (1 + i % 7)) for i in range(150)]
    r, = check(ctx, (types, [cases.request(150)], ZONES, [ARM, AMD], 150))
    assert len(r["configs"]) == 14 and r["configs"][0]["types"] == list(range(0, 150, 14))


def test_efa(ctx):
    types = cases.efa_types()
    reqs = [cases.request(5), cases.request(5, resources={"cpu": 1000, EFA: 0}),
            cases.request(5, resources={"cpu": 1000, EFA: 1000}), cases.request([0], resources={"cpu": 1000, EFA: 0})]
    got = check(ctx, (types, reqs, ZONES, [AMD], 60))
    assert [[c["efa_count"] for c in r["configs"]] for r in got] == [[0], [0, 1, 4], [1, 4], [0]]


@pytest.mark.parametrize("where", [{0}, {3}, {6}, {0, 6}, set(range(7))], ids=["first", "middle", "last", "ends", "all"])
def test_unmapped_types(ctx, where):
    r, = check(ctx, cases.unmapped_at(7, where))
    assert r["unmapped"] == len(where) and r["lt_status"] == ("NO_COMPATIBLE_AMI" if len(where) == 7 else "OK")


def test_unmapped_past_the_first_pass(ctx):
    r, = check(ctx, cases.unmapped_at(70, {0, 63, 64, 69})[:4] + (70,))
    assert r["unmapped"] == 4 and len(r["configs"]) == 1 and len(r["configs"][0]["types"]) == 66


@pytest.mark.parametrize("name,amis", cases.ami_lists(), ids=[n for n, _ in cases.ami_lists()])
def test_ami_lists(ctx, name, amis):
    check(ctx, (cases.mixed(), [cases.request(12), cases.request([11, 2, 5])], ZONES, amis, 60))


def test_subnets(ctx):
    types = [cases.typ(0), cases.typ(1, pods=29, zones=ZONES[2:]), cases.typ(2, zones=ZONES[1:])]
    r, = check(ctx, (types, [cases.request(3)], [], [AMD], 60))
    assert r["lt_status"] == "NO_OFFERINGS" and r["dropped"] == 2
    r, = check(ctx, (types, [cases.request(3)], ZONES[:2], [AMD], 60))
    assert r["lt_status"] == "OK" and r["dropped"] == 1 and [c["types"] for c in r["configs"]] == [[0, 2]]
    assert r["configs"][0]["overrides"] == [(0, ZONES[0]), (0, ZONES[1]), (2, ZONES[1])]


def test_reservation_suite(ctx):
    r, = check(ctx, cases.reservation_suite())
    assert [c["reservation_id"] for c in r["configs"]] == ["cr-m5.large-1a-2", "cr-m5.large-1b-1", "cr-m5.xlarge-1b-1"]


def test_reserved_edges(ctx):
    got = check(ctx, cases.reserved_edges())
    assert [r["lt_status"] for r in got] == ["OK", "OK", "OK", "NO_COMPATIBLE_AMI", "OK", "NO_OFFERINGS", "OK", "OK"]
    assert got[2]["configs"][0]["reservation_type"] == "capacity-block" and got[0]["dropped"] == 1


@pytest.mark.parametrize("seed", range(2))
def test_random_reserved_catalogue(ctx, catalog, seed):
    """Random requests over a catalogue with 18 reserved types (tests/test_reserved_offerings.py builds it): the slices
    the three reservation filters leave, recomputed on the device, against the oracle's filters"""
    import test_reserved_offerings as tro
    cat = tro.reserved_catalogue(catalog, 200, seed)
    reqs = tro.reserved_requests(cat, 48, 40 + seed)
    got = check(ctx, (cat, reqs, [ZONES, ZONES[:2]][seed], [AMD, ARM], 60))
    assert sum(r["capacity_type"] == "reserved" and len(r["configs"]) > 0 for r in got) > 0


@pytest.mark.parametrize("n", [1, 2, 257])
def test_batch_sizes_mixing_statuses(ctx, n):
    types, requests, zones, amis, mt = cases.statuses()
    got = check(ctx, (types, [requests[i % len(requests)] for i in range(n)], zones, amis, mt))
    if n == 257:
        assert {(r["status"], r["lt_status"]) for r in got} == {(0, "OK"), (1, "SKIPPED"), (2, "SKIPPED")}


def test_full_catalogue(ctx, catalog):
    from kpamd import synth
    from kpamd.model import AMI
    amis = [AMI("ami-gpu", [(K + "instance-gpu-count", "Exists", [])]), AMD, ARM,
            AMI("ami-rest", [(K + "instance-gpu-count", "DoesNotExist", [])])]
    reqs = synth.random_launch_requests(catalog, 24, seed=11)
    reqs.append(([(CT, "In", ["on-demand"]), (K + "instance-family", "Exists", [], 1)], {"cpu": 100, "pods": 1000},
                 list(range(len(catalog)))))
    got = check(ctx, (catalog, reqs, ZONES, amis, 60))
    assert {"ami-gpu", "ami-123", "ami-456"} <= {c["ami"] for r in got for c in r["configs"]}
    got = check(ctx, (catalog, reqs[-1:], ZONES[:1], amis[:3], 1024))
    assert len(got[0]["types"]) > 900 and len(got[0]["configs"]) > 10


def test_refresh_equals_a_fresh_plan_and_a_stale_plan_is_refused(ctx):
    import kpamd
    types = [cases.typ(i, pods=[29, 110][i % 2]) for i in range(8)]
    requests, amis = [cases.request(8), cases.request([1, 3, 5])], [AMD]
    ch = kpamd.Catalog(ctx, types)
    plan = kpamd.LaunchPlan(ctx, ch, requests, ZONES)
    try:
        before, _ = plan.templates(amis)
        ch.update_offerings([(1, "on-demand", ZONES[0], False), (3, "on-demand", ZONES[1], True, 0.5)], ch.seqnum() + 1)
        with pytest.raises(kpamd.KPError) as e:
            plan.templates(amis)
        assert e.value.code == kpamd.abi.KP_E_INVAL and "stale plan" in str(e.value)
        plan.refresh(ch)
        after, _ = plan.templates(amis)
        fresh = ctx.launch_templates(ch, requests, ZONES, amis)
    finally:
        plan.close()
    want = ref.launch_templates(ch.instance_types, requests, ZONES, amis)
    ch.close()
    assert after == fresh == want and after != before
    assert after[0]["types"][0] == 3 and after[0]["configs"][0]["types"] == [3, 1, 5, 7]
    assert (1, ZONES[0]) not in after[0]["configs"][0]["overrides"] and (1, ZONES[1]) in after[0]["configs"][0]["overrides"]


def test_errors_of_the_device_entry(ctx):
    import kpamd
    from kpamd.model import AMI
    types, requests, zones, _, _ = cases.uniform(3)
    ch = kpamd.Catalog(ctx, types)
    try:
        with pytest.raises(kpamd.KPError) as e:
            ctx.launch_templates(ch, requests, zones, [AMI("ami-x", [("kubernetes.io/arch", 7, ["amd64"])])])
        assert e.value.code == kpamd.abi.KP_E_INVAL
        with pytest.raises(kpamd.KPError) as e:
            ctx.launch_templates(ch, requests, zones, [AMD] * 65536)
        assert e.value.code == kpamd.abi.KP_E_UNSUPPORTED
        r, = ctx.launch_templates(ch, requests, zones, [AMD])  # (the context and the catalogue stay usable)
        assert r["lt_status"] == "OK"
    finally:
        ch.close()
