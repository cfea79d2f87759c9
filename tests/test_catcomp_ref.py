"""tests/catcomp_ref.py, the plain-Python statement of kp_catalog_compile's rule, held to hand-written cases and, with
all_zones equal to the subnet zones, to catalog.create_offerings on the whole 919-row table (CPU only)."""
import catcomp_ref as ref
from kpamd import abi, catalog
from kpamd.catalog import CapacityReservation as CR
from kpamd.model import Offering

A = {"name": "a.large", "od_price": 1.0}
B = {"name": "b.large", "od_price": -1.0}  # no on-demand price
ALL = ["z1", "z2", "z3"]
SUBNETS, IDS = ["z1", "z2"], ["i1", "i2"]
SPOT = {("a.large", "z1"): 0.5, ("a.large", "z2"): 0.4, ("a.large", "z3"): 0.3, ("b.large", "z1"): 0.2}


def offs(row=A, bits=0b111, spot=SPOT, unavailable=frozenset(), reservations=()):
    return ref.offerings(row, SUBNETS, IDS, ALL, bits, spot, unavailable, reservations)


def test_a_zone_outside_the_subnets_is_offered_never_available_and_has_no_zone_id():
    assert offs() == [
        Offering("on-demand", "z1", "i1", 1.0, True), Offering("spot", "z1", "i1", 0.5, True),
        Offering("on-demand", "z2", "i2", 1.0, True), Offering("spot", "z2", "i2", 0.4, True),
        Offering("on-demand", "z3", None, 1.0, False), Offering("spot", "z3", None, 0.3, False)]
    assert ref.it_zones(SUBNETS, ALL, 0b111) == 0b011


def test_a_zone_the_type_is_not_offered_in_keeps_its_zone_id():
    got = offs(bits=0b101)
    assert [o.available for o in got] == [True, True, False, False, False, False]
    assert [o.zone_id for o in got] == ["i1", "i1", "i2", "i2", None, None]
    assert ref.it_zones(SUBNETS, ALL, 0b101) == 0b001
    assert ref.it_zones(["z9"], ALL, 0b111) == 0  # a subnet zone that is not in all_zones takes no part


def test_the_three_kinds_of_unavailable_entry():
    assert [o.available for o in offs(unavailable={("spot", "a.large", "z1")})] == [True, False, True, True, False, False]
    assert [o.available for o in offs(unavailable={("spot", "b.large", "z1")})] == [True, True, True, True, False, False]
    assert [o.available for o in offs(unavailable={"on-demand"})] == [False, True, False, True, False, False]
    assert [o.available for o in offs(unavailable={"z2"})] == [True, True, False, False, False, False]
    assert [o.available for o in offs(unavailable={"z2", "spot", ("on-demand", "a.large", "z1")})] == [False] * 6


def test_a_missing_price_is_zero_and_never_available():
    spot = {k: v for k, v in SPOT.items() if k != ("a.large", "z2")}
    got = offs(spot=spot)
    assert (got[3].price, got[3].available) == (0.0, False) and got[2].available
    got = offs(row=B)  # no on-demand price: the spot offering stands on SpotPrice alone
    assert [(o.price, o.available) for o in got] == [(0.0, False), (0.2, True), (0.0, False), (0.0, False), (0.0, False),
                                                     (0.0, False)]


def test_reserved_offerings():
    crs = [CR("cr-1", "a.large", "z1", "default", 2), CR("cr-2", "a.large", "z2", "capacity-block", 0),
           CR("cr-3", "a.large", "z3", "default", 5)]
    got = offs(reservations=crs, unavailable={"z1", "on-demand"})[6:]  # (the unavailable offerings play no part)
    assert got == [Offering("reserved", "z1", "i1", 1.0 / 10_000_000.0, True, "cr-1", "default", 2),
                   Offering("reserved", "z2", "i2", 1.0 / 10_000_000.0, False, "cr-2", "capacity-block", 0),
                   Offering("reserved", "z3", None, 1.0 / 10_000_000.0, False, "cr-3", "default", 5)]
    got = offs(row=B, reservations=[CR("cr-4", "b.large", "z1", "default", 1)])[6:]
    assert got == [Offering("reserved", "z1", "i1", 0.0, True, "cr-4", "default", 1)]
    assert offs(reservations=[CR("cr-1", "a.large", "z1", "default", 2)], bits=0b110)[6].available is False


def test_tables_of_a_small_compile():
    nc = dict(zones=SUBNETS, zone_ids=IDS)
    tab = ref.compile_catalogs([A, B], [nc, dict(zones=["z3"], zone_ids=["i3"])], all_zones=ALL, type_zones=[0b111, 0b001],
                               spot_prices=SPOT, unavailable={("spot", "a.large", "z1")},
                               reservations=[[CR("cr-1", "a.large", "z1", "default", 2)],
                                             [CR("cr-2", "a.large", "z1", "default", 2), CR("cr-3", "b.large", "z3", "default", 0)]],
                               lists=False)
    assert tab["it_zones"].tolist() == [[0b011, 0b001], [0b100, 0]]
    assert tab["available"].tolist() == [[[0b011, 0b010], [0, 0b001]], [[0b100, 0b100], [0, 0]]]
    assert tab["price"].tolist() == [[[1.0, 0.5], [1.0, 0.4], [1.0, 0.3]], [[0.0, 0.2], [0.0, 0.0], [0.0, 0.0]]]
    assert tab["reserved"].tolist() == [(1e-7, 1, 2), (1e-7, 0, 2), (0.0, 0, 0)]
    off = ref.compile_catalogs([A, B], [nc], all_zones=ALL, spot_prices=SPOT, lists=False, reserved_capacity=False,
                               reservations=[[CR("cr-1", "a.large", "z1", "default", 2)]])
    assert len(off["reserved"]) == 0  # the feature gate


def test_discovered_memory_replaces_the_memory_capacity_alone():
    rows = catalog.load_ec2_table()[:3]
    ncs = [dict(), dict(max_pods=20)]
    plain = ref.resource_lists(rows, ncs)
    got = ref.resource_lists(rows, ncs, discovered_memory={(1, rows[2]["name"]): 12345, (0, rows[0]["name"]): -1})
    mem = abi.RES_INDEX["memory"]
    assert got["capacity"][1, 2]["milli"][mem] == 12345 * 1000
    want = plain["capacity"].copy()
    want[1, 2]["milli"][mem] = 12345 * 1000
    assert (got["capacity"] == want).all()
    for k in abi.COMPILE_LISTS[1:]:
        assert (got[k] == plain[k]).all(), k
    t = plain["overhead"]["milli"]
    assert (t == plain["kube_reserved"]["milli"] + plain["system_reserved"]["milli"] + plain["eviction_threshold"]["milli"]).all()


def test_equals_create_offerings_when_all_zones_are_the_subnet_zones():
    rows = catalog.load_ec2_table()
    assert len(rows) == 919 and any(r["od_price"] < 0 for r in rows)
    table = catalog.spot_price_table(rows)          # what build_catalog hands create_offerings
    spot = catalog.default_spot_prices(rows)        # the same prices, unpriced types left out
    unavailable = {("spot", rows[5]["name"], catalog.ZONES[1]), ("on-demand", rows[7]["name"], catalog.ZONES[0]),
                   catalog.ZONES[2]}
    by_type = {rows[3]["name"]: [CR("cr-1", rows[3]["name"], catalog.ZONES[0], "default", 3),
                                 CR("cr-2", rows[3]["name"], catalog.ZONES[2], "capacity-block", 0)]}
    full = (1 << len(catalog.ZONES)) - 1
    for r in rows:
        crs = by_type.get(r["name"], [])
        reqs = catalog.compute_requirements(r, reservations=crs)
        want = catalog.create_offerings(r, reqs, table, unavailable=unavailable, reservations=crs)
        got = ref.offerings(r, catalog.ZONES, catalog.ZONE_IDS, catalog.ZONES, full, spot, unavailable, crs)
        assert got == want, r["name"]
