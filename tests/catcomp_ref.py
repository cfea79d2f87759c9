"""Plain-Python statement of what kp_catalog_compile returns (include/kp/kp_abi.h) — test infrastructure.

The offering rule is createOfferings (R:pkg/providers/instancetype/offering/offering.go:101-187) with the provider's
all_zones distinct from a NodeClass's subnet zones: an offering exists for every zone of all_zones, one in a zone
outside the subnets is never available and carries no zone id. The resource lists come from the oracle
(pyoracle.instance_type_resolve), not from the library; a discovered memory replaces the memory capacity alone
(R:pkg/providers/instancetype/instancetype.go:213-215).
"""
import math

import numpy as np

from kpamd import abi, catalog
from kpamd.model import Offering

CAPACITY_TYPES = ("on-demand", "spot")


def it_zones(nc_zones, all_zones, type_zone_bits):
    """the values of the type's zone requirement, as bits over all_zones"""
    return sum(1 << z for z, name in enumerate(all_zones) if type_zone_bits >> z & 1 and name in set(nc_zones))


def is_unavailable(unavailable, capacity_type, name, zone):
    """UnavailableOfferings.IsUnavailable (R:pkg/cache/unavailableofferings.go:58-63)"""
    return (capacity_type, name, zone) in unavailable or capacity_type in unavailable or zone in unavailable


def price_of(row, zone, capacity_type, spot_prices):
    """(price, hasPrice): OnDemandPrice / SpotPrice; a row's od_price < 0 and a missing spot key are no price"""
    p = (row["od_price"] if row["od_price"] >= 0 else None) if capacity_type == "on-demand" else \
        spot_prices.get((row["name"], zone))
    return (0.0, False) if p is None or math.isnan(p) else (p + 0.0, True)


def offerings(row, nc_zones, nc_zone_ids, all_zones, type_zone_bits, spot_prices, unavailable=frozenset(), reservations=()):
    """createOfferings for one (NodeClass, type): model.Offering records, zones of all_zones x {on-demand, spot}, then
    one reserved offering per reservation of the type"""
    itz = it_zones(nc_zones, all_zones, type_zone_bits)
    zid = dict(zip(nc_zones, nc_zone_ids))  # subnetZonesToZoneIDs
    index = {z: i for i, z in enumerate(all_zones)}
    out = []
    for z, zone in enumerate(all_zones):
        for ct in CAPACITY_TYPES:
            price, has = price_of(row, zone, ct, spot_prices)
            out.append(Offering(ct, zone, zid.get(zone), price,
                                (not is_unavailable(unavailable, ct, row["name"], zone)) and has and bool(itz >> z & 1)))
    od, has_od = price_of(row, None, "on-demand", spot_prices)
    for cr in reservations:
        out.append(Offering("reserved", cr.availability_zone, zid.get(cr.availability_zone),
                            od / 10_000_000.0 if has_od else 0.0,
                            cr.available_count != 0 and bool(itz >> index[cr.availability_zone] & 1),
                            cr.id, cr.reservation_type, int(cr.available_count)))
    return out


def _record(rl):
    return np.frombuffer(bytes(rl), dtype=abi.resource_list_dtype())[0]


def _total(parts):
    """InstanceTypeOverhead.Total(): resources.Merge of the three lists"""
    t = abi.ResourceList()
    for l in parts:
        for r in range(abi.NUM_RES):
            if l.present >> r & 1:
                t.milli[r] += l.milli[r]
                t.present |= 1 << r
    return t


def resource_lists(rows, nodeclasses, opts=None, discovered_memory=None):
    """{list name: [N, T] records} from the oracle"""
    from oracle import pyoracle
    opts = opts or catalog.default_options()
    arena = abi.Arena()
    infos = [catalog.ec2_info(arena, r) for r in rows]
    out = {k: np.zeros((len(nodeclasses), len(rows)), dtype=abi.resource_list_dtype()) for k in abi.COMPILE_LISTS}
    for n, kw in enumerate(nodeclasses):
        nc = catalog.nodeclass(arena, **kw)
        for t, r in enumerate(rows):
            cap, ovh = pyoracle.instance_type_resolve(opts, infos[t], nc)
            d = (discovered_memory or {}).get((n, r["name"]), -1)
            if d >= 0:
                cap.milli[abi.RES_INDEX["memory"]] = d * 1000
            parts = (ovh.kube_reserved, ovh.system_reserved, ovh.eviction_threshold)
            for k, v in zip(abi.COMPILE_LISTS, (cap, _total(parts)) + parts):
                out[k][n, t] = _record(v)
    return out


def compile_catalogs(rows, nodeclasses, all_zones=None, type_zones=None, spot_prices=None, unavailable=(),
                     reservations=None, discovered_memory=None, reserved_capacity=True, opts=None, lists=True):
    """Context.compile_catalogs' tables, from the rule above (lists=False leaves the five resource lists out)"""
    all_zones = list(catalog.ZONES if all_zones is None else all_zones)
    spot_prices = catalog.default_spot_prices(rows, all_zones) if spot_prices is None else spot_prices
    unavailable = set(unavailable)
    N, T, Z = len(nodeclasses), len(rows), len(all_zones)
    tz = [(1 << Z) - 1] * T if type_zones is None else [int(x) for x in type_zones]
    tab = resource_lists(rows, nodeclasses, opts, discovered_memory) if lists else {}
    tab["it_zones"] = np.zeros((N, T), dtype=np.uint64)
    tab["available"] = np.zeros((N, T, 2), dtype=np.uint64)
    tab["price"] = np.zeros((T, Z, 2))
    crs = [list(x) for x in (reservations or [])] if reserved_capacity else []
    recs = []
    for n, kw in enumerate(nodeclasses):
        zones, zone_ids = kw.get("zones", catalog.ZONES), kw.get("zone_ids", catalog.ZONE_IDS)
        mine = crs[n] if n < len(crs) else []
        for t, r in enumerate(rows):
            offs = offerings(r, zones, zone_ids, all_zones, tz[t], spot_prices, unavailable)
            tab["it_zones"][n, t] = it_zones(zones, all_zones, tz[t])
            for j, o in enumerate(offs):
                z, c = divmod(j, 2)
                tab["price"][t, z, c] = o.price
                if o.available:
                    tab["available"][n, t, c] |= np.uint64(1 << z)
        for cr in mine:
            t = next(i for i, r in enumerate(rows) if r["name"] == cr.instance_type)
            o = offerings(rows[t], zones, zone_ids, all_zones, tz[t], spot_prices, unavailable, [cr])[-1]
            recs.append((o.price, int(o.available), o.reservation_capacity))
    tab["reserved"] = np.array(recs, dtype=abi.reserved_offering_dtype()) if recs else \
        np.zeros(0, dtype=abi.reserved_offering_dtype())
    return tab
