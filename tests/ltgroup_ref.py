"""Plain-Python reference of the launch-template grouping (kp_launch_templates; the rule: include/kp/
kp_abi.h). The selection comes from the oracle's launch_select, every compatibility judgement from the oracle's
Requirements.Compatible, the offering slices the launch filters leave from the oracle's three reservation filters;
the AMI map, the grouping, the config expansion and the canonical order are dicts and lists. It shares only the model
dataclasses with kpamd. One dict per request, shaped as kpamd.Context.launch_templates returns it."""
import dataclasses

from oracle import pyoracle

CT = "karpenter.sh/capacity-type"
ZONE = "topology.kubernetes.io/zone"
ZONE_ID = "topology.k8s.aws/zone-id"
RES_ID = "karpenter.k8s.aws/capacity-reservation-id"
RES_TYPE = "karpenter.k8s.aws/capacity-reservation-type"
EFA = "vpc.amazonaws.com/efa"
PODS_INDEX, EFA_INDEX = 3, 5  # kp_resource: a resource list may name resources by index


def value(milli):
    """resource.Quantity.Value() of a non-negative quantity held in milli-units: rounded up"""
    return -(-int(milli) // 1000)


def offering_requirements(o):
    """createOfferings (R:offering.go:115-147): the labels an offering requires"""
    reqs = [(CT, "In", [o.capacity_type])]
    if o.zone is not None:
        reqs.append((ZONE, "In", [o.zone]))
    reqs.append((RES_ID, "In", [o.reservation_id]) if o.reservation_id is not None else (RES_ID, "DoesNotExist", []))
    reqs.append((RES_TYPE, "In", [o.reservation_type]) if o.reservation_type is not None
                else (RES_TYPE, "DoesNotExist", []))
    if o.zone_id is not None:
        reqs.append((ZONE_ID, "In", [o.zone_id]))
    return reqs


def ami_for_type(it, amis):
    """MapToInstanceTypes for one type: the first AMI in status order the type is compatible with, no allowance for
    undefined well-known labels; None when no AMI takes it"""
    for i, a in enumerate(amis):
        if pyoracle.requirements_compatible(list(it.requirements), list(a.requirements), allow_wellknown=False):
            return i
    return None


def filtered_slices(instance_types, request):
    """{type index: indices of its offerings} after CompatibleAvailableFilter and the CapacityReservationType /
    CapacityBlock / ReservedOffering filters (R:filter.go:39-274), which replace a type's offering slice; the later
    filters of the chain keep or drop types and leave the slices alone"""
    reqs, requests, listed = request
    if not listed:
        return {}
    kept, _ = pyoracle.compatible_available_filter([instance_types[t] for t in listed], reqs, requests)
    work = [(t, list(range(len(instance_types[t].offerings)))) for t, k in zip(listed, kept) if k]
    for which in ("type", "block", "offering"):
        if not work:
            break
        sub = [dataclasses.replace(instance_types[t], offerings=[instance_types[t].offerings[j] for j in offs])
               for t, offs in work]
        kept, okept = pyoracle.reservation_filter(sub, reqs, which)
        work = [(t, [offs[j] for j in okept[i]]) for i, (t, offs) in enumerate(work) if kept[i]]
    return dict(work)


def launch_templates(instance_types, requests, subnet_zones, amis, max_types=60):
    sels = pyoracle.launch_select(instance_types, requests, subnet_zones, max_types=max_types)
    any_reserved = any(o.capacity_type == "reserved" for it in instance_types for o in it.offerings)
    ami_of = {}
    out = []
    for request, sel in zip(requests, sels):
        d = dict(sel)
        d["n_overrides"] = len(d.pop("overrides"))
        d.update(lt_status="SKIPPED", unmapped=0, dropped=0, configs=[])
        out.append(d)
        if sel["status"] != 0:
            continue
        for t in sel["types"]:
            if t not in ami_of:
                ami_of[t] = ami_for_type(instance_types[t], amis)
        _group(instance_types, request, sel, subnet_zones, amis, ami_of, any_reserved, d)
    return out


def _group(instance_types, request, sel, subnet_zones, amis, ami_of, any_reserved, d):
    reqs, resources, _ = request
    ct = sel["capacity_type"]
    narrowed = [r for r in reqs if r[0] != CT] + [(CT, "In", [ct])]
    efa_asked = EFA in resources or EFA_INDEX in resources
    slices = filtered_slices(instance_types, request) if any_reserved else None
    compatible = {}

    def launchable(o):
        """an override exists for the offering: available, compatible with the narrowed requirements, zone subnet"""
        sig = (o.capacity_type, o.zone, o.zone_id, o.reservation_id, o.reservation_type)
        if sig not in compatible:
            compatible[sig] = pyoracle.requirements_compatible(narrowed, offering_requirements(o), allow_wellknown=True)
        return o.available and compatible[sig] and o.zone in subnet_zones

    def offerings_of(t):
        it = instance_types[t]
        return [(j, it.offerings[j]) for j in (slices[t] if slices is not None else range(len(it.offerings)))]

    def params(t):
        cap = instance_types[t].capacity
        return value(cap.get("pods", cap.get(PODS_INDEX, 0))), value(cap.get(EFA, cap.get(EFA_INDEX, 0))) if efa_asked else 0

    mapped = [t for t in sel["types"] if ami_of[t] is not None]
    d["unmapped"] = len(sel["types"]) - len(mapped)
    configs = []
    if ct == "reserved":
        for t in mapped:  # launch order, then the reservations of the type's slice in offering order
            reserved = [(j, o) for j, o in offerings_of(t) if o.capacity_type == "reserved"]
            for j, o in reserved:
                pods, efa = params(t)
                configs.append({"ami": amis[ami_of[t]].id, "max_pods": pods, "efa_count": efa,
                                "reservation_id": o.reservation_id, "reservation_type": reserved[0][1].reservation_type,
                                "types": [t], "overrides": [(t, o.zone)] if launchable(o) else []})
    else:
        groups = {}  # insertion order: by the launch position of a group's first type
        for t in mapped:
            groups.setdefault((ami_of[t],) + params(t), []).append(t)
        for (ami, pods, efa), members in groups.items():
            configs.append({"ami": amis[ami].id, "max_pods": pods, "efa_count": efa, "reservation_id": None,
                            "reservation_type": None, "types": members,
                            "overrides": [(t, o.zone) for t in members for _, o in offerings_of(t) if launchable(o)]})
    d["configs"] = [c for c in configs if c["overrides"]]
    d["dropped"] = len(configs) - len(d["configs"])
    d["lt_status"] = ("NO_AMIS" if not amis else "NO_COMPATIBLE_AMI" if not mapped
                      else "NO_OFFERINGS" if not d["configs"] else "OK")
