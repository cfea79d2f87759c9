"""kpamd — Python host binding of the MI355X bin-packing hot path (libkp.so, include/kp/kp_abi.h).

The surfaces mirror the reference's plugin/operator interface for the path:
  CloudProvider.get_instance_types(nodepool)  <- R:pkg/cloudprovider/cloudprovider.go:177-193
  Scheduler(...).solve(pods)                  <- upstream scheduling.Scheduler.Solve
  compatible_available_filter(...)            <- R:pkg/providers/instance/filter/filter.go:39-64
  ClusterPlan(...).simulate(subsets)          <- upstream disruption computeConsolidation / SimulateScheduling
  ClusterPlan(...).drift(subsets)             <- upstream disruption Drift: SimulateScheduling, the whole Solve
  ClusterPlan(...).command(subsets)           <- computeConsolidation's Command: the replacement NodeClaim + placements
  ClusterPlan(...).candidates(method, now)    <- upstream disruption GetCandidates: reasons, costs and the order
  Context(...).scheduler_inputs(state)        <- upstream NewScheduler's inputs: daemonset overhead, remaining limits,
                                                 StateNode.Available(), the nodes' remaining daemonset requests
  Context(...).compile_catalogs(rows, ncs)    <- GetInstanceTypes' resource and offering halves for every EC2NodeClass
                                                 (catalog.build_catalogs assembles the InstanceType lists from them)
Everything computes behind the C ABI on the GPU; a missing libkp.so or HIP device raises.
"""
import ctypes as C
import os

import numpy as np

from . import abi
from .abi import Arena

_LIB = None
LIB_PATH = os.path.join(abi.PKG_ROOT, "libkp.so")


class KPError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"kp error {code}: {msg}")
        self.code = code


def load_lib(path=None):
    """Load libkp.so (built in-tree by __graft_entry__.build()). Raises if absent — no fallback."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = path or os.environ.get("KP_LIB") or LIB_PATH  # KP_LIB: a diagnostic build (tools/), same ABI
    if not os.path.exists(path):
        raise KPError(abi.KP_E_DEVICE, f"{path} missing: run __graft_entry__.build()")
    lib = C.CDLL(path)
    P = C.POINTER
    sig = {
        "kp_last_error": (C.c_char_p, []),
        "kp_abi_version": (C.c_int32, []),
        "kp_ctx_create": (C.c_int32, [P(abi.Options), P(C.c_void_p)]),
        "kp_ctx_destroy": (None, [C.c_void_p]),
        "kp_ctx_set_overrides": (C.c_int32, [C.c_void_p, P(abi.Overrides)]),
        "kp_ctx_get_overrides": (C.c_int32, [C.c_void_p, P(abi.Overrides)]),
        "kp_catalog_upload": (C.c_int32, [C.c_void_p, P(abi.CatalogDesc), C.c_uint64, P(C.c_void_p)]),
        "kp_catalog_seqnum": (C.c_uint64, [C.c_void_p]),
        "kp_catalog_size": (C.c_uint32, [C.c_void_p]),
        "kp_catalog_destroy": (None, [C.c_void_p]),
        "kp_catalog_update_offerings": (C.c_int32, [C.c_void_p, P(abi.OfferingUpdate), C.c_uint32, C.c_uint64]),
        "kp_instance_type_resolve": (C.c_int32, [P(abi.Options), P(abi.EC2Info), P(abi.NodeClass),
                                                 P(abi.ResourceList), P(abi.ResourceList)]),
        "kp_instance_type_overhead": (C.c_int32, [P(abi.Options), P(abi.EC2Info), P(abi.NodeClass),
                                                  P(abi.ResourceList), P(abi.ResourceList), P(abi.ResourceList)]),
        "kp_filter_compatible_available": (C.c_int32, [C.c_void_p, C.c_void_p, P(abi.FeasibilityQuery), C.c_uint32,
                                                       P(C.c_uint64), P(C.c_double), P(abi.SolveStats)]),
        "kp_filter_prepare": (C.c_int32, [C.c_void_p, C.c_void_p, P(abi.FeasibilityQuery), C.c_uint32, C.c_int32,
                                          P(C.c_void_p)]),
        "kp_filter_run": (C.c_int32, [C.c_void_p, P(C.c_uint64), P(C.c_double), P(abi.SolveStats)]),
        "kp_filter_run_compact": (C.c_int32, [C.c_void_p, P(C.c_uint64), P(C.c_uint64), P(abi.SolveStats)]),
        "kp_filter_class_prices": (C.c_int32, [C.c_void_p, P(C.c_double), C.c_uint32, P(C.c_uint32)]),
        "kp_filter_plan_destroy": (None, [C.c_void_p]),
        "kp_filter_refresh": (C.c_int32, [C.c_void_p, C.c_void_p]),
        "kp_launch_refresh": (C.c_int32, [C.c_void_p, C.c_void_p]),
        "kp_launch_prepare": (C.c_int32, [C.c_void_p, C.c_void_p, P(abi.LaunchRequest), C.c_uint32, P(C.c_char_p),
                                          C.c_uint32, C.c_uint32, P(C.c_void_p)]),
        "kp_launch_run": (C.c_int32, [C.c_void_p, P(abi.LaunchResult), P(C.c_uint32), P(C.c_uint32),
                                      P(abi.SolveStats)]),
        "kp_launch_plan_destroy": (None, [C.c_void_p]),
        "kp_launch_select": (C.c_int32, [C.c_void_p, C.c_void_p, P(abi.LaunchRequest), C.c_uint32, P(C.c_char_p),
                                         C.c_uint32, C.c_uint32, P(abi.LaunchResult), P(C.c_uint32), P(C.c_uint32),
                                         P(abi.SolveStats)]),
        "kp_launch_templates_validate": (C.c_int32, [P(abi.Ami), C.c_uint32]),
        "kp_launch_run_templates": (C.c_int32, [C.c_void_p, P(abi.Ami), C.c_uint32, P(abi.LaunchResult), P(C.c_uint32),
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(abi.SolveStats)]),
        "kp_launch_templates": (C.c_int32, [C.c_void_p, C.c_void_p, P(abi.LaunchRequest), C.c_uint32, P(C.c_char_p),
                                            C.c_uint32, C.c_uint32, P(abi.Ami), C.c_uint32, P(abi.LaunchResult),
                                            P(C.c_uint32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            P(abi.SolveStats)]),
        "kp_solve": (C.c_int32, [C.c_void_p, P(abi.SolveIn), P(C.c_void_p)]),
        "kp_solve_validate": (C.c_int32, [P(abi.SolveIn)]),
        "kp_solve_prepare": (C.c_int32, [C.c_void_p, P(abi.SolveIn), P(C.c_void_p)]),
        "kp_solve_prepare_comm": (C.c_int32, [C.c_void_p, P(abi.SolveIn), C.c_void_p, P(C.c_void_p)]),
        "kp_solve_run": (C.c_int32, [C.c_void_p, P(C.c_void_p)]),
        "kp_solve_run_cancellable": (C.c_int32, [C.c_void_p, C.c_void_p, P(C.c_void_p)]),
        "kp_solve_cancellable": (C.c_int32, [C.c_void_p, P(abi.SolveIn), C.c_void_p, P(C.c_void_p)]),
        "kp_cancel_create": (C.c_int32, [C.c_void_p, P(C.c_void_p)]),
        "kp_cancel_set": (C.c_int32, [C.c_void_p]),
        "kp_cancel_reset": (C.c_int32, [C.c_void_p]),
        "kp_cancel_destroy": (None, [C.c_void_p]),
        "kp_solve_refresh": (C.c_int32, [C.c_void_p]),
        "kp_cluster_refresh": (C.c_int32, [C.c_void_p]),
        "kp_solve_plan_destroy": (None, [C.c_void_p]),
        "kp_result_nodeclaim_count": (C.c_uint32, [C.c_void_p]),
        "kp_result_pod_placements": (C.c_int32, [C.c_void_p, P(C.c_int32), C.c_uint32]),
        "kp_result_nodeclaim": (C.c_int32, [C.c_void_p, C.c_uint32, P(abi.NodeClaimInfo)]),
        "kp_result_stats": (C.c_int32, [C.c_void_p, P(abi.SolveStats)]),
        "kp_result_destroy": (None, [C.c_void_p]),
        "kp_solve_explained": (C.c_int32, [C.c_void_p, P(abi.SolveIn), C.c_void_p, P(C.c_void_p)]),
        "kp_solve_run_explained": (C.c_int32, [C.c_void_p, C.c_void_p, P(C.c_void_p)]),
        "kp_result_explained": (C.c_int32, [C.c_void_p]),
        "kp_result_reason_count": (C.c_uint32, [C.c_void_p, C.c_uint32]),
        "kp_result_pod_reasons": (C.c_int32, [C.c_void_p, C.c_uint32, P(abi.PoolReason), C.c_uint32]),
        "kp_simulate_batch": (C.c_int32, [C.c_void_p, P(abi.Cluster), P(C.c_uint32), P(C.c_uint32), C.c_uint32,
                                          C.c_int32, P(abi.SimResult), P(abi.SolveStats)]),
        "kp_cluster_prepare": (C.c_int32, [C.c_void_p, P(abi.Cluster), P(C.c_void_p)]),
        "kp_cluster_simulate": (C.c_int32, [C.c_void_p, P(C.c_uint32), P(C.c_uint32), C.c_uint32, C.c_int32,
                                            P(abi.SimResult), P(abi.SolveStats)]),
        "kp_cluster_simulate_cancellable": (C.c_int32, [C.c_void_p, C.c_void_p, P(C.c_uint32), P(C.c_uint32), C.c_uint32,
                                                        C.c_int32, P(abi.SimResult), P(abi.SolveStats)]),
        "kp_cluster_plan_destroy": (None, [C.c_void_p]),
        "kp_comm_unique_id": (C.c_int32, [C.c_char_p]),
        "kp_comm_init": (C.c_int32, [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, P(C.c_void_p)]),
        "kp_comm_destroy": (None, [C.c_void_p]),
        "kp_comm_init_all": (C.c_int32, [P(C.c_void_p), C.c_int32, P(C.c_void_p)]),
        "kp_comm_init_host": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, abi.AllGatherFn, C.c_void_p,
                                          P(C.c_void_p)]),
        "kp_comm_rank": (C.c_int32, [C.c_void_p, P(C.c_int32), P(C.c_int32)]),
        "kp_consolidate_argmin": (C.c_int32, [C.c_void_p, C.c_void_p, P(C.c_uint32), P(C.c_uint32), C.c_uint32,
                                              C.c_uint64, C.c_int32, P(abi.SimResult), P(abi.Choice),
                                              P(abi.SolveStats)]),
        "kp_consolidate_argmin_cancellable": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_uint32),
                                                          P(C.c_uint32), C.c_uint32, C.c_uint64, C.c_int32,
                                                          P(abi.SimResult), P(abi.Choice), P(abi.SolveStats)]),
        "kp_choice_reduce": (C.c_int32, [P(abi.Choice), C.c_uint32, P(abi.Choice)]),
        "kp_cluster_simulate_budgeted": (C.c_int32, [C.c_void_p, C.c_void_p, P(C.c_uint32), P(C.c_uint32), C.c_uint32,
                                                     C.c_int32, P(C.c_uint32), C.c_uint32, P(abi.SimResult),
                                                     P(C.c_uint64), P(abi.SolveStats)]),
        "kp_consolidate_argmin_budgeted": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_uint32), P(C.c_uint32),
                                                       C.c_uint32, C.c_uint64, C.c_int32, P(C.c_uint32), C.c_uint32,
                                                       P(abi.SimResult), P(abi.Choice), P(C.c_uint64),
                                                       P(abi.SolveStats)]),
        "kp_cluster_drift": (C.c_int32, [C.c_void_p, C.c_void_p, P(C.c_uint32), P(C.c_uint32), C.c_uint32, P(C.c_uint32),
                                         C.c_uint32, P(abi.DriftResult), P(C.c_int64), P(C.c_void_p), P(C.c_uint64),
                                         P(abi.SolveStats)]),
        "kp_cluster_command": (C.c_int32, [C.c_void_p, C.c_void_p, P(C.c_uint32), P(C.c_uint32), C.c_uint32, C.c_int32,
                                           P(C.c_uint32), C.c_uint32, P(abi.SimResult), P(C.c_void_p), P(C.c_uint64),
                                           P(abi.SolveStats)]),
        "kp_cluster_validate": (C.c_int32, [C.c_void_p, C.c_void_p, P(C.c_uint32), P(C.c_uint32), C.c_uint32,
                                            P(abi.CommandCheck), P(C.c_uint32), C.c_uint32, P(abi.Validation),
                                            P(C.c_uint64), P(abi.SolveStats)]),
        "kp_cluster_candidates": (C.c_int32, [C.c_void_p, P(abi.CandidatesIn), C.c_void_p, P(C.c_uint32), P(C.c_uint32),
                                              P(abi.SolveStats)]),
        "kp_cluster_detect_drift": (C.c_int32, [C.c_void_p, P(abi.DriftIn), C.c_void_p, P(C.c_uint64),
                                                P(abi.SolveStats)]),
        "kp_interruptions_validate": (C.c_int32, [P(abi.InterruptIn)]),
        "kp_cluster_interruptions": (C.c_int32, [C.c_void_p, P(abi.InterruptIn), C.c_void_p, C.c_void_p, C.c_void_p,
                                                 P(C.c_uint32), C.c_void_p, P(C.c_uint32), P(C.c_uint64),
                                                 P(abi.SolveStats)]),
        "kp_cluster_simulate_explained": (C.c_int32, [C.c_void_p, C.c_void_p, P(C.c_uint32), P(C.c_uint32), C.c_uint32,
                                                      C.c_int32, P(C.c_uint32), C.c_uint32, P(abi.SimResult),
                                                      P(abi.SimWhy), P(C.c_uint64), P(C.c_uint64), P(abi.SolveStats)]),
        "kp_scheduler_inputs": (C.c_int32, [C.c_void_p, P(abi.SchedState), P(abi.SchedOut), P(abi.SolveStats)]),
        "kp_catalog_compile": (C.c_int32, [C.c_void_p, P(abi.CompileIn), P(abi.CompileOut), P(abi.SolveStats)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name, None)
        if f is None and path != LIB_PATH:  # a tools/ build of an older commit (A/B): its ABI may lack newer entries
            continue
        if f is None:
            raise KPError(abi.KP_E_DEVICE, f"{path} lacks {name}: rebuild (__graft_entry__.build())")
        f.restype = res
        f.argtypes = args
    _LIB = lib
    return lib


def _check(lib, rc):
    if rc != 0:
        raise KPError(rc, lib.kp_last_error().decode())


class Context:
    """kp_ctx: one HIP device + stream."""

    def __init__(self, device=0, vm_memory_overhead_percent=0.075, reserved_enis=0):
        self.lib = load_lib()
        self.opts = abi.Options(vm_memory_overhead_percent, reserved_enis, device)
        h = C.c_void_p()
        _check(self.lib, self.lib.kp_ctx_create(C.byref(self.opts), C.byref(h)))
        self.h = h

    def overrides(self):
        """kp_ctx_get_overrides -> dict of the kp_overrides fields."""
        ov = abi.Overrides()
        _check(self.lib, self.lib.kp_ctx_get_overrides(self.h, C.byref(ov)))
        return {k: getattr(ov, k) for k, _ in abi.Overrides._fields_}

    def set_overrides(self, **kw):
        """kp_ctx_set_overrides: the given kp_overrides fields, every other field 0 (the production choice)."""
        ov = abi.Overrides(**kw)
        _check(self.lib, self.lib.kp_ctx_set_overrides(self.h, C.byref(ov)))

    def scheduler_inputs(self, state):
        """kp_scheduler_inputs: the daemonset overhead per NodePool template and per node, the remaining limits and the
        nodes' available resources, computed on the device from a model.SchedulerState."""
        arena = Arena()
        st = abi.build_sched_state(arena, state)
        return SchedulerInputs(*_scheduler_inputs_raw(self.lib, self.h, st))

    def compile_catalogs(self, rows, nodeclasses, all_zones=None, type_zones=None, spot_prices=None, unavailable=(),
                         reservations=None, discovered_memory=None, reserved_capacity=True, outputs=None, opts=None):
        """kp_catalog_compile: the capacity / overhead lists and the offering tables of every (NodeClass, instance
        type) pair, computed on the device. rows: EC2 table rows; nodeclasses: one dict of
        catalog.nodeclass keyword arguments per EC2NodeClass; all_zones: the provider's zones (default catalog.ZONES);
        type_zones: per row, the zones it is offered in as bits over all_zones (default: all); spot_prices:
        {(type name, zone): price}, a missing key is no price (default catalog.default_spot_prices); a row's od_price
        < 0 is no on-demand price; unavailable: (capacity type, type name, zone) triples, capacity types and zones;
        reservations: per NodeClass a list of catalog.CapacityReservation; discovered_memory: {(NodeClass index, type
        name): bytes}; outputs: the tables wanted (default abi.COMPILE_OUTPUTS); opts: abi.Options in place of the
        context's (the call carries its own kp_options). Returns a dict of numpy arrays:
        the five lists [N, T] of abi.resource_list_dtype(), it_zones [N, T], price [T, Z, 2], available [N, T, 2],
        reserved [n_reservations] of abi.reserved_offering_dtype(), plus "stats"."""
        from . import catalog
        all_zones = list(catalog.ZONES if all_zones is None else all_zones)
        spot_prices = catalog.default_spot_prices(rows, all_zones) if spot_prices is None else spot_prices
        arena = Arena()
        cin = build_compile_in(arena, opts or self.opts, rows, nodeclasses, all_zones, type_zones, spot_prices, unavailable,
                               reservations, discovered_memory, reserved_capacity)
        return _catalog_compile_raw(self.lib, self.h, cin, abi.COMPILE_OUTPUTS if outputs is None else outputs)

    def launch_templates(self, catalog, requests, subnet_zones, amis, max_types=60):
        """kp_launch_templates: the launch-side selection of each request followed by its CreateFleet launch-template
        configs. Returns one dict per request: the launch_select fields (the flat override list replaced
        by its length, n_overrides), lt_status, unmapped, dropped and configs [{ami, max_pods, efa_count,
        reservation_id, reservation_type, types, overrides}] in canonical order."""
        arena = Arena()
        rq = abi.launch_requests(arena, requests)
        zones = list(subnet_zones)
        zs = arena.arr(C.c_char_p, [z.encode() for z in zones])
        am, n_amis = abi.amis(arena, amis)
        lib = self.lib
        return _read_templates(lib, lambda *bufs: lib.kp_launch_templates(self.h, catalog.h, rq, len(requests), zs,
                                                                          len(zones), max_types, am, n_amis, *bufs),
                               len(requests), max_types, zones, amis, catalog.instance_types)[0]

    def close(self):
        if self.h:
            self.lib.kp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build_compile_in(arena, opts, rows, nodeclasses, all_zones, type_zones=None, spot_prices=None, unavailable=(),
                     reservations=None, discovered_memory=None, reserved_capacity=True):
    """The arguments of Context.compile_catalogs -> kp_compile_in (buffers kept by the arena)."""
    from . import catalog
    T, N, Z = len(rows), len(nodeclasses), len(all_zones)
    index = {r["name"]: t for t, r in enumerate(rows)}
    nan = float("nan")
    tz = np.full(max(1, T), (1 << Z) - 1 if type_zones is None else 0, dtype=np.uint64)
    if type_zones is not None:
        tz[:T] = np.asarray(list(type_zones), dtype=np.uint64)
    od = np.full(max(1, T), nan)
    spot = np.full((max(1, T), max(1, Z)), nan)
    for t, r in enumerate(rows):
        if r["od_price"] >= 0:
            od[t] = r["od_price"]
        for z, zone in enumerate(all_zones):
            p = (spot_prices or {}).get((r["name"], zone))
            if p is not None:
                spot[t, z] = p
    spot = np.ascontiguousarray(spot[:, :Z]) if Z else spot
    unav = []
    for u in unavailable:
        if isinstance(u, tuple):
            unav.append(abi.Unavailable(arena.s(u[0]), arena.s(u[2]), index[u[1]], 0))
        elif u in abi.CAPACITY_TYPES:
            unav.append(abi.Unavailable(arena.s(u), None, -1, 0))
        else:
            unav.append(abi.Unavailable(None, arena.s(u), -1, 0))
    offs = np.zeros(N + 1, dtype=np.uint32)
    res = []
    for n, crs in enumerate(reservations or []):
        for cr in crs:
            res.append(abi.CompileReservation(arena.s(cr.id), arena.s(cr.availability_zone), arena.s(cr.reservation_type),
                                              index[cr.instance_type], int(cr.available_count)))
        offs[n + 1] = len(res)
    offs[len(reservations or []) + 1:] = len(res)
    disc = None
    if discovered_memory is not None:
        disc = np.full((max(1, N), max(1, T)), -1, dtype=np.int64)
        for (n, name), b in discovered_memory.items():
            disc[n, index[name]] = b
    arena.keep.extend([tz, od, spot, offs, disc])
    ptr = lambda a, ct: a.ctypes.data_as(C.POINTER(ct))
    cin = abi.CompileIn(opts, arena.arr(abi.EC2Info, [catalog.ec2_info(arena, r) for r in rows]),
                        arena.arr(abi.NodeClass, [catalog.nodeclass(arena, **kw) for kw in nodeclasses]),
                        arena.arr(C.c_char_p, [arena.s(z) for z in all_zones]), ptr(tz, C.c_uint64), ptr(od, C.c_double),
                        ptr(spot, C.c_double), arena.arr(abi.Unavailable, unav), ptr(offs, C.c_uint32),
                        arena.arr(abi.CompileReservation, res), None if disc is None else ptr(disc, C.c_int64),
                        T, N, Z, len(unav), len(res), 1 if reserved_capacity else 0)
    arena.keep.append(cin)
    return cin


def _catalog_compile_raw(lib, ctx_h, cin, outputs=abi.COMPILE_OUTPUTS):
    """One kp_catalog_compile call on a marshalled kp_compile_in: {output name: numpy array} of the outputs asked
    for, plus "stats"."""
    N, T, Z, R = cin.n_nodeclasses, cin.n_types, cin.n_all_zones, cin.n_reservations
    rl = abi.resource_list_dtype()
    shapes = {"it_zones": ((N, T), np.uint64), "price": ((T, Z, 2), np.float64), "available": ((N, T, 2), np.uint64),
              "reserved": ((R,), abi.reserved_offering_dtype())}
    shapes.update({k: ((N, T), rl) for k in abi.COMPILE_LISTS})
    unknown = set(outputs) - set(abi.COMPILE_OUTPUTS)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    tables, out = {}, abi.CompileOut()
    for k, ctype in abi.CompileOut._fields_:
        if k not in outputs:
            continue
        shape, dt = shapes[k]
        n = int(np.prod(shape))
        buf = np.zeros(max(1, n), dtype=dt)  # (never a NULL pointer for an output that was asked for)
        tables[k] = buf[:n].reshape(shape)
        setattr(out, k, C.cast(buf.ctypes.data, ctype))
    stats = abi.SolveStats()
    _check(lib, lib.kp_catalog_compile(ctx_h, C.byref(cin), C.byref(out), C.byref(stats)))
    tables["stats"] = stats_dict(stats)
    return tables


def _scheduler_inputs_raw(lib, ctx_h, st):
    """One kp_scheduler_inputs call on a marshalled kp_sched_state: (node records, pool records, words, stats)."""
    N, P, D = st.n_nodes, st.n_nodepools, st.n_daemonsets
    W = max(1, (D + 63) // 64)
    nodes = (abi.SchedNodeOut * max(1, N))()
    pools = (abi.SchedPoolOut * max(1, P))()
    words = np.zeros((max(1, N), W), dtype=np.uint64)
    out = abi.SchedOut(nodes, pools, words.ctypes.data_as(C.POINTER(C.c_uint64)))
    stats = abi.SolveStats()
    _check(lib, lib.kp_scheduler_inputs(ctx_h, C.byref(st), C.byref(out), C.byref(stats)))
    return nodes, pools, words[:N], N, P, stats


class SchedulerInputs:
    """What kp_scheduler_inputs returns. Per node: available, requests (the remaining daemonset requests),
    n_compatible and the compatibility words (uint64 [N, ceil(D / 64)]: template d at bit d % 64 of word d // 64); per
    NodePool: daemon_requests, remaining (None: the pool has no limits) and n_compatible."""

    def __init__(self, nodes, pools, words, n_nodes, n_pools, stats=None):
        self.raw_nodes, self.raw_pools = nodes, pools  # the records as the library wrote them (byte comparisons)
        self.available = [abi.read_resources(nodes[i].available) for i in range(n_nodes)]
        self.requests = [abi.read_resources(nodes[i].requests) for i in range(n_nodes)]
        self.node_compatible = [int(nodes[i].n_compatible) for i in range(n_nodes)]
        self.compat = words
        self.daemon_requests = [abi.read_resources(pools[p].daemon_requests) for p in range(n_pools)]
        self.remaining = [abi.read_resources(pools[p].remaining) if pools[p].remaining.present else None
                          for p in range(n_pools)]
        self.pool_compatible = [int(pools[p].n_compatible) for p in range(n_pools)]
        self.stats = stats_dict(stats) if stats is not None else None

    def apply(self, target):
        """Write NodePool.daemon_requests, NodePool.limits (the remainder), ExistingNode.available and
        ExistingNode.requests onto a model.Problem or model.Cluster whose NodePools and nodes are in the state's
        order. Returns target."""
        nodes = target.existing if hasattr(target, "existing") else [n.node for n in target.nodes]
        if len(nodes) != len(self.available) or len(target.nodepools) != len(self.daemon_requests):
            raise ValueError("the target's nodes and NodePools are not the state's")
        for np_, dr, rem in zip(target.nodepools, self.daemon_requests, self.remaining):
            np_.daemon_requests = dict(dr)
            np_.limits = dict(rem) if rem is not None else {}
        for n, av, rq in zip(nodes, self.available, self.requests):
            n.available = dict(av)
            n.requests = dict(rq)
        return target


class Catalog:
    """A GetInstanceTypes result uploaded behind the ABI (kp_catalog_upload)."""

    def __init__(self, ctx, instance_types, seqnum=0):
        self.ctx = ctx
        self.instance_types = instance_types
        arena = Arena()
        desc = arena.catalog_desc(instance_types)
        h = C.c_void_p()
        _check(ctx.lib, ctx.lib.kp_catalog_upload(ctx.h, C.byref(desc), seqnum, C.byref(h)))
        self.h = h

    def update_offerings(self, updates, seqnum):
        """kp_catalog_update_offerings: UnavailableOfferings.MarkUnavailable + SeqNum bump
        (R:pkg/cache/unavailableofferings.go:66-92). updates: (type index, capacity type, zone, available[, price
        [, reservation id[, reservation capacity]]]); the matching offerings of self.instance_types change with the
        device-side catalogue (all or nothing)."""
        def opt(u, i):
            return u[i] if len(u) > i else None
        for i, u in enumerate(updates):  # (behind the ABI a NaN price means "keep": it cannot be set)
            if opt(u, 4) is not None and float(u[4]) != float(u[4]):
                raise KPError(abi.KP_E_INVAL, f"update {i}: type {u[0]} ({self.instance_types[u[0]].name}) given price "
                                              f"nan (a price is a number >= 0)")
        ups = [abi.OfferingUpdate(int(u[0]), 1 if u[3] else 0, u[1].encode() if u[1] is not None else None,
                                  u[2].encode() if u[2] is not None else None,
                                  float(u[4]) if opt(u, 4) is not None else float("nan"),
                                  opt(u, 5).encode() if opt(u, 5) is not None else None,
                                  int(opt(u, 6)) if opt(u, 6) is not None else -1, 0) for u in updates]
        arr = (abi.OfferingUpdate * max(1, len(ups)))(*ups)
        _check(self.ctx.lib, self.ctx.lib.kp_catalog_update_offerings(self.h, arr, len(ups), seqnum))
        for u in updates:
            for o in self.instance_types[u[0]].offerings:
                if o.capacity_type == u[1] and o.zone == u[2] and (opt(u, 5) is None or o.reservation_id == opt(u, 5)):
                    o.available = bool(u[3])
                    if opt(u, 4) is not None:
                        o.price = float(u[4]) + 0.0  # (-0.0 is stored as +0.0)
                    if opt(u, 6) is not None and int(opt(u, 6)) >= 0:
                        o.reservation_capacity = int(opt(u, 6))

    def seqnum(self):
        return self.ctx.lib.kp_catalog_seqnum(self.h)

    def close(self):
        if self.h:
            self.ctx.lib.kp_catalog_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def validate(problem):
    """kp_solve_validate: host compile of the batch without a device (KP_OK or the error kp_solve would give)."""
    lib = load_lib()
    arena = Arena()
    handles = []
    for c in problem.catalogs:
        h = C.c_void_p()
        _check(lib, lib.kp_catalog_upload(None, C.byref(arena.catalog_desc(c)), 0, C.byref(h)))
        handles.append(h)
    try:
        si = abi.build_solve_in(arena, problem, catalog_handles=[h.value for h in handles])
        return lib.kp_solve_validate(C.byref(si))
    finally:
        for h in handles:
            lib.kp_catalog_destroy(h)


def read_result(lib, res, n_pods, prefix="kp_result_"):
    """Copy a (kp|kpo)_solve_result into plain Python: placement + NodeClaims in creation order."""
    get = lambda n: getattr(lib, prefix + n)
    placement = np.zeros(n_pods, dtype=np.int32)
    if n_pods:
        _check_generic(lib, get("pod_placements")(res, placement.ctypes.data_as(C.POINTER(C.c_int32)), n_pods))
    ncs = []
    n = get("nodeclaim_count")(res)
    for i in range(n):
        info = abi.NodeClaimInfo()
        _check_generic(lib, get("nodeclaim")(res, i, C.byref(info)))
        ncs.append({
            "nodepool": int(info.nodepool),
            "pods": [int(info.pods[j]) for j in range(info.n_pods)],
            "options": [int(info.options[j]) for j in range(info.n_options)],
            "n_remaining": int(info.n_remaining),
            "requirements": abi.read_requirements(info.requirements),
            "requests": abi.read_resources(info.requests),
        })
    st = abi.SolveStats()
    get("stats")(res, C.byref(st))
    return {"placement": placement, "nodeclaims": ncs, "stats": stats_dict(st)}


def read_reasons(lib, res, placement):
    """result["reasons"] of an explained kp_solve_result: for every unscheduled pod (placement -1), one dict per
    NodePool template in the Solve's template order: nodepool, code (abi.KP_WHY_*), taint, keys and the counts."""
    out = {}
    for p in np.flatnonzero(placement == -1):
        n = lib.kp_result_reason_count(res, int(p))
        buf = (abi.PoolReason * max(1, n))()
        _check_generic(lib, lib.kp_result_pod_reasons(res, int(p), buf, n))
        rows = []
        for r in buf[:n]:
            d = {"nodepool": int(r.nodepool), "code": int(r.code), "taint": int(r.taint),
                 "keys": [r.keys[i].decode() for i in range(r.n_keys)]}
            d.update({f: int(getattr(r, f)) for f in abi.REASON_COUNTS})
            rows.append(d)
        out[int(p)] = rows
    return out


def stats_dict(st):
    d = {f: getattr(st, f) for f, _ in abi.SolveStats._fields_}
    d["phase_cycles"] = list(st.phase_cycles)
    d["attempt_cycles"] = list(st.attempt_cycles)
    d["fast_cycles"] = list(st.fast_cycles)
    d["fast_bails"] = list(st.fast_bails)
    d["order_chunks"] = list(st.order_chunks)
    return d


def _check_generic(lib, rc):
    if rc != 0:
        msg = lib.kp_last_error().decode() if hasattr(lib, "kp_last_error") else ""
        raise KPError(rc, msg)


class Scheduler:
    """upstream scheduling.Scheduler for one batch: NodePools (templates), existing nodes, catalogues."""

    def __init__(self, ctx, problem, catalogs=None):
        self.ctx = ctx
        self.problem = problem
        self.catalogs = catalogs or [Catalog(ctx, c) for c in problem.catalogs]

    def solve_in(self):
        """The kp_solve_in of this batch (marshalled once; the C ABI owns nothing of it)."""
        if getattr(self, "_si", None) is None:
            self._arena = Arena()
            self._si = abi.build_solve_in(self._arena, self.problem, catalog_handles=[c.h.value for c in self.catalogs])
        return self._si

    def solve(self, read=True, explain=False):
        """kp_solve: compile the per-Solve half (the catalogue half comes resident from the ctx cache after the first
        Solve on these catalogues + NodePools), upload, run, copy the results back. read=False returns stats only.
        explain=True: kp_solve_explained; the result's "reasons" maps every unscheduled pod to its per-NodePool
        reasons (read_reasons)."""
        lib = self.ctx.lib
        si = self.solve_in()
        res = C.c_void_p()
        if explain:
            _check(lib, lib.kp_solve_explained(self.ctx.h, C.byref(si), None, C.byref(res)))
        else:
            _check(lib, lib.kp_solve(self.ctx.h, C.byref(si), C.byref(res)))
        try:
            if read:
                out = read_result(lib, res, self.problem.n_pods)
                if explain:
                    out["reasons"] = read_reasons(lib, res, out["placement"])
                return out
            st = abi.SolveStats()
            lib.kp_result_stats(res, C.byref(st))
            return {"stats": stats_dict(st)}
        finally:
            lib.kp_result_destroy(res)

    def prepare(self, comm=None):
        """kp_solve_prepare: compile + upload once; returns a SolvePlan whose run() repeats Solve. With a Comm,
        kp_solve_prepare_comm: a collective whose template-options table is row-sharded over the ranks and
        all-gathered (every rank passes the same batch)."""
        return SolvePlan(self, comm)


class Cancel:
    """kp_cancel: the token a Go shim sets when ctx.Done() fires during a Solve (set() is lock-free, any thread)."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = C.c_void_p()
        _check(ctx.lib, ctx.lib.kp_cancel_create(ctx.h, C.byref(h)))
        self.h = h

    def set(self):
        _check(self.ctx.lib, self.ctx.lib.kp_cancel_set(self.h))

    def reset(self):
        _check(self.ctx.lib, self.ctx.lib.kp_cancel_reset(self.h))

    def close(self):
        if self.h:
            self.ctx.lib.kp_cancel_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SolvePlan:
    def __init__(self, sched, comm=None):
        self.sched = sched
        lib = sched.ctx.lib
        arena = Arena()
        si = abi.build_solve_in(arena, sched.problem, catalog_handles=[c.h.value for c in sched.catalogs])
        h = C.c_void_p()
        if comm is None:
            _check(lib, lib.kp_solve_prepare(sched.ctx.h, C.byref(si), C.byref(h)))
        else:
            _check(lib, lib.kp_solve_prepare_comm(sched.ctx.h, C.byref(si), comm.h, C.byref(h)))
        self.h = h

    def run(self, read=True, cancel=None, explain=False):
        """kp_solve_run; with a Cancel token, kp_solve_run_cancellable (KPError KP_E_CANCELED once it is set).
        explain=True: kp_solve_run_explained (the token optional); the result's "reasons" maps every unscheduled pod
        to its per-NodePool reasons (read_reasons)."""
        lib = self.sched.ctx.lib
        res = C.c_void_p()
        if explain:
            _check(lib, lib.kp_solve_run_explained(self.h, cancel.h if cancel is not None else None, C.byref(res)))
        elif cancel is None:
            _check(lib, lib.kp_solve_run(self.h, C.byref(res)))
        else:
            _check(lib, lib.kp_solve_run_cancellable(self.h, cancel.h, C.byref(res)))
        try:
            if read:
                out = read_result(lib, res, self.sched.problem.n_pods)
                if explain:
                    out["reasons"] = read_reasons(lib, res, out["placement"])
                return out
            st = abi.SolveStats()
            lib.kp_result_stats(res, C.byref(st))
            return {"stats": stats_dict(st)}
        finally:
            lib.kp_result_destroy(res)

    def refresh(self):
        """kp_solve_refresh: re-apply the catalogues' current offerings (after update_offerings) in place."""
        _check(self.sched.ctx.lib, self.sched.ctx.lib.kp_solve_refresh(self.h))

    def close(self):
        if self.h:
            self.sched.ctx.lib.kp_solve_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def compatible_available_filter(ctx, catalog, queries):
    """queries: list of (requirements, requests). Returns (kept bool[Q,T], cheapest f64[Q,T], stats)."""
    lib = ctx.lib
    arena = Arena()
    qs = arena.arr(abi.FeasibilityQuery, [abi.FeasibilityQuery(arena.requirements(r), arena.resources(q))
                                          for r, q in queries])
    T = len(catalog.instance_types)
    tiles = (T + 63) // 64
    mask = np.zeros(max(1, len(queries) * tiles), dtype=np.uint64)
    cheapest = np.zeros(max(1, len(queries) * T), dtype=np.float64)
    st = abi.SolveStats()
    _check(lib, lib.kp_filter_compatible_available(ctx.h, catalog.h, qs, len(queries),
                                                   mask.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   cheapest.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st)))
    bits = np.unpackbits(mask[:len(queries) * tiles].view(np.uint8), bitorder="little").reshape(len(queries), tiles * 64)
    return bits[:, :T].astype(bool), cheapest[:len(queries) * T].reshape(len(queries), T), st


class FilterPlan:
    """kp_filter_prepare / kp_filter_run: CompatibleAvailableFilter rows resident on the device."""

    def __init__(self, ctx, catalog, queries, cheapest=True):
        """cheapest: True (KP_FILTER_CHEAPEST: a price row per query), False (mask only) or "compact"
        (KP_FILTER_COMPACT: the query's compatible offering classes; prices via class_prices())."""
        self.ctx = ctx
        self.T = len(catalog.instance_types)
        self.n = len(queries)
        mode = 2 if cheapest == "compact" else (1 if cheapest else 0)
        self.mode = mode
        arena = Arena()
        qs = arena.arr(abi.FeasibilityQuery, [abi.FeasibilityQuery(arena.requirements(r), arena.resources(q))
                                              for r, q in queries])
        h = C.c_void_p()
        _check(ctx.lib, ctx.lib.kp_filter_prepare(ctx.h, catalog.h, qs, len(queries), mode, C.byref(h)))
        self.h = h

    def run(self, read=False):
        """One launch; read=True copies (kept bool[Q,T], cheapest f64[Q,T]) back, else results stay resident. A plan
        without price rows (mask only, compact) gives cheapest = None."""
        st = abi.SolveStats()
        lib = self.ctx.lib
        if not read:
            _check(lib, lib.kp_filter_run(self.h, None, None, C.byref(st)))
            return stats_dict(st)
        tiles = (self.T + 63) // 64
        mask = np.zeros(max(1, self.n * tiles), dtype=np.uint64)
        cheapest = np.zeros(max(1, self.n * self.T), dtype=np.float64) if self.mode == 1 else None
        _check(lib, lib.kp_filter_run(self.h, mask.ctypes.data_as(C.POINTER(C.c_uint64)),
                                      cheapest.ctypes.data_as(C.POINTER(C.c_double)) if self.mode == 1 else None,
                                      C.byref(st)))
        bits = np.unpackbits(mask[:self.n * tiles].view(np.uint8), bitorder="little").reshape(self.n, tiles * 64)
        if cheapest is not None:
            cheapest = cheapest[:self.n * self.T].reshape(self.n, self.T)
        return bits[:, :self.T].astype(bool), cheapest, stats_dict(st)

    def run_compact(self, read=True):
        """kp_filter_run_compact: (kept bool[Q,T], classes uint64[Q], stats); read=False: stats only."""
        st = abi.SolveStats()
        lib = self.ctx.lib
        if not read:
            _check(lib, lib.kp_filter_run_compact(self.h, None, None, C.byref(st)))
            return stats_dict(st)
        tiles = (self.T + 63) // 64
        mask = np.zeros(max(1, self.n * tiles), dtype=np.uint64)
        cls = np.zeros(max(1, self.n), dtype=np.uint64)
        _check(lib, lib.kp_filter_run_compact(self.h, mask.ctypes.data_as(C.POINTER(C.c_uint64)),
                                              cls.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(st)))
        bits = np.unpackbits(mask[:self.n * tiles].view(np.uint8), bitorder="little").reshape(self.n, tiles * 64)
        return bits[:, :self.T].astype(bool), cls[:self.n], stats_dict(st)

    def class_prices(self):
        """kp_filter_class_prices: float64[C, T], the cheapest available offering of each type per offering class."""
        lib = self.ctx.lib
        n = C.c_uint32()
        _check(lib, lib.kp_filter_class_prices(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value * self.T), dtype=np.float64)
        _check(lib, lib.kp_filter_class_prices(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), out.size,
                                               C.byref(n)))
        return out[:n.value * self.T].reshape(n.value, self.T)

    @staticmethod
    def cheapest_from_compact(classes, class_prices):
        """min over the row's classes of the class price rows (+inf: none) = kp_filter_run's out_cheapest."""
        out = np.full((len(classes), class_prices.shape[1]), np.inf)
        for c in range(class_prices.shape[0]):
            sel = ((classes >> np.uint64(c)) & np.uint64(1)).astype(bool)
            out[sel] = np.minimum(out[sel], class_prices[c])
        return out

    def refresh(self, catalog):
        """kp_filter_refresh: re-apply the catalogue's current offerings (ICE / price) to the resident plan."""
        _check(self.ctx.lib, self.ctx.lib.kp_filter_refresh(self.h, catalog.h))

    def close(self):
        if self.h:
            self.ctx.lib.kp_filter_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MAX_LAUNCH_TYPES = 60  # maxInstanceTypes (R:pkg/providers/instance/instance.go:60)


def _read_templates(lib, call, n, max_types, zones, amis, instance_types):
    """Allocate kp_launch_templates' outputs, run call(out, out_types, lt_out, out_type_config, out_configs,
    out_overrides, stats) and read them: ([dict per request], stats)."""
    st = abi.SolveStats()
    stride = max_types * max(1, len(zones))
    out = (abi.LaunchResult * max(1, n))()
    types = np.zeros(max(1, n * max_types), dtype=np.uint32)
    lt = np.zeros(max(1, n), dtype=abi.lt_result_dtype())
    tcfg = np.zeros(max(1, n * max_types), dtype=np.int32)
    cfgs = np.zeros(max(1, n * stride), dtype=abi.lt_config_dtype())
    ovr = np.zeros(max(1, n * stride), dtype=np.uint32)
    _check(lib, call(out, types.ctypes.data_as(C.POINTER(C.c_uint32)), lt.ctypes.data, tcfg.ctypes.data, cfgs.ctypes.data,
                     ovr.ctypes.data, C.byref(st)))
    res = []
    for i in range(n):
        # (a launch result dict's overrides are kp_launch_run's flat list, which this call does not return: its length
        # stays, the overrides are the configs')
        base = abi.launch_result_dict(out[i], types[i * max_types:(i + 1) * max_types], ovr[:0], zones)
        del base["overrides"]
        base["n_overrides"] = int(out[i].n_overrides)
        res.append(abi.launch_templates_dict(base, lt[i], tcfg[i * max_types:(i + 1) * max_types],
                                             cfgs[i * stride:(i + 1) * stride], ovr[i * stride:(i + 1) * stride], zones,
                                             amis, instance_types))
    return res, stats_dict(st)


class LaunchPlan:
    """kp_launch_prepare / kp_launch_run: instance.DefaultProvider.Create's launch-side selection for a batch of
    NodeClaims (filters, Truncate, capacity type, CreateFleet overrides), requests resident on the device.
    requests: [(requirements, requests, [catalogue indices])]; subnet_zones: zones with a launch subnet."""

    def __init__(self, ctx, catalog, requests, subnet_zones, max_types=MAX_LAUNCH_TYPES):
        self.ctx = ctx
        self.catalog = catalog
        self.n = len(requests)
        self.zones = list(subnet_zones)
        self.max_types = max_types
        arena = Arena()
        rq = abi.launch_requests(arena, requests)
        zs = arena.arr(C.c_char_p, [z.encode() for z in self.zones])
        h = C.c_void_p()
        _check(ctx.lib, ctx.lib.kp_launch_prepare(ctx.h, catalog.h, rq, self.n, zs, len(self.zones), max_types,
                                                  C.byref(h)))
        self.h = h

    def run(self, read=True):
        """One launch; read=True returns ([result dict per request], stats), else (None, stats)."""
        st = abi.SolveStats()
        lib = self.ctx.lib
        if not read:
            _check(lib, lib.kp_launch_run(self.h, None, None, None, C.byref(st)))
            return None, stats_dict(st)
        out = (abi.LaunchResult * max(1, self.n))()
        stride = self.max_types * max(1, len(self.zones))
        types = np.zeros(max(1, self.n * self.max_types), dtype=np.uint32)
        ovr = np.zeros(max(1, self.n * stride), dtype=np.uint32)
        _check(lib, lib.kp_launch_run(self.h, out, types.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      ovr.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(st)))
        res = [abi.launch_result_dict(out[i], types[i * self.max_types:(i + 1) * self.max_types],
                                      ovr[i * stride:(i + 1) * stride], self.zones) for i in range(self.n)]
        return res, stats_dict(st)

    def templates(self, amis, read=True):
        """kp_launch_run_templates: one launch followed by the launch-template grouping on the device.
        amis: the EC2NodeClass's status.amis ([model.AMI], status order). read=True returns ([the run() dict plus
        lt_status, unmapped, dropped, configs per request], stats), else (None, stats)."""
        st = abi.SolveStats()
        lib, n = self.ctx.lib, self.n
        arena = Arena()
        am, n_amis = abi.amis(arena, amis)
        if not read:
            _check(lib, lib.kp_launch_run_templates(self.h, am, n_amis, None, None, None, None, None, None, C.byref(st)))
            return None, stats_dict(st)
        return _read_templates(lib, lambda *bufs: lib.kp_launch_run_templates(self.h, am, n_amis, *bufs), n, self.max_types,
                               self.zones, amis, self.catalog.instance_types)

    def refresh(self, catalog):
        """kp_launch_refresh: re-apply the catalogue's current offerings (ICE / price) to the resident plan."""
        _check(self.ctx.lib, self.ctx.lib.kp_launch_refresh(self.h, catalog.h))

    def close(self):
        if self.h:
            self.ctx.lib.kp_launch_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def launch_requests_from_solve(result):
    """One launch request per NodeClaim of a Solve result: its final requirements, requests and options."""
    reqs = []
    for n in result["nodeclaims"]:
        reqs.append((n["requirements"], n["requests"], n["options"]))
    return reqs


def pod_queries(problem):
    """One CompatibleAvailableFilter row per pod: NewPodRequirements (nodeSelector + heaviest preferred term +
    first required term) and the pod's requests."""
    rows = []
    for sh in problem.shapes:
        reqs = [(k, "In", [v]) for k, v in sh.node_selector.items()]
        if sh.preferred_terms:
            reqs += list(max(sh.preferred_terms, key=lambda t: t[0])[1])
        if sh.required_terms:
            reqs += list(sh.required_terms[0])
        rows.append((reqs, sh.requests))
    return [rows[int(s)] for s in problem.pod_shape]


def sim_dict(r):
    """kp_sim_result (ctypes struct or a record of abi.sim_dtype()) -> dict."""
    if isinstance(r, np.void):
        g, np_key = (lambda k: r[k]), "nodepool"
    else:
        g, np_key = (lambda k: getattr(r, k)), "replacement_nodepool"
    return {"decision": int(g("decision")), "nodepool": int(g(np_key)),
            "candidate_price": float(g("candidate_price")), "replacement_price": float(g("replacement_price")),
            "savings": float(g("savings")), "n_options": int(g("n_options")), "n_pods": int(g("n_pods"))}


class ClusterPlan:
    """Resident cluster snapshot for consolidation (kp_cluster_prepare); simulate() evaluates a batch of
    candidate subsets as computeConsolidation would (kp_cluster_simulate)."""

    def __init__(self, ctx, cluster, catalogs=None):
        import time
        self.ctx = ctx
        self.cluster = cluster
        t0 = time.perf_counter()
        self.catalogs = catalogs or [Catalog(ctx, c) for c in cluster.catalogs]
        t1 = time.perf_counter()
        arena = Arena()
        cl = abi.build_cluster(arena, cluster, catalog_handles=[c.h.value for c in self.catalogs])
        t2 = time.perf_counter()
        h = C.c_void_p()
        _check(ctx.lib, ctx.lib.kp_cluster_prepare(ctx.h, C.byref(cl), C.byref(h)))
        self.h = h
        # where the construction's time went: catalogue upload (when not passed in), this binding's marshalling of the
        # cluster into kp_cluster structs (a caller's shim builds those itself), and kp_cluster_prepare
        self.prepare_times = {"catalog_s": t1 - t0, "marshal_s": t2 - t1, "kp_cluster_prepare_s": time.perf_counter() - t2}

    def refresh(self):
        """kp_cluster_refresh: re-apply the catalogues' current offerings (after update_offerings) in place."""
        _check(self.ctx.lib, self.ctx.lib.kp_cluster_refresh(self.h))

    @staticmethod
    def _allowed(allowed):
        arr = np.ascontiguousarray(allowed, dtype=np.uint32)
        return arr, arr.ctypes.data_as(C.POINTER(C.c_uint32)), len(arr)

    def _simulate(self, cancel, offs, flat, n, multi_node, out, st, allowed):
        """kp_cluster_simulate_cancellable, or with allowed (disruption.allowed_disruptions) kp_cluster_simulate_budgeted;
        returns the stats dict (with budget_blocked when allowed is given)."""
        lib, ch = self.ctx.lib, cancel.h if cancel is not None else None
        if allowed is None:
            _check(lib, lib.kp_cluster_simulate_cancellable(self.h, ch, offs, flat, n, 1 if multi_node else 0, out,
                                                            C.byref(st)))
            return stats_dict(st)
        keep, ap, na = self._allowed(allowed)
        blocked = C.c_uint64(0)
        _check(lib, lib.kp_cluster_simulate_budgeted(self.h, ch, offs, flat, n, 1 if multi_node else 0, ap, na, out,
                                                     C.byref(blocked), C.byref(st)))
        return dict(stats_dict(st), budget_blocked=int(blocked.value))

    def simulate(self, subsets, multi_node=True, raw=False, cancel=None, allowed=None):
        """subsets: list of node-index lists (candidate order). Returns (results, stats); raw=True returns
        the kp_sim_result array instead of dicts. cancel: a Cancel token (kp_cluster_simulate_cancellable). allowed:
        allowed disruptions per NodePool (kp_cluster_simulate_budgeted; stats gain budget_blocked)."""
        arena = Arena()
        offs, flat = abi.subsets_csr(arena, subsets)
        out = (abi.SimResult * max(1, len(subsets)))()
        st = abi.SolveStats()
        sd = self._simulate(cancel, offs, flat, len(subsets), multi_node, out, st, allowed)
        if raw:
            return out, sd
        return [sim_dict(out[i]) for i in range(len(subsets))], sd

    def simulate_csr(self, offsets, nodes, multi_node=True, cancel=None, allowed=None):
        """CSR batch (uint32 offsets[n+1], node indices) -> numpy structured array (abi.sim_dtype()), stats. allowed: as
        simulate()."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        n = len(offsets) - 1
        out = np.zeros(max(n, 1), dtype=abi.sim_dtype())
        st = abi.SolveStats()
        P = C.POINTER
        sd = self._simulate(cancel, offsets.ctypes.data_as(P(C.c_uint32)),
                            nodes.ctypes.data_as(P(C.c_uint32)) if len(nodes) else None, n, multi_node,
                            out.ctypes.data_as(P(abi.SimResult)), st, allowed)
        return out[:n], sd

    def argmin(self, offsets, nodes, base_index=0, comm=None, multi_node=True, read_all=False, cancel=None,
               allowed=None):
        """kp_consolidate_argmin: this rank's subsets (CSR, global indices base_index + i) simulated, reduced on the
        device and across ranks (RCCL all-gather when comm is a Comm). Returns (choice dict, per-subset results
        or None, stats). cancel: a Cancel token (kp_consolidate_argmin_cancellable). allowed: allowed disruptions per
        NodePool (kp_consolidate_argmin_budgeted): the subsets over a pool's allowance are gated out on the device and
        stats gain budget_blocked (this rank's count)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        n = len(offsets) - 1
        out = np.zeros(max(n, 1), dtype=abi.sim_dtype()) if read_all else None
        ch = abi.Choice()
        st = abi.SolveStats()
        P = C.POINTER
        head = (self.h, comm.h if comm is not None else None, cancel.h if cancel is not None else None,
                offsets.ctypes.data_as(P(C.c_uint32)), nodes.ctypes.data_as(P(C.c_uint32)) if len(nodes) else None, n,
                int(base_index), 1 if multi_node else 0)
        outp = out.ctypes.data_as(P(abi.SimResult)) if out is not None else None
        if allowed is None:
            _check(self.ctx.lib, self.ctx.lib.kp_consolidate_argmin_cancellable(*head, outp, C.byref(ch), C.byref(st)))
            sd = stats_dict(st)
        else:
            keep, ap, na = self._allowed(allowed)
            blocked = C.c_uint64(0)
            _check(self.ctx.lib, self.ctx.lib.kp_consolidate_argmin_budgeted(*head, ap, na, outp, C.byref(ch),
                                                                             C.byref(blocked), C.byref(st)))
            sd = dict(stats_dict(st), budget_blocked=int(blocked.value))
        return choice_dict(ch), (out[:n] if out is not None else None), sd

    def drift(self, subsets, allowed=None, cancel=None, read_all=False):
        """kp_cluster_drift: every subset (list of node indices; Drift passes singletons) simulated as a whole Solve.
        Returns {"first": the lowest admissible feasible subset index or -1, "replacements": read_result of that subset's
        Solve (placements in the simulation's input order: pending, deleting nodes' pods, the subset's pods) or None,
        "results": the per-subset kp_drift_result dicts when read_all, "blocked": subsets the budget blocked (allowed:
        allowed disruptions per NodePool, reason Drifted), "stats"}."""
        lib = self.ctx.lib
        arena = Arena()
        offs, flat = abi.subsets_csr(arena, subsets)
        n = len(subsets)
        out = (abi.DriftResult * max(1, n))() if read_all else None
        first, res, blocked, st = C.c_int64(-1), C.c_void_p(), C.c_uint64(0), abi.SolveStats()
        keep, ap, na = self._allowed(allowed) if allowed is not None else (None, None, 0)
        _check(lib, lib.kp_cluster_drift(self.h, cancel.h if cancel is not None else None, offs, flat, n, ap, na, out,
                                         C.byref(first), C.byref(res), C.byref(blocked), C.byref(st)))
        try:
            repl = None
            if res.value:
                cl, w = self.cluster, subsets[first.value]
                n_pods = len(cl.pending) + sum(len(x.pods) for x in cl.nodes if x.deleting) + sum(len(cl.nodes[c].pods) for c in w)
                repl = read_result(lib, res, n_pods)
        finally:
            if res.value:
                lib.kp_result_destroy(res)
        results = None
        if read_all:
            results = [{f: int(getattr(out[i], f)) for f, _ in abi.DriftResult._fields_} for i in range(n)]
        return {"first": int(first.value), "replacements": repl, "results": results, "blocked": int(blocked.value),
                "stats": stats_dict(st)}

    def command(self, subsets, multi_node=True, allowed=None, cancel=None):
        """kp_cluster_command: simulate() plus each decision's command. Returns (results, commands, stats): results as
        simulate() gives them; commands[s] None for a no-op or a budget-blocked subset, else read_result of the command
        (the dict form drift() uses for "replacements": no NodeClaim for a DELETE, one for a REPLACE whose options are
        the ones the price filters kept; placements in the simulation's input order: pending, deleting nodes' pods, the
        subset's pods); stats gain budget_blocked when allowed is given."""
        lib = self.ctx.lib
        arena = Arena()
        offs, flat = abi.subsets_csr(arena, subsets)
        n = len(subsets)
        out = (abi.SimResult * max(1, n))()
        cmds = (C.c_void_p * max(1, n))()
        blocked, st = C.c_uint64(0), abi.SolveStats()
        keep, ap, na = self._allowed(allowed) if allowed is not None else (None, None, 0)
        _check(lib, lib.kp_cluster_command(self.h, cancel.h if cancel is not None else None, offs, flat, n,
                                           1 if multi_node else 0, ap, na, out, cmds, C.byref(blocked), C.byref(st)))
        commands = []
        try:
            cl = self.cluster
            n_base = len(cl.pending) + sum(len(x.pods) for x in cl.nodes if x.deleting)
            for s in range(n):
                if not cmds[s]:
                    commands.append(None)
                    continue
                commands.append(read_result(lib, C.c_void_p(cmds[s]), n_base + sum(len(cl.nodes[c].pods) for c in subsets[s])))
        finally:
            for s in range(n):
                if cmds[s]:
                    lib.kp_result_destroy(C.c_void_p(cmds[s]))
        sd = stats_dict(st)
        if allowed is not None:
            sd["budget_blocked"] = int(blocked.value)
        return [sim_dict(out[i]) for i in range(n)], commands, sd

    def validate(self, subsets, checks, allowed=None, cancel=None):
        """kp_cluster_validate on this plan, one prepared from CURRENT state: subsets[s] the candidates of a command
        (node indices of this plan's cluster), checks[s] what it decided: {"decision": abi.DECISION_DELETE} or
        {"decision": abi.DECISION_REPLACE, "options": [instance-type names]}. Returns (list of kp_validation dicts,
        stats); stats gain budget_blocked when allowed (the allowed disruptions per NodePool for the command's
        reason) is given."""
        lib = self.ctx.lib
        if len(checks) != len(subsets):
            raise ValueError("one check per subset")
        arena = Arena()
        offs, flat = abi.subsets_csr(arena, subsets)
        n = len(subsets)
        arr = (abi.CommandCheck * max(1, n))()
        keep = []
        for s, c in enumerate(checks):
            names = c.get("options") or []
            arr[s].decision = int(c["decision"])
            arr[s].n_options = len(names)
            if names:
                buf = (C.c_char_p * len(names))(*[None if x is None else x.encode() for x in names])
                keep.append(buf)
                arr[s].options = C.cast(buf, C.POINTER(C.c_char_p))
        out = (abi.Validation * max(1, n))()
        blocked, st = C.c_uint64(0), abi.SolveStats()
        keep_a, ap, na = self._allowed(allowed) if allowed is not None else (None, None, 0)
        _check(lib, lib.kp_cluster_validate(self.h, cancel.h if cancel is not None else None, offs, flat, n, arr, ap, na,
                                            out, C.byref(blocked), C.byref(st)))
        sd = stats_dict(st)
        if allowed is not None:
            sd["budget_blocked"] = int(blocked.value)
        return [{f: int(getattr(out[i], f)) for f, _ in abi.Validation._fields_} for i in range(n)], sd

    def simulate_explained(self, subsets, multi_node=True, allowed=None, cancel=None, records=True):
        """kp_cluster_simulate_explained: simulate() plus, per subset, which exit of computeConsolidation made it a
        no-op. Returns (sims, whys, counts, stats): sims as simulate() gives them (bit for bit kp_cluster_simulate_budgeted's),
        whys the kp_sim_why dicts (reason: abi.UNCONS_*), counts the abi.UNCONS_COUNT-entry histogram of the reasons;
        stats gain budget_blocked when allowed is given. records=False passes why = NULL: whys is None and only the
        histogram is read back."""
        lib = self.ctx.lib
        arena = Arena()
        offs, flat = abi.subsets_csr(arena, subsets)
        n = len(subsets)
        out = (abi.SimResult * max(1, n))()
        why = (abi.SimWhy * max(1, n))() if records else None
        counts = (C.c_uint64 * abi.UNCONS_COUNT)()
        blocked, st = C.c_uint64(0), abi.SolveStats()
        keep, ap, na = self._allowed(allowed) if allowed is not None else (None, None, 0)
        _check(lib, lib.kp_cluster_simulate_explained(self.h, cancel.h if cancel is not None else None, offs, flat, n,
                                                      1 if multi_node else 0, ap, na, out, why, counts, C.byref(blocked),
                                                      C.byref(st)))
        sd = stats_dict(st)
        if allowed is not None:
            sd["budget_blocked"] = int(blocked.value)
        return ([sim_dict(out[i]) for i in range(n)], [abi.why_dict(why[i]) for i in range(n)] if records else None,
                [int(c) for c in counts], sd)

    def candidates(self, method, now, controls=None):
        """kp_cluster_candidates for one method (abi.METHOD_*) at unix time now, on controls (default: the cluster's
        DisruptionControls). Returns (records, order, stats): records the numpy array of abi.candidate_dtype(), one per
        node (reason 0: a candidate); order the candidates' node indices in disruption order."""
        controls = self.cluster.controls if controls is None else controls
        if controls is None:
            raise ValueError("the cluster carries no DisruptionControls")
        arena = Arena()
        ci = abi.build_candidates_in(arena, controls, method, now)
        n = len(self.cluster.nodes)
        out = np.zeros(max(n, 1), dtype=abi.candidate_dtype())
        order = np.zeros(max(n, 1), dtype=np.uint32)
        count, st = C.c_uint32(0), abi.SolveStats()
        _check(self.ctx.lib, self.ctx.lib.kp_cluster_candidates(self.h, C.byref(ci), out.ctypes.data,
                                                                order.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                                C.byref(count), C.byref(st)))
        return out[:n], [int(x) for x in order[:count.value]], stats_dict(st)

    def detect_drift(self, inputs=None, records=True):
        """kp_cluster_detect_drift on inputs (default: the cluster's DriftInputs): IsDrifted for every node of the
        snapshot in one call. Returns (records, counts, stats): records the numpy array of abi.node_drift_dtype(), one
        per node (reason: abi.DRIFT_*, non-zero only when status is DRIFT_OK); counts the abi.DRIFT_REASON_COUNT-entry
        histogram of the reasons. records=False passes out = NULL: records is None and only the histogram is read back."""
        inputs = self.cluster.drift_inputs if inputs is None else inputs
        if inputs is None:
            raise ValueError("the cluster carries no DriftInputs")
        arena = Arena()
        di = abi.build_drift_in(arena, inputs)
        n = len(inputs.nodes)
        out = np.zeros(max(n, 1), dtype=abi.node_drift_dtype()) if records else None
        counts, st = (C.c_uint64 * abi.DRIFT_REASON_COUNT)(), abi.SolveStats()
        _check(self.ctx.lib, self.ctx.lib.kp_cluster_detect_drift(self.h, C.byref(di), out.ctypes.data if records else None,
                                                                  counts, C.byref(st)))
        return (out[:n] if records else None), [int(c) for c in counts], stats_dict(st)

    def interruptions(self, messages, node_ids, table_log2=0, raw=False):
        """kp_cluster_interruptions: messages [(kind abi.MSG_*, [instance id])] resolved against the snapshot's nodes,
        whose instance ids are node_ids (None: no provider id). Returns a dict: nodes [{first_message, kinds,
        n_messages, flags}] per node, matches [nodes matched] per (message, id) entry, deletes [{node, message, kind}]
        in node order, marks [{node, n_nodes}] in order of node, counts (deletes per kind) and stats. raw=True leaves
        nodes, matches, deletes and marks as the numpy arrays the call wrote. table_log2 forces the join's table size."""
        arena = Arena()
        ii = abi.build_interrupt_in(arena, messages, node_ids, table_log2)
        n, e = len(node_ids), int(ii.n_ids)
        nodes = np.zeros(max(n, 1), dtype=abi.interrupt_node_dtype())
        matches = np.zeros(max(e, 1), dtype=np.uint32)
        deletes = np.zeros(max(n, 1), dtype=abi.interrupt_delete_dtype())
        marks = np.zeros(max(n, 1), dtype=abi.interrupt_mark_dtype())
        nd, nm = C.c_uint32(0), C.c_uint32(0)
        counts, st = (C.c_uint64 * abi.MESSAGE_KIND_COUNT)(), abi.SolveStats()
        _check(self.ctx.lib, self.ctx.lib.kp_cluster_interruptions(self.h, C.byref(ii), nodes.ctypes.data,
                                                                   matches.ctypes.data, deletes.ctypes.data, C.byref(nd),
                                                                   marks.ctypes.data, C.byref(nm), counts, C.byref(st)))
        out = {"nodes": nodes[:n], "matches": matches[:e], "deletes": deletes[:nd.value], "marks": marks[:nm.value],
               "counts": [int(c) for c in counts], "stats": stats_dict(st)}
        if not raw:
            for key in ("nodes", "deletes", "marks"):
                out[key] = [{f: int(r[f]) for f in r.dtype.names if f != "reserved"} for r in out[key]]
            out["matches"] = [int(x) for x in out["matches"]]
        return out

    def close(self):
        if self.h:
            self.ctx.lib.kp_cluster_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def choice_dict(ch):
    return {"subset": int(ch.subset), "counts": [int(x) for x in ch.counts], "overflowed": int(ch.overflowed),
            "result": sim_dict(ch.result)}


def comm_unique_id(lib=None):
    """kp_comm_unique_id (rank 0): 128 bytes every rank passes to Comm."""
    lib = lib or load_lib()
    buf = C.create_string_buffer(abi.COMM_ID_BYTES)
    _check(lib, lib.kp_comm_unique_id(buf))
    return buf.raw


class Comm:
    """kp_comm: one rank of a communicator over the node's GPUs. Comm(ctx, uid, n, rank) is one rank of an RCCL
    communicator (kp_comm_init, collective, one process per GPU); Comm.init_all(ctxs) builds the n RCCL ranks of one
    process (kp_comm_init_all, one thread per GPU); Comm.host(ctx, n, rank, allgather) uses a host all-gather
    (kp_comm_init_host): allgather(rank, data: bytes) -> list of n bytes objects, blocking until every rank sent."""

    def __init__(self, ctx, uid=None, n_ranks=1, rank=0, _handle=None):
        self.ctx = ctx
        self._cb = None
        if _handle is not None:
            self.h = _handle
            return
        h = C.c_void_p()
        _check(ctx.lib, ctx.lib.kp_comm_init(ctx.h, bytes(uid), n_ranks, rank, C.byref(h)))
        self.h = h

    @classmethod
    def init_all(cls, ctxs):
        lib = ctxs[0].lib
        hs = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
        out = (C.c_void_p * len(ctxs))()
        _check(lib, lib.kp_comm_init_all(hs, len(ctxs), out))
        return [cls(c, _handle=C.c_void_p(out[i])) for i, c in enumerate(ctxs)]

    @classmethod
    def host(cls, ctx, n_ranks, rank, allgather):
        def fn(_user, r, send, recv, nbytes):
            try:
                parts = allgather(int(r), C.string_at(send, nbytes))
                C.memmove(recv, b"".join(parts), nbytes * n_ranks)
                return 0
            except Exception:  # the library turns a non-zero return into KP_E_DEVICE
                return 1
        cb = abi.AllGatherFn(fn)
        h = C.c_void_p()
        _check(ctx.lib, ctx.lib.kp_comm_init_host(ctx.h, n_ranks, rank, cb, None, C.byref(h)))
        c = cls(ctx, _handle=h)
        c._cb = cb  # keep the trampoline alive as long as the communicator
        return c

    def rank(self):
        r, n = C.c_int32(), C.c_int32()
        _check(self.ctx.lib, self.ctx.lib.kp_comm_rank(self.h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def close(self):
        if self.h:
            self.ctx.lib.kp_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ThreadAllGather:
    """In-process host all-gather for n threads (one per kp_ctx): the exchange step of Comm.host when the ranks
    are threads of one process (the one-goroutine-per-GPU pattern; tests run it on one GPU)."""

    def __init__(self, n):
        import threading
        self.n = n
        self.slots = [None] * n
        self.b1 = threading.Barrier(n)
        self.b2 = threading.Barrier(n)

    def __call__(self, rank, data):
        self.slots[rank] = data
        self.b1.wait(timeout=120)
        out = list(self.slots)
        self.b2.wait(timeout=120)
        return out


def torch_allgather(group=None):
    """Host all-gather over torch.distributed (e.g. gloo across processes) for Comm.host."""
    import torch
    import torch.distributed as dist

    def ag(rank, data):
        n = dist.get_world_size(group)
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        parts = [torch.empty_like(t) for _ in range(n)]
        dist.all_gather(parts, t, group=group)
        return [bytes(p.numpy().tobytes()) for p in parts]
    return ag


def choice_reduce(records, lib=None):
    """kp_choice_reduce over per-rank kp_choice records (the all-gather's host step)."""
    lib = lib or load_lib()
    arr = (abi.Choice * max(1, len(records)))(*records)
    out = abi.Choice()
    _check(lib, lib.kp_choice_reduce(arr, len(records), C.byref(out)))
    return out
