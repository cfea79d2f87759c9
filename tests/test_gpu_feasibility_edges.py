"""The device CompatibleAvailableFilter (feasibility_quad_kernel<7> / <8>, feasibility_bits_kernel, feasibility_kernel)
== the batched CPU oracle on every row, whole arrays, at the shapes where the kernels change behaviour: Fits requests at
and next to every allocatable value (the lower bounds' >= edge, 1 / 2 / 16 / 17 / 256 / 257 distinct values), catalogue
sizes around the 64-type words, the 512-type copy halves and the 1,024-type dispatch, row counts around the 28- and
32-row blocks, and the requirement branches (custom labels, the complement walk's tie, bounds, the class-price fallback
past KP_SUB_MAX_C classes, no available offering).

Prices are compared on every type, its mask bit set or not: kp_abi.h defines out_cheapest (and the compact result's
class minima) as the cheapest available offering among the query's compatible classes for every type, which is what the
oracle computes per type. Equality is exact: mask bits and copied doubles.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import feasibility_cases as fcases

pytestmark = pytest.mark.gpu

MODES = [("prices", True), ("mask", False), ("compact", "compact")]
KERNELS = [0, 1, 2]  # kp_overrides.feasibility_kernel: the production choice, per-type, one row per wave (bits)


def expected_launch(T, kernel, mode):
    """kp_solve_stats.phase_cycles[0] of a filter run: 1 per-type, 2 bits, 3 quad with copy wave, 4 quad all-eval."""
    if kernel == 1:
        return 1
    if kernel == 2 or T > 1024:
        return 2
    return 3 if mode == "prices" else 4


def assert_rows(what, got_k, want_k, got_c=None, want_c=None):
    assert got_k.shape == want_k.shape, what
    bad = np.nonzero((got_k != want_k).any(axis=1))[0]
    if len(bad):
        t = np.nonzero(got_k[bad[0]] != want_k[bad[0]])[0]
        raise AssertionError(f"{what}: masks differ on {len(bad)} rows, first row {bad[0]}, types {t[:8].tolist()} "
                             f"(device {got_k[bad[0]][t[:8]].tolist()})")
    if got_c is not None:
        bad = np.nonzero((got_c != want_c).any(axis=1))[0]
        if len(bad):
            t = np.nonzero(got_c[bad[0]] != want_c[bad[0]])[0]
            raise AssertionError(f"{what}: prices differ on {len(bad)} rows, first row {bad[0]}, types {t[:8].tolist()}: "
                                 f"{got_c[bad[0]][t[:8]].tolist()} vs {want_c[bad[0]][t[:8]].tolist()}")


def check_filter(ctx, ov, its, queries, want=None, kernels=KERNELS):
    """The rows through a FilterPlan in all three result modes on each kernel, every row of every array against the
    oracle; the kernel each run launched is the one its shape calls for. Returns {(kernel, mode): launched}, the
    oracle's (kept, cheapest) and the class count."""
    import kpamd
    from oracle import pyoracle
    want_k, want_c = want if want is not None else pyoracle.compatible_available_filter_many(its, queries)
    T = len(its)
    cat = kpamd.Catalog(ctx, its)
    launched, n_classes = {}, None
    try:
        for kernel in kernels:
            ov(feasibility_kernel=kernel)
            for mode, flag in MODES:
                what = f"T={T} n={len(queries)} kernel={kernel} {mode}"
                fp = kpamd.FilterPlan(ctx, cat, queries, cheapest=flag)
                try:
                    if mode == "compact":
                        k, cls, st = fp.run_compact(read=True)
                        prices = fp.class_prices()
                        n_classes = prices.shape[0]
                        c = kpamd.FilterPlan.cheapest_from_compact(cls, prices)
                    else:
                        k, c, st = fp.run(read=True)
                        assert (c is None) == (mode == "mask")
                finally:
                    fp.close()
                assert_rows(what, k, want_k, c, want_c)
                assert st["attempts"] == len(queries) * T
                launched[(kernel, mode)] = st["phase_cycles"][0]
                assert launched[(kernel, mode)] == expected_launch(T, kernel, mode), what
    finally:
        cat.close()
    return launched, (want_k, want_c), n_classes


# ---- a. Fits thresholds ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fcases.FITS_CASES)
def test_fits_thresholds(ctx, ov, lib, case):
    """Requests v - 1, v, v + 1 for every distinct allocatable v, 1, max + 1, 1 << 62, and rows asking two to five
    resources at once, against two references: numpy's alloc >= need and the oracle. full-*: the whole catalogue (168
    distinct memory allocatables); memory-N: a sub-catalogue with exactly N (asserted), N = 256 / 257 reached with
    cloned rows of new memory sizes, no resource of the table having that many distinct values."""
    its, rows, kept, cheapest = fcases.fits_case(lib, case)
    if case.startswith("memory-"):
        assert fcases.distinct_count(its, "memory") == int(case.split("-")[1])
    want_k, want_c = fcases.numpy_filter(its, rows)
    assert np.array_equal(want_k, kept) and np.array_equal(want_c, cheapest)
    check_filter(ctx, ov, its, rows, want=(want_k, want_c))


# ---- b. catalogue sizes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_types", fcases.SIZES)
def test_catalogue_sizes(ctx, ov, lib, n_types):
    """61 distinct rows (two full 28-row blocks, one full and one partial quad) at every size where the kernels switch:
    one type, the 64-type words, the 512-type halves of the copy waves, the 1,024-type dispatch and past it, where
    feasibility_bits_kernel is the production kernel (TW = 17, 18). Every size compiles: the dictionary needs W = 47
    words at 919 types and 50 at 1,100 (of 64), so KP_E_UNSUPPORTED is never met up to the largest size run, 1,100."""
    from kpamd import synth
    its = fcases.sized_catalog(lib, n_types)
    queries = synth.distinct_queries(its, 61)
    assert fcases.dict_words(its, queries) <= 64
    launched, (want_k, _), _ = check_filter(ctx, ov, its, queries)
    assert want_k.any() and not want_k.all()
    if n_types == 1024:
        assert launched[(0, "prices")] == 3 and launched[(0, "mask")] == 4 and launched[(0, "compact")] == 4
    if n_types == 1025:
        assert set(launched[(0, m)] for m, _ in MODES) == {2}


# ---- c. row counts ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _row_count_reference(lib):
    from kpamd import catalog as cmod, synth
    from oracle import pyoracle
    its = cmod.build_catalog(lib)
    queries = synth.distinct_queries(its, 65)
    k, c = pyoracle.compatible_available_filter_many(its, queries)
    k.setflags(write=False)
    c.setflags(write=False)
    return its, queries, k, c


@pytest.mark.parametrize("n", [1, 4, 27, 28, 29, 31, 32, 33, 56, 57, 64, 65])
def test_row_counts(ctx, ov, lib, n):
    """Row counts around one quad (4), the price-row block (28) and the mask-only / compact block (32), 919 types."""
    its, queries, k, c = _row_count_reference(lib)
    launched, _, _ = check_filter(ctx, ov, its, queries[:n], want=(k[:n], c[:n]))
    assert launched[(0, "prices")] == 3 and launched[(0, "mask")] == 4 and launched[(0, "compact")] == 4


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_no_rows(ctx, catalog, mode):
    """n = 0: KP_OK, nothing launched, the caller's buffers untouched."""
    import kpamd
    from kpamd import abi
    lib = ctx.lib
    cat = kpamd.Catalog(ctx, catalog[:70])
    fp = kpamd.FilterPlan(ctx, cat, [], cheapest={0: False, 1: True, 2: "compact"}[mode])
    try:
        mask = np.full(4, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        price = np.full(140, -7.0)
        cls = np.full(2, 0x5A5A, dtype=np.uint64)
        st = abi.SolveStats()
        if mode == 2:
            rc = lib.kp_filter_run_compact(fp.h, mask.ctypes.data_as(C.POINTER(C.c_uint64)),
                                           cls.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(st))
        else:
            rc = lib.kp_filter_run(fp.h, mask.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   price.ctypes.data_as(C.POINTER(C.c_double)) if mode == 1 else None, C.byref(st))
        assert rc == 0
        assert st.phase_cycles[0] == 0 and st.attempts == 0
        assert (mask == 0xA5A5A5A5A5A5A5A5).all() and (price == -7.0).all() and (cls == 0x5A5A).all()
    finally:
        fp.close()
        cat.close()


# ---- d. requirement edges --------------------------------------------------------------------------------------------
def test_custom_label_rows(ctx, ov, catalog):
    """About a third of the types carry example.com/team In {a} / {b} (the custom_any & ~present branch): rows that omit
    the key and rows with In / NotIn / Exists / DoesNotExist on it; with them the arch tie of the complement walk
    (amd64 against arm64: nE == nA), instance-type In / NotIn with 1, half and all but one of its 919 values (a 15-word
    key), instance-cpu Gt / Lt at and beyond its range and an empty range, Exists / DoesNotExist on
    instance-gpu-manufacturer."""
    its = fcases.with_team_labels(catalog)
    queries = fcases.requirement_edge_queries(its)
    _, (want_k, _), _ = check_filter(ctx, ov, its, queries)
    n = want_k.sum(axis=1)
    assert n[0] < n[1] < n[3] and n[7] == n[3] and n[8] == n[0]  # no key < In {a} < In {a, b} == Exists; DNE == no key
    assert (n == 0).any() and (n == 1).any()


def test_requirement_edges_plain_catalogue(ctx, ov, catalog):
    """The same rows on the catalogue without the label (custom_any == 0: the branch is skipped; the rows that name the
    key meet no type that defines it)."""
    check_filter(ctx, ov, catalog, fcases.requirement_edge_queries(catalog))


@pytest.mark.parametrize("n_types", [65, 513, 919])
def test_many_zone_price_fallback(ctx, ov, lib, n_types):
    """Four zones: 8 offering classes > KP_SUB_MAX_C, so no class-subset price table exists (price_sub null) and the
    price rows are the min over the row's classes' price rows: the quad kernel's copy waves, the bits kernel and the
    per-type kernel."""
    from kpamd import synth
    zones, zone_ids = fcases.FOUR_ZONES
    its = fcases.sized_catalog(lib, n_types, zones=zones, zone_ids=zone_ids)
    queries = synth.distinct_queries(its, 61) + [
        ([("topology.kubernetes.io/zone", "In", [zones[3]])], {"cpu": 500}),
        ([("topology.kubernetes.io/zone", "NotIn", zones[:3]), ("karpenter.sh/capacity-type", "In", ["spot"])], {"cpu": 500}),
        ([("topology.k8s.aws/zone-id", "In", [zone_ids[3], zone_ids[0]])], {"cpu": 500})]
    _, (want_k, want_c), n_classes = check_filter(ctx, ov, its, queries)
    assert n_classes == 8 and n_classes > 6
    assert want_k.any() and not want_k.all() and np.isfinite(want_c).any()
    assert want_k[-3:].any(axis=1).all()  # the rows that name the fourth zone keep types


def test_every_offering_unavailable(ctx, ov, lib):
    """No available offering anywhere: every mask is zero and every price +inf, in every mode on every kernel."""
    from kpamd import synth
    its = fcases.all_unavailable(fcases.sized_catalog(lib, 130))
    _, (want_k, want_c), _ = check_filter(ctx, ov, its, synth.distinct_queries(its, 33))
    assert not want_k.any() and np.isposinf(want_c).all()
