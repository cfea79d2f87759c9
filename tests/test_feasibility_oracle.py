"""CPU checks of the references the device filter tests (test_gpu_feasibility_edges.py) compare with: the batched
oracle filter equals the single-query entry bit for bit, and on every Fits-sweep input a numpy statement of
resources.Fits agrees with the oracle, so those inputs are known good before any device run."""
import ctypes as C

import numpy as np
import pytest

import feasibility_cases as fcases


def single_rows(its, queries):
    """kpo_filter_compatible_available (the single-query entry), once per row over one marshalled catalogue."""
    from kpamd import abi
    from oracle import pyoracle
    lib = pyoracle.load()
    arena = abi.Arena()
    desc = arena.catalog_desc(its)
    kept = np.zeros((len(queries), len(its)), dtype=np.uint8)
    cheapest = np.zeros((len(queries), len(its)), dtype=np.float64)
    for i, (r, q) in enumerate(queries):
        fq = abi.FeasibilityQuery(arena.requirements(r), arena.resources(q))
        assert lib.kpo_filter_compatible_available(C.byref(desc), C.byref(fq),
                                                   kept[i].ctypes.data_as(C.POINTER(C.c_uint8)),
                                                   cheapest[i].ctypes.data_as(C.POINTER(C.c_double))) == 0
    return kept.astype(bool), cheapest


def check_batch_equals_single(its, queries):
    from oracle import pyoracle
    kept, cheapest = pyoracle.compatible_available_filter_many(its, queries)
    assert kept.shape == cheapest.shape == (len(queries), len(its))
    want_k, want_c = single_rows(its, queries)
    assert np.array_equal(kept, want_k)
    assert np.array_equal(cheapest.view(np.uint64), want_c.view(np.uint64))  # bit for bit
    for i in (0, len(queries) - 1):  # and through the single-query wrapper
        k, c = pyoracle.compatible_available_filter(its, *queries[i])
        assert np.array_equal(kept[i], k) and np.array_equal(cheapest[i].view(np.uint64), c.view(np.uint64))
    return kept


def test_batch_equals_single_distinct_queries(catalog):
    from kpamd import synth
    kept = check_batch_equals_single(catalog, synth.distinct_queries(catalog, 64))
    assert kept.any() and not kept.all()


def test_batch_equals_single_reservation_requests(catalog):
    from test_reserved_offerings import reserved_catalogue, reserved_requests
    cat = reserved_catalogue(catalog, 300, 7)
    kept = check_batch_equals_single(cat, [(r, q) for r, q, _ in reserved_requests(cat, 40, 77)])
    assert kept.any() and not kept.all()


def test_batch_of_no_rows(catalog):
    from oracle import pyoracle
    kept, cheapest = pyoracle.compatible_available_filter_many(catalog[:5], [])
    assert kept.shape == cheapest.shape == (0, 5)


@pytest.mark.parametrize("case", fcases.FITS_CASES)
def test_fits_sweep_numpy_equals_oracle(lib, case):
    """Every row of every Fits sweep: numpy's alloc[t][r] >= need (with the non-negative rule and an available
    offering) == the batched oracle, masks and prices. The sub-catalogues have exactly the distinct memory allocatable
    counts their names say (the table alone stops at 168; see feasibility_cases._memory_pool)."""
    its, rows, kept, cheapest = fcases.fits_case(lib, case)
    if case.startswith("memory-"):
        assert fcases.distinct_count(its, "memory") == int(case.split("-")[1])
    else:
        assert fcases.distinct_count(its, "memory") == 168 and len(its) == 919
    want_k, want_c = fcases.numpy_filter(its, rows)
    bad = np.nonzero((kept != want_k).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} rows differ, first {rows[bad[0]]}"
    assert np.array_equal(cheapest, want_c)
    assert kept.any() and not kept.all()
    # a request equal to an allocatable value keeps that type, one above drops it
    a = fcases.alloc_matrix(its)[0]
    from kpamd import abi
    m = abi.RES_INDEX["memory"]
    if case != "full-other":
        v = int(a[:, m].max())
        at, above = rows.index(([], {"memory": v})), rows.index(([], {"memory": v + 1}))
        assert want_k[at].any() and not want_k[above].any()


def test_edge_catalogues_shapes(lib, catalog):
    """The catalogues the device edge tests are built on: sizes, the many-zone class count, the custom label share and
    the dictionary word count W (the device supports W <= 64)."""
    from kpamd import synth
    for n in (1, 64, 919, 1025, 1100):
        its = fcases.sized_catalog(lib, n)
        assert len(its) == n and len({t.name for t in its}) == n
    big = fcases.sized_catalog(lib, 1100)
    src = {t.name: t for t in big[:919]}
    for c in big[919:]:
        s = src[c.name.rsplit("-clone", 1)[0]]
        assert [r for r in c.requirements if r[0] != fcases.IT] == [r for r in s.requirements if r[0] != fcases.IT]
        assert c.capacity == s.capacity
        assert c.offerings[0].price != s.offerings[0].price or s.offerings[0].price == 0  # (0: no on-demand price)
    assert fcases.dict_words(catalog, synth.distinct_queries(catalog, 61)) == 47
    assert fcases.dict_words(big, synth.distinct_queries(big, 61)) == 50
    z4 = fcases.sized_catalog(lib, 65, zones=fcases.FOUR_ZONES[0], zone_ids=fcases.FOUR_ZONES[1])
    assert len({(o.capacity_type, o.zone) for t in z4 for o in t.offerings}) == 8  # > KP_SUB_MAX_C = 6 classes
    team = fcases.with_team_labels(catalog)
    n = sum(any(r[0] == fcases.TEAM for r in t.requirements) for t in team)
    assert abs(n - len(team) / 3) <= 1
    assert all(not o.available for t in fcases.all_unavailable(catalog[:10]) for o in t.offerings)
