"""OrderByPrice + Truncate on the device at price ties and size edges. Every result ends in this step:
order the remaining instance types by (cheapest compatible available offering, name), cut to max types, re-check
minValues. The device has three copies of it: finalize_nodeclaim (256-thread bitonic sort; the Solve, the general
consolidation path, Drift), sim_kernel's wave_bitonic_kv (batched consolidation and the command) and launch_kernel.
All three compare prices as their bit patterns, pack the name rank above the type index, and pad the list to a power of
two with keys that must sort last.

Every case is a builder in tests/option_order_cases.py, a CPU-only *_inputs test that proves from the oracle and the
plain Python sort (plain_options, which shares nothing with oracle.cpp or the device encoding) that the input is the
edge it claims to be, and a gpu test that holds the device to it. No asserted value comes from the device; lists are
compared with ==, in order."""
import math
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import command_ref  # noqa: E402
import drift_ref  # noqa: E402
import option_order_cases as oc  # noqa: E402

_BUILT, _SOLVED, _CLUSTERS = {}, {}, {}


def _built(lib, builder, *args):
    """A builder's return, once per process."""
    key = (builder.__name__,) + args
    if key not in _BUILT:
        _BUILT[key] = builder(lib, *args)
    return _BUILT[key]


def _solved(lib, max_types, builder, *args):
    """(catalogues, claims, Problem, oracle result) of a Solve builder at one max_instance_types, once per process."""
    from oracle import pyoracle
    key = (builder.__name__, max_types) + args
    if key not in _SOLVED:
        cats, claims = _built(lib, builder, *args)[:2]
        prob = oc.solve_problem(cats, claims, max_types, f"{builder.__name__}-{max_types}")
        _SOLVED[key] = (cats, claims, prob, pyoracle.solve(prob))
    return _SOLVED[key]


def _hold_solve(ctx, prob, want):
    import kpamd
    from test_gpu_parity import check_same
    got = kpamd.Scheduler(ctx, prob).solve()
    check_same(got, want)
    return got


def _names(its, ts):
    return [its[t].name for t in ts]


def _keys(its, ts, zones=(oc.ZA,), cts=oc.OD):
    return [oc.cheapest(its[t], zones, cts) for t in ts]


# ---- A. option-count edges in the Solve (finalize_kernel<false>) ----------------------------------------------------
A_PARAMS = [(z, m) for z in (3, 4) for m in (100, 0, 1, 101)]


def _pre_counts(cats, claims, want, n_zones, max_types):
    assert oc.offering_classes(cats[0]) == 2 * n_zones  # 6: the subset-minimum table; 8: the loop over class rows
    assert len(cats[0]) == 1100 and len(claims[-1]["types"]) > 1025
    got = oc.by_claim(want)
    wanted = oc.COUNTS + [len(claims[-1]["types"])]
    assert [got[i]["n_remaining"] for i in range(len(claims))] == wanted
    assert [len(got[i]["options"]) for i in range(len(claims))] == [min(n, max_types) if max_types else n for n in wanted]
    oc.assert_plain(cats, claims, max_types, want)
    for i, n in enumerate(wanted):  # every list past five types is a tie case: fewer distinct keys than options
        if n >= 5 and max_types != 1:
            assert len(set(_keys(cats[0], got[i]["options"]))) < len(got[i]["options"])


@pytest.mark.parametrize("n_zones,max_types", A_PARAMS)
def test_counts_inputs(lib, n_zones, max_types):
    cats, claims, _, want = _solved(lib, max_types, oc.build_counts, n_zones)
    _pre_counts(cats, claims, want, n_zones, max_types)


@pytest.mark.gpu
@pytest.mark.parametrize("n_zones,max_types", A_PARAMS)
def test_counts(ctx, lib, n_zones, max_types):
    """One launch finalizes NodeClaims of 1 to 1,087 remaining types side by side: 64-lane and 256-thread boundaries,
    powers of two and one past them; max_instance_types 0 returns every list whole (the option rows' stride is T)."""
    cats, claims, prob, want = _solved(lib, max_types, oc.build_counts, n_zones)
    _pre_counts(cats, claims, want, n_zones, max_types)
    oc.assert_plain(cats, claims, max_types, _hold_solve(ctx, prob, want))


def _pre_two_catalogues(cats, claims, want, max_types):
    small, large = cats
    assert len(small) == 65 and len(large) == 1100
    a, b = claims[0]["types"], claims[1]["types"]
    assert _names(small, a) == _names(large, b)
    assert _keys(small, a) != _keys(large, b)  # the same names, other prices
    oc.assert_plain(cats, claims, max_types, want)
    got = oc.by_claim(want)
    assert _names(small, got[0]["options"]) != _names(large, got[1]["options"])


@pytest.mark.parametrize("max_types", [100, 0])
def test_two_catalogues_inputs(lib, max_types):
    cats, claims, _, want = _solved(lib, max_types, oc.build_two_catalogues)
    _pre_two_catalogues(cats, claims, want, max_types)


@pytest.mark.gpu
@pytest.mark.parametrize("max_types", [100, 0])
def test_two_catalogues(ctx, lib, max_types):
    cats, claims, prob, want = _solved(lib, max_types, oc.build_two_catalogues)
    _pre_two_catalogues(cats, claims, want, max_types)
    oc.assert_plain(cats, claims, max_types, _hold_solve(ctx, prob, want))


# ---- B. ties and price values ---------------------------------------------------------------------------------------
def _pre_all_equal(lib, cats, claims, want, max_types):
    its, ts = cats[0], claims[0]["types"]
    assert len(ts) == oc.N_EQUAL and len(set(_keys(its, ts))) == 1
    opts = oc.by_claim(want)[0]["options"]
    assert len(opts) == (max_types or oc.N_EQUAL)
    assert opts != sorted(opts) and opts != sorted(opts, reverse=True)  # neither index order nor its reverse
    names = _names(its, opts)
    assert names == sorted(names, key=str.encode)
    at = {n: i for i, n in enumerate(names)}
    assert at["c5.large-clone10"] < at["c5.large-clone9"] and at["c5.12xlarge"] < at["c5.2xlarge"] < at["c5.metal"]
    idx = {its[t].name: t for t in ts}  # ... against the catalogue's index order
    assert idx["c5.large-clone10"] > idx["c5.large-clone9"] and idx["c5.12xlarge"] > idx["c5.2xlarge"]


def _pre_signed_zeros(lib, cats, claims, want, max_types):
    its, ts = cats[0], claims[0]["types"]
    signs = {math.copysign(1.0, k) for k in _keys(its, ts)}
    assert signs == {1.0, -1.0} and set(_keys(its, ts)) == {0.0}
    same = _solved(lib, max_types, oc.build_all_equal, 0.0)  # ... and the list is that of +0.0 throughout
    assert _names(its, oc.by_claim(want)[0]["options"]) == _names(same[0][0], oc.by_claim(same[3])[0]["options"])


def _pre_tie_across_cut(lib, cats, claims, want, max_types):
    its, ts = cats[0], claims[0]["types"]
    full = oc.plain_options(its, ts, [oc.ZA], oc.OD, 0)
    keys = _keys(its, full)
    assert len(set(keys[89:115])) == 1 and keys[88] < keys[89] and keys[114] < keys[115]  # positions 90 to 115
    assert len(set(keys[:89])) == 89
    group = sorted(full[89:115], key=lambda t: its[t].name.encode())
    opts = oc.by_claim(want)[0]["options"]
    assert opts[89:] == group[:11] and group[:11] != sorted(full[89:115])[:11]  # the name decides, not the index


def _pre_ulp(lib, cats, claims, want, max_types):
    its, ts = cats[0], claims[0]["types"]
    keys = _keys(its, ts)
    assert len(set(keys)) == len(keys) == 18
    assert len(set(np.float32(keys).tolist())) < len(keys)  # float32 cannot tell them apart
    assert keys != sorted(keys) and keys != sorted(keys, reverse=True)
    opts = oc.by_claim(want)[0]["options"]
    assert _keys(its, opts) == sorted(keys)
    srt = sorted(keys)
    assert sum(math.nextafter(a, math.inf) == b for a, b in zip(srt, srt[1:])) == 16  # two chains of nine, one ulp apart


def _pre_extremes(lib, cats, claims, want, max_types):
    its = cats[0]
    keys = _keys(its, claims[0]["types"])
    scale = [o.price for it in its for o in it.offerings if o.reservation_id is not None]
    assert len(scale) == oc.N_RESERVED and all(0.0 < p < 1e-5 for p in scale)
    assert {0.0, oc.SUBNORMAL, 2 * oc.SUBNORMAL, 1e300, 1.0} | set(scale) == set(keys)
    got = oc.by_claim(want)
    assert got[1]["n_remaining"] == oc.N_RESERVED  # the reserved-only claim: keyed by the reserved offerings' prices
    assert sorted(_keys(its, got[1]["options"], cts=("reserved",))) == sorted(scale)


def _pre_zone_reversal(lib, cats, claims, want, max_types):
    its, ts = cats[0], claims[0]["types"]
    got = oc.by_claim(want)
    a, b = got[0]["options"], got[1]["options"]
    assert ts[0] not in a and ts[0] in b and len(a) == 99 and len(b) == 100  # unavailable in A: gone, not repriced
    assert oc.cheapest(its[ts[0]], [oc.ZB, oc.ZC], oc.OD) < 1e308
    assert a == [t for t in reversed(b) if t != ts[0]]  # mutually reversed
    zones = [oc.ZA, oc.ZB, oc.ZC]
    by_min = oc.plain_options(its, [t for t in ts if t != ts[0]], zones, oc.OD, 0)
    assert by_min != a and by_min != a[::-1]  # the order by the cheapest offering of any zone is neither


B_CASES = {"all-equal": (oc.build_all_equal, _pre_all_equal), "signed-zeros": (oc.build_signed_zeros, _pre_signed_zeros),
           "tie-across-cut": (oc.build_tie_across_cut, _pre_tie_across_cut), "ulp": (oc.build_ulp, _pre_ulp),
           "extremes": (oc.build_extremes, _pre_extremes), "zone-reversal": (oc.build_zone_reversal, _pre_zone_reversal)}
B_PARAMS = [("all-equal", 100), ("all-equal", 0), ("signed-zeros", 100), ("tie-across-cut", 100), ("ulp", 100),
            ("extremes", 100), ("extremes", 0), ("zone-reversal", 100)]


def _pre_b(lib, which, max_types):
    build, pre = B_CASES[which]
    cats, claims, prob, want = _solved(lib, max_types, build)
    oc.assert_plain(cats, claims, max_types, want)
    pre(lib, cats, claims, want, max_types)
    return cats, claims, prob, want


@pytest.mark.parametrize("which,max_types", B_PARAMS)
def test_ties_inputs(lib, which, max_types):
    _pre_b(lib, which, max_types)


@pytest.mark.gpu
@pytest.mark.parametrize("which,max_types", B_PARAMS)
def test_ties(ctx, lib, which, max_types):
    cats, claims, prob, want = _pre_b(lib, which, max_types)
    oc.assert_plain(cats, claims, max_types, _hold_solve(ctx, prob, want))


def _families(its, ts):
    return {next(r[2][0] for r in its[t].requirements if r[0] == oc.FAMILY) for t in ts}


def _pre_min_values_tie(lib, swapped):
    cats, claims, k, x, y = _built(lib, oc.build_min_values_tie, swapped)
    _, _, prob, want = _solved(lib, 100, oc.build_min_values_tie, swapped)
    its, ts = cats[0], claims[0]["types"]
    full = oc.plain_options(its, ts, [oc.ZA], oc.OD, 0)
    assert len(full) == 101 and set(full[99:]) == {x, y}  # positions 100 and 101 ...
    assert len(set(_keys(its, full[99:]))) == 1 and _keys(its, full)[98] < _keys(its, full)[99]  # ... tie on price
    assert len(_families(its, full)) == k and len(_families(its, full[:99])) == k - 1
    assert _families(its, [x]) - _families(its, full[:99]) and _families(its, [y]) <= _families(its, full[:99])
    if not swapped:
        assert full[99] == x
        oc.assert_plain(cats, claims, 100, want)
        assert len(_families(its, oc.by_claim(want)[0]["options"])) == k
    else:  # the cut keeps Y: k - 1 families, the NodeClaim's pod fails as in SolveCore
        assert full[99] == y and len(_families(its, full[:100])) == k - 1
        assert list(want["placement"]) == [-1] and [n["options"] for n in want["nodeclaims"]] == [[]]
    return prob, want


@pytest.mark.parametrize("swapped", [False, True])
def test_min_values_tie_inputs(lib, swapped):
    _pre_min_values_tie(lib, swapped)


@pytest.mark.gpu
@pytest.mark.parametrize("swapped", [False, True])
def test_min_values_tie(ctx, lib, swapped):
    """A price tie at the cut decides minValues by the name alone: the NodeClaim stands or its pod fails."""
    _hold_solve(ctx, *_pre_min_values_tie(lib, swapped))


# ---- C. batched consolidation and the command (sim_kernel) ----------------------------------------------------------
def _cluster_case(lib, builder, spread=False):
    """(cluster, subsets, types by intended position, reference per multi_node) with the oracle Solves shared."""
    key = (builder.__name__, spread)
    if key not in _CLUSTERS:
        cl, subs, ts = builder(lib, spread)
        solves, refs = {}, {}

        def ref(multi_node, subsets=None):
            k = (multi_node, None if subsets is None else tuple(map(tuple, subsets)))
            if k not in refs:
                refs[k] = command_ref.reference(cl, subs if subsets is None else subsets, multi_node, solves=solves)
            return refs[k]
        _CLUSTERS[key] = (cl, subs, ts, ref)
    return _CLUSTERS[key]


def _options(cmd):
    return [int(t) for t in cmd["nodeclaims"][0]["options"]]


def _agrees_with_oracle(cl, subs, multi_node, sims):
    from oracle import pyoracle
    assert sims == pyoracle.simulate_batch(cl, subs, multi_node=multi_node)[0]


def _pre_price_boundary(lib, spread=False):
    cl, subs, ts, ref = _cluster_case(lib, oc.build_price_boundary, spread)
    for multi_node in (False, True):
        sims, cmds, infos = ref(multi_node)
        _agrees_with_oracle(cl, subs, multi_node, sims)
        opts, kept, worst = oc.plain_kept(cl, ts, len(ts), oc.P)
        info = infos[0]
        assert sims[0]["decision"] == command_ref.REPLACE and sims[0]["candidate_price"] == oc.P
        assert cmds[0]["nodeclaims"][0]["n_remaining"] == 140 and info["truncated"] == 100 == len(opts)
        assert {oc.ULP_DOWN, oc.P, oc.ULP_UP} <= {worst[t] for t in opts}  # all three inside the cut
        assert info["after_price"] == len(kept) < info["truncated"] and info["price_hole"]
        assert _options(cmds[0]) == kept and max(worst[t] for t in kept) == oc.ULP_DOWN
    return cl, subs, ref


def test_price_boundary_inputs(lib):
    _pre_price_boundary(lib)


def _pre_same_type(lib, spread=False):
    cl, subs, ts, ref = _cluster_case(lib, oc.build_same_type, spread)
    its = cl.catalogs[0]
    x = cl.nodes[0].instance_type
    for multi_node in (False, True):
        sims, cmds, infos = ref(multi_node)
        _agrees_with_oracle(cl, subs, multi_node, sims)
        opts, kept3, worst = oc.plain_kept(cl, ts, len(ts), 3.0, pods=2)
        assert subs[0] == [0, 1] and sims[0]["candidate_price"] == 3.0 and x in opts and worst[x] == oc.P
        assert infos[0]["truncated"] == 100 and infos[0]["after_price"] == 100 == len(kept3)
        if multi_node:  # X's own price caps the list: strictly below P stays
            capped = [t for t in opts if worst[t] < oc.P]
            assert infos[0]["after_same_type"] == len(capped) == 90 and _options(cmds[0]) == capped
            assert max(worst[t] for t in capped) == oc.ULP_DOWN and sum(worst[t] == oc.P for t in opts) == 7
        else:
            assert _options(cmds[0]) == opts
        assert its[x].name in _names(its, opts)
    return cl, subs, ref


def test_same_type_inputs(lib):
    _pre_same_type(lib)


def _pre_lengths(lib, spread=False):
    cl, subs, ts, ref = _cluster_case(lib, oc.build_lengths, spread)
    sims, cmds, infos = ref(False)
    _agrees_with_oracle(cl, subs, False, sims)
    for n, sim, cmd, info in zip(oc.LENGTHS, sims, cmds, infos):
        opts, kept, worst = oc.plain_kept(cl, ts, n, oc.P)
        assert sim["decision"] == command_ref.REPLACE
        assert cmd["nodeclaims"][0]["n_remaining"] == n and info["truncated"] == min(n, 100) == len(opts)
        assert _options(cmd) == kept and info["price_hole"] == (n > 10)
        keys = [oc.cheapest(cl.catalogs[0][t], [oc.ZA, oc.ZB, oc.ZC], oc.OD) for t in opts]
        if n > 64:
            assert keys[59] < keys[60] == keys[63] == keys[64]  # a tie over lane 64 ...
            assert n < 71 or keys[64] == keys[69] < keys[70]  # ... of ten
        if n > 100:
            full = oc.plain_options(cl.catalogs[0], ts[:n], [oc.ZA, oc.ZB, oc.ZC], oc.OD, 0)
            fk = [oc.cheapest(cl.catalogs[0][t], [oc.ZA, oc.ZB, oc.ZC], oc.OD) for t in full]
            assert fk[94] < fk[95] == fk[99] == fk[100] == fk[110]  # a tie over the cut
    assert sorted(len(_options(c)) for c in cmds)[0] == 1 and {63, 64, 65, 100} <= {i["truncated"] for i in infos}
    return cl, subs, ref


def test_lengths_inputs(lib):
    _pre_lengths(lib)


def _hold_command(plan, cl, subs, multi_node, want):
    """plan.command against the reference in every field, and plan.simulate against it bit for bit."""
    from test_gpu_command import _bits
    sims_w, cmds_w, _ = want
    sims, cmds, st = plan.command(subs, multi_node=multi_node)
    assert sims == sims_w
    for s, (g, w) in enumerate(zip(cmds, cmds_w)):
        assert command_ref.command_fields(g) == command_ref.command_fields(w), f"{cl.name} subset {s} {subs[s]}"
    plain, _ = plan.simulate(subs, multi_node=multi_node)
    assert [_bits(d) for d in plain] == [_bits(d) for d in sims_w]
    return st


@pytest.fixture(scope="module")
def plans(ctx):
    """ClusterPlans by (builder, spread), compiled once per module."""
    import kpamd
    made = {}

    def get(lib, builder, spread=False):
        key = (builder.__name__, spread)
        if key not in made:
            made[key] = kpamd.ClusterPlan(ctx, _cluster_case(lib, builder, spread)[0])
        return made[key]
    yield get
    for p in made.values():
        p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("multi_node", [False, True])
def test_price_boundary(lib, plans, multi_node):
    """filterByPrice is strict: with P - ulp, P and P + ulp inside the cut, only what is below P stays."""
    cl, subs, ref = _pre_price_boundary(lib)
    _hold_command(plans(lib, oc.build_price_boundary), cl, subs, multi_node, ref(multi_node))


@pytest.mark.gpu
@pytest.mark.parametrize("multi_node", [False, True])
def test_same_type(lib, plans, multi_node):
    cl, subs, ref = _pre_same_type(lib)
    _hold_command(plans(lib, oc.build_same_type), cl, subs, multi_node, ref(multi_node))


@pytest.mark.gpu
@pytest.mark.parametrize("multi_node", [False, True])
def test_lengths(lib, plans, multi_node):
    """Lists of 1, 63, 64, 65 and 100 options and remaining sets of 127, 128, 129 and 513 in one call."""
    cl, subs, ref = _pre_lengths(lib)
    _hold_command(plans(lib, oc.build_lengths), cl, subs, multi_node, ref(multi_node))


@pytest.mark.gpu
def test_lengths_slot_reuse(lib, plans, ov):
    """sim_slots 4: every wave runs several subsets in a row in one slot. The subsets repeat in two arrangements, so
    that a long list is followed by the one-option list in the same slot whether a slot takes every fourth subset or a
    run of consecutive ones."""
    cl, subs, ref = _pre_lengths(lib)
    long_, one = oc.LENGTHS.index(513), oc.LENGTHS.index(1)
    order = []
    for i in range(len(subs)):  # by fours: long x 4, one x 4, the next length x 4, one x 4, ...
        order += [i] * 4 + ([one] * 4 if i != one else [long_] * 4)
    order += [long_, one] * 4 + list(range(len(subs)))
    many = [subs[i] for i in order]
    ov(sim_slots=4)
    st = _hold_command(plans(lib, oc.build_lengths), cl, many, False, ref(False, many))
    assert st["phase_cycles"][1] == 4 and st["phase_cycles"][2] > 1


# ---- D. the general path (finalize_kernel<true>) --------------------------------------------------------------------
D_CASES = {"price-boundary": (oc.build_price_boundary, _pre_price_boundary, (False, True)),
           "same-type": (oc.build_same_type, _pre_same_type, (False, True)),
           "lengths": (oc.build_lengths, _pre_lengths, (False,))}


@pytest.mark.parametrize("which", sorted(D_CASES))
def test_general_path_inputs(lib, which):
    """The clusters of C with a hostname topology spread on every shape: the same edges, held by the oracle."""
    _, pre, _ = D_CASES[which]
    cl, _, _ = pre(lib, True)
    assert all(sh.topology_spread for sh in cl.shapes)


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(D_CASES))
def test_general_path(lib, plans, general_mode, which):
    build, pre, multi = D_CASES[which]
    cl, subs, ref = pre(lib, True)
    for multi_node in multi:
        st = _hold_command(plans(lib, build, True), cl, subs, multi_node, ref(multi_node))
        batched, single = st["phase_cycles"][:2]
        assert [batched, single] == ([len(subs), 0] if general_mode == "batch" else [0, len(subs)])


# ---- E. Drift (finalize_drift_kernel) -------------------------------------------------------------------------------
def _pre_drift(lib):
    key = "drift"
    if key not in _CLUSTERS:
        cl, subs, ts = oc.build_drift(lib)
        _CLUSTERS[key] = (cl, subs, ts, drift_ref.drift(cl, subs))
    cl, subs, ts, want = _CLUSTERS[key]
    its = cl.catalogs[0]
    ncs = want["replacements"]["nodeclaims"]
    assert want["first"] == 0 and sorted(n["n_remaining"] for n in ncs) == [1, oc.N_EQUAL]
    for n in ncs:
        zone = oc.ZA if n["n_remaining"] == 1 else oc.ZB
        rem = ts[128:129] if n["n_remaining"] == 1 else ts
        assert n["options"] == oc.plain_options(its, rem, [zone], oc.OD, 100)
    return cl, subs, want


def test_drift_inputs(lib):
    _pre_drift(lib)


@pytest.mark.gpu
def test_drift(ctx, lib):
    """A replace-all simulation with two NodeClaims of 1 and 257 remaining types, all 257 at one price."""
    import kpamd
    from test_gpu_drift import _check
    cl, subs, want = _pre_drift(lib)
    plan = kpamd.ClusterPlan(ctx, cl)
    try:
        _check(plan.drift(subs, read_all=True), want)
    finally:
        plan.close()


# ---- F. launch selection (launch_kernel) ----------------------------------------------------------------------------
_LAUNCHED = {}


def _launch_oracle(lib, group, max_types):
    from oracle import pyoracle
    its, groups, info = _built(lib, oc.build_launch)
    key = (group, max_types)
    if key not in _LAUNCHED:
        _LAUNCHED[key] = pyoracle.launch_select(its, groups[group], [oc.ZA], max_types=max_types)
    return its, groups[group], info, _LAUNCHED[key]


def _pre_launch(lib, group, max_types):
    its, reqs, info, want = _launch_oracle(lib, group, max_types)
    for (_, _, lst), w in zip(reqs, want):
        assert w["status"] == 0 and w["rejected_exotic"] == 0
        if group != "spot":
            assert w["n_compatible"] == len(lst) and w["rejected_spot"] == 0
            assert w["types"] == oc.plain_options(its, lst, [oc.ZA], oc.OD, max_types)
    if group == "sizes":
        assert [len(r[2]) for r in reqs] == oc.LAUNCH_M
        for _, _, lst in reqs:  # positions 56 to 67 tie, across the cut at 60
            keys = _keys(its, oc.plain_options(its, lst, [oc.ZA], oc.OD, 0))
            assert keys[54] < keys[55] == keys[59] == keys[60] and (len(keys) < 68 or keys[60] == keys[66] < keys[67])
    if group == "exotic":  # minValues: the exotic filter is skipped, and exotic types lead their generic ties
        lst, names = reqs[0][2], _names(its, want[0]["types"])
        assert len(set(_keys(its, lst))) == 1 and any(len(r) > 3 and r[3] for r in reqs[0][0])
        flags = [oc.is_exotic(its[t]) for t in want[0]["types"]]
        assert flags[0] is False and True in flags and flags.index(True) < len(flags) - flags[::-1].index(False) - 1
        assert sum(flags) == len(info["metal"]) == 8 and names == sorted(names, key=str.encode)
    if group == "spot":  # a spot price equal to the cheapest on-demand price stays; one ulp above goes
        lst, M = reqs[0][2], info["M"]
        od = min(_keys(its, lst))
        spot = {t: oc.cheapest(its[t], [oc.ZA], ("spot",)) for t in lst}
        assert od == M and {M, math.nextafter(M, math.inf), math.nextafter(M, 0.0)} <= set(spot.values())
        above = [t for t in lst if spot[t] > M]
        assert want[0]["capacity_type"] == "spot" and want[0]["rejected_spot"] == len(above) == 7
        kept = set(want[0]["types"])
        assert max_types < len(lst) - len(above) or kept == set(lst) - set(above)
        assert not kept & set(above)
    return its, reqs, want


F_PARAMS = [("sizes", 60), ("sizes", 1), ("sizes", 200), ("exotic", 60), ("spot", 60), ("spot", 200)]


@pytest.mark.parametrize("group,max_types", F_PARAMS)
def test_launch_inputs(lib, group, max_types):
    _pre_launch(lib, group, max_types)


@pytest.fixture(scope="module")
def launch_catalog(ctx, lib):
    import kpamd
    ch = kpamd.Catalog(ctx, _built(lib, oc.build_launch)[0])
    yield ch
    ch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("group,max_types", F_PARAMS)
def test_launch(ctx, lib, launch_catalog, group, max_types):
    import kpamd
    from test_gpu_launch import check_same
    its, reqs, want = _pre_launch(lib, group, max_types)
    plan = kpamd.LaunchPlan(ctx, launch_catalog, reqs, [oc.ZA], max_types=max_types)
    try:
        got, _ = plan.run(read=True)
    finally:
        plan.close()
    check_same(got, want)


# ---- G. the price domain --------------------------------------------------------------------------------------------
BAD_PRICES = [-1.0, -oc.SUBNORMAL, -math.inf, math.nan]


def _small(lib):
    return oc.fresh(lib, 65)


def _host_only(lib):
    """A stand-in context without a device: kp_catalog_upload takes a NULL context (host-only catalogues)."""
    return types.SimpleNamespace(lib=lib, h=None)


def _bad_upload(ctx_like, its, price):
    import kpamd
    from kpamd import abi
    t = 7
    its[t].offerings[1].price = price
    with pytest.raises(kpamd.KPError) as e:
        kpamd.Catalog(ctx_like, its)
    assert e.value.code == abi.KP_E_INVAL and its[t].name in str(e.value)


def _bad_update(cat, its, price):
    import kpamd
    from kpamd import abi
    t = 7
    before = [(o.price, o.available) for o in its[t].offerings]
    with pytest.raises(kpamd.KPError) as e:
        cat.update_offerings([(3, "spot", oc.ZA, False), (t, "on-demand", oc.ZA, True, price)], seqnum=9)
    assert e.value.code == abi.KP_E_INVAL and its[t].name in str(e.value)
    assert [(o.price, o.available) for o in its[t].offerings] == before and cat.seqnum() != 9  # all or nothing


@pytest.mark.parametrize("price", BAD_PRICES)
def test_price_domain_upload(lib, price):
    """A negative or NaN price is refused at upload with the type's name; the next upload works."""
    import kpamd
    its = _small(lib)
    _bad_upload(_host_only(lib), its, price)
    kpamd.Catalog(_host_only(lib), _small(lib)).close()


@pytest.mark.parametrize("price", BAD_PRICES)
def test_price_domain_update(lib, price):
    """... and at the offering update, which changes nothing; the catalogue takes the next update."""
    import kpamd
    its = _small(lib)
    cat = kpamd.Catalog(_host_only(lib), its, seqnum=1)
    try:
        _bad_update(cat, its, price)
        cat.update_offerings([(7, "on-demand", oc.ZA, True, 0.5)], seqnum=2)
        assert cat.seqnum() == 2 and oc.cheapest(its[7], [oc.ZA], oc.OD) == 0.5
    finally:
        cat.close()


def test_price_domain_keeps_the_rest(lib):
    """+inf (no finite price), 0.0 and the largest float are prices; a NaN behind the ABI still means "keep"."""
    import ctypes as C
    import kpamd
    from kpamd import abi
    its = _small(lib)
    for o, p in zip(its[7].offerings, [math.inf, 0.0, sys.float_info.max, -0.0]):
        o.price = p
    cat = kpamd.Catalog(_host_only(lib), its, seqnum=1)
    try:
        up = abi.OfferingUpdate(7, 1, b"on-demand", oc.ZA.encode(), math.nan, None, -1, 0)
        assert lib.kp_catalog_update_offerings(cat.h, C.byref(up), 1, 2) == 0 and cat.seqnum() == 2
        cat.update_offerings([(7, "on-demand", oc.ZA, True, -0.0)], seqnum=3)
        assert math.copysign(1.0, next(o.price for o in its[7].offerings if o.capacity_type == "on-demand"
                                       and o.zone == oc.ZA)) == 1.0  # the wrapper's mirror stores +0.0 as the ABI does
    finally:
        cat.close()


@pytest.mark.gpu
def test_price_domain_on_the_device(ctx, lib):
    """Refusals on a live context leave it usable; prices that reach the device as -0.0, at upload and through an
    update, order as +0.0 (the signed-zeros list equals the oracle's, whose < cannot tell the zeros apart)."""
    import kpamd
    for price in BAD_PRICES:
        _bad_upload(ctx, _small(lib), price)
    cats, claims, prob, want = _pre_b(lib, "signed-zeros", 100)
    oc.assert_plain(cats, claims, 100, _hold_solve(ctx, prob, want))
    # ... and through the update path: uploaded at 1.0, then every type set to its zero
    its = _built(lib, oc.build_all_equal)[0][0]
    ts = claims[0]["types"]
    assert _names(its, ts) == _names(cats[0], ts)
    import copy
    live = copy.deepcopy(its)
    cat = kpamd.Catalog(ctx, live, seqnum=1)
    try:
        for price in BAD_PRICES:
            _bad_update(cat, live, price)
        cat.update_offerings([(t, "on-demand", oc.ZA, True, (-0.0 if j % 2 else 0.0)) for j, t in enumerate(ts)], seqnum=2)
        updated = oc.solve_problem([live], claims, 100, "signed-zeros-updated")
        got = kpamd.Scheduler(ctx, updated, catalogs=[cat]).solve()
        assert oc.by_claim(got)[0]["options"] == oc.by_claim(want)[0]["options"]
    finally:
        cat.close()
