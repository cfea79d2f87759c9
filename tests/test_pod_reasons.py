"""Why a pod is unschedulable: kp_solve_run_explained's per-NodePool reasons against a plain reference.

Upstream `Scheduler.add` returns, for a pod it cannot place, one error per NodeClaimTemplate; the device returns their
causes (enum kp_why) with the counts behind `filterInstanceTypesByRequirements`' message. The reference is
`pod_reason_cases.plain_reasons` (oracle primitives + numpy; see its docstring for what it models). Upstream core is
not in the tree: parity beyond the semantics written in include/kp/kp_abi.h and DESIGN.md is unpinned.

CPU tests hold every builder's reference to a hand-written expectation and prove from the oracle that the input is
the case it claims (the pod is unschedulable, and schedules once the named cause is removed). The gpu tests hold the
device to the reference (`==` on every field), and the explained run to the plain run of the same plan.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import pod_reason_cases as prc

gpu = pytest.mark.gpu
FIELDS = ("nodepool", "code", "taint", "keys", "n_types") + prc.COUNTS


def _check_expectation(rows, expect):
    assert len(rows) == len(expect)
    for row, e in zip(rows, expect):
        for k, v in e.items():
            if k == "zero":
                assert [row[f] for f in v] == [0] * len(v), (row, e)
            elif k == "full":
                assert row["n_types"] > 0 and [row[f] for f in v] == [row["n_types"]] * len(v), (row, e)
            elif k == "positive":
                assert all(row[f] > 0 for f in v), (row, e)
            elif k == "all_but_one":
                assert [row[f] for f in v] == [row["n_types"] - 1] * len(v), (row, e)
            else:
                assert row[k] == v, (k, row, e)


# ---- CPU: the reference and the builders -----------------------------------------------------------------------
def test_pool_reason_struct_size(tmp_path):
    """The ctypes mirror of kp_pool_reason has the size gcc gives the header's struct."""
    import os
    import shutil
    import subprocess
    from kpamd import abi
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "kp/kp_abi.h"\nint main(void){printf("%zu %d\\n", '
                   'sizeof(kp_pool_reason), (int)KP_WHY_MIN_VALUES);return 0;}\n')
    subprocess.check_call(["gcc", "-I", inc, str(src), "-o", str(tmp_path / "sz")])
    size, last = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()]
    assert size == C.sizeof(abi.PoolReason) == 12 * 4 + 8
    assert last == abi.KP_WHY_MIN_VALUES == 6


def test_concatenated_requirements_intersect_a_repeated_key(lib):
    """The reference merges by concatenating the template's and the pod's lists: the oracle's FromABI Adds entry by
    entry, so two entries on one key act as their intersection."""
    from oracle import pyoracle
    two = [(prc.ZONE, "In", ["a", "b"]), (prc.ZONE, "In", ["b", "c"])]
    assert pyoracle.requirements_intersects([(prc.ZONE, "In", ["b"])], two)
    assert not pyoracle.requirements_intersects([(prc.ZONE, "In", ["a"])], two)
    assert not pyoracle.requirements_intersects([(prc.ZONE, "In", ["c"])], two)
    assert pyoracle.requirements_compatible(two, [(prc.ZONE, "In", ["b"])], True)
    assert not pyoracle.requirements_compatible(two, [(prc.ZONE, "In", ["a"])], True)


@pytest.mark.parametrize("name", prc.CASE_NAMES)
def test_builder_is_the_case_it_claims(lib, name):
    from oracle import pyoracle
    c, want, ref = prc.case(lib, name)
    assert len(c.problem.nodepools) == 3 and c.problem.n_pods <= 36
    assert [int(p) for p in np.flatnonzero(want["placement"] == -1)] == c.fail
    assert all(want["placement"][p] != -1 for p in c.ok)
    assert sorted(ref) == c.fail
    for p in c.fail:
        _check_expectation(ref[p], c.expect)
        assert all(r["code"] != prc.NONE for r in ref[p])
        assert [r["nodepool"] for r in ref[p]] == prc.template_order(c.problem)
    fixed = pyoracle.solve(c.fixed)
    assert all(fixed["placement"][p] != -1 for p in c.fail), "the pod does not schedule once the cause is removed"


def test_topology_kat_on_the_oracle(lib):
    """The KAT's pod is unschedulable pinned or not (nothing fits its request). With a request that fits, the pinned
    pod still fails (topology alone) and the unpinned one schedules: topology is the pinned pod's cause. Without
    minDomains the pinned pod schedules: the minimum is taken over the pod's own domains (pod_reason_cases.topology_kat)."""
    from oracle import pyoracle
    its = copy.deepcopy(prc.fc.sized_catalog(lib, prc.BASE_TYPES))
    for pinned, placed in ((True, False), (False, True)):
        assert pyoracle.solve(prc.topology_kat(its, pinned=pinned))["placement"][0] == -1
        small = pyoracle.solve(prc.topology_kat(its, pinned=pinned, requests=prc.SMALL))
        assert (small["placement"][0] != -1) == placed
        assert small["placement"][1] != -1
    assert pyoracle.solve(prc.topology_kat(its, pinned=True, min_domains=None, requests=prc.SMALL))["placement"][0] != -1


def test_random_seeds_cover_the_codes(lib):
    """Chosen on the CPU: every seed leaves a pod unscheduled; over the seeds the reference reports at least three
    distinct codes, and both a zero and a non-zero n_requirements under INSTANCE_TYPES; KP_WHY_NONE never occurs."""
    codes, nreq = set(), set()
    for seed in prc.RANDOM_SEEDS:
        prob, want, ref = prc.random_case(lib, seed)
        assert ref, seed
        assert all(not p.limits for p in prob.nodepools) and not prob.existing
        assert all(not s.topology_spread for s in prob.shapes)
        for rows in ref.values():
            codes |= {r["code"] for r in rows}
            nreq |= {r["n_requirements"] > 0 for r in rows if r["code"] == prc.INSTANCE_TYPES}
    assert prc.NONE not in codes and len(codes) >= 3, codes
    assert nreq == {False, True}


# ---- device ------------------------------------------------------------------------------------------------------
def _strip(reasons):
    return {p: [{f: r[f] for f in FIELDS} for r in rows] for p, rows in reasons.items()}


def _explained_and_plain(ctx, prob):
    """One plan: a plain run, an explained run."""
    import kpamd
    plan = kpamd.Scheduler(ctx, prob).prepare()
    try:
        return plan.run(), plan.run(explain=True)
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("name", prc.CASE_NAMES)
def test_device_reasons_equal_the_reference(ctx, lib, name):
    c, want, ref = prc.case(lib, name)
    plain, got = _explained_and_plain(ctx, c.problem)
    assert prc.same_solve(got, plain) and prc.same_solve(got, want)
    assert _strip(got["reasons"]) == _strip(ref)


@gpu
@pytest.mark.parametrize("seed", prc.RANDOM_SEEDS)
def test_device_reasons_equal_the_reference_randomized(ctx, lib, seed):
    prob, want, ref = prc.random_case(lib, seed)
    plain, got = _explained_and_plain(ctx, prob)
    assert prc.same_solve(got, plain) and prc.same_solve(got, want)
    assert _strip(got["reasons"]) == _strip(ref)


@gpu
def test_topology_kat(ctx, lib):
    """Code 4 on every template for the pinned pod; not pinned, topology passes and the request is what fails."""
    from oracle import pyoracle
    its = copy.deepcopy(prc.fc.sized_catalog(lib, prc.BASE_TYPES))
    for pinned in (True, False):
        prob = prc.topology_kat(its, pinned=pinned)
        plain, got = _explained_and_plain(ctx, prob)
        assert prc.same_solve(got, plain) and prc.same_solve(got, pyoracle.solve(prob))
        assert sorted(got["reasons"]) == [0]
        rows = got["reasons"][0]
        assert [r["nodepool"] for r in rows] == prc.template_order(prob)
        if pinned:
            assert [r["code"] for r in rows] == [prc.TOPOLOGY] * 3
            assert all(r["n_types"] > 0 and all(r[f] == 0 for f in prc.COUNTS) for r in rows)
        else:
            assert [r["code"] for r in rows] == [prc.INSTANCE_TYPES] * 3
            assert all(r["n_fits"] == 0 and r["n_requirements"] > 0 for r in rows)


@gpu
def test_explained_plan_reruns_to_identical_results(ctx, lib):
    """The explanation step writes nothing the Solve reads: plain and explained runs alternate, three times."""
    import kpamd
    c, want, ref = prc.case(lib, "limits-exhausted")
    plan = kpamd.Scheduler(ctx, c.problem).prepare()
    try:
        for _ in range(3):
            plain = plan.run()
            got = plan.run(explain=True)
            assert prc.same_solve(plain, want) and prc.same_solve(got, want)
            assert "reasons" not in plain and _strip(got["reasons"]) == _strip(ref)
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("seed", prc.RANDOM_SEEDS[:2])
def test_fast_lane_variants_give_identical_reasons(ctx, ov, lib, seed):
    import kpamd
    prob, want, ref = prc.random_case(lib, seed)
    got = []
    for fl in (0, 1):
        ov(fast_lane=fl)
        got.append(kpamd.Scheduler(ctx, prob).solve(explain=True))
    assert prc.same_solve(got[0], got[1])
    assert _strip(got[0]["reasons"]) == _strip(got[1]["reasons"]) == _strip(ref)


@gpu
def test_reservation_catalogue_is_unsupported(ctx, lib):
    import kpamd
    from test_reserved_solve import FALLBACK, _big_pods_problem
    _, prob = _big_pods_problem(lib, FALLBACK)
    sched = kpamd.Scheduler(ctx, prob)
    sched.solve()  # the plain Solve takes it
    with pytest.raises(kpamd.KPError) as e:
        sched.solve(explain=True)
    assert e.value.code == kpamd.abi.KP_E_UNSUPPORTED


@gpu
def test_reading_reasons_from_a_plain_result_is_invalid(ctx, lib):
    import kpamd
    from kpamd import abi
    c, _, _ = prc.case(lib, "only-fits")
    plan = kpamd.Scheduler(ctx, c.problem).prepare()
    res = C.c_void_p()
    try:
        assert lib.kp_solve_run(plan.h, C.byref(res)) == 0
        buf = (abi.PoolReason * 3)()
        assert lib.kp_result_explained(res) == 0
        assert lib.kp_result_reason_count(res, 0) == 0
        assert lib.kp_result_pod_reasons(res, 0, buf, 3) == abi.KP_E_INVAL
        lib.kp_result_destroy(res)
        res = C.c_void_p()
        assert lib.kp_solve_run_explained(plan.h, None, C.byref(res)) == 0
        assert lib.kp_result_explained(res) == 1
        assert lib.kp_result_reason_count(res, 0) == 3 and lib.kp_result_reason_count(res, 2) == 0
        assert lib.kp_result_pod_reasons(res, c.problem.n_pods, buf, 3) == abi.KP_E_INVAL  # pod out of range
        assert lib.kp_result_pod_reasons(res, 2, buf, 3) == 0  # a scheduled pod: no entries
    finally:
        if res:
            lib.kp_result_destroy(res)
        plan.close()


@gpu
def test_cancelled_explained_run_leaves_the_plan_usable(ctx, lib):
    import kpamd
    c, want, ref = prc.case(lib, "taint")
    plan = kpamd.Scheduler(ctx, c.problem).prepare()
    cancel = kpamd.Cancel(ctx)
    try:
        cancel.set()
        with pytest.raises(kpamd.KPError) as e:
            plan.run(explain=True, cancel=cancel)
        assert e.value.code == kpamd.abi.KP_E_CANCELED
        cancel.reset()
        got = plan.run(explain=True, cancel=cancel)
        assert prc.same_solve(got, want) and _strip(got["reasons"]) == _strip(ref)
    finally:
        cancel.close()
        plan.close()
