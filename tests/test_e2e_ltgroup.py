"""End to end: one Solve on the device, its NodeClaims launched through kp_launch_templates with an amd64
and an arm64 AMI. Every NodeClaim gets the CreateFleet launch-template configs the plain-Python reference
(tests/ltgroup_ref.py) gives, and every override names a type the launch selected."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ltgroup_ref as ref  # noqa: E402
from ltgroup_cases import AMD, ARM  # noqa: E402

pytestmark = pytest.mark.gpu


def test_solve_then_launch_templates(ctx, catalog):
    import kpamd
    from kpamd import catalog as cmod, synth
    prob = synth.config2(catalog, n_pods=400, seed=7)
    res = kpamd.Scheduler(ctx, prob).solve()
    requests = kpamd.launch_requests_from_solve(res)
    assert len(requests) == len(res["nodeclaims"]) > 3
    ch = kpamd.Catalog(ctx, catalog)
    try:
        got = ctx.launch_templates(ch, requests, cmod.ZONES, [AMD, ARM])
    finally:
        ch.close()
    want = ref.launch_templates(catalog, requests, cmod.ZONES, [AMD, ARM])
    assert len(got) == len(requests)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"NodeClaim {i}: device {g} vs reference {w}"
        assert g["lt_status"] == "OK" and g["configs"] and g["unmapped"] == 0
        for c in g["configs"]:
            assert c["ami"] in ("ami-123", "ami-456") and c["overrides"]
            assert {t for t, _ in c["overrides"]} <= set(c["types"]) <= set(g["types"])
        assert sum(len(c["overrides"]) for c in g["configs"]) == g["n_overrides"]
