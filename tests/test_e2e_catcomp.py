"""Consumers see no difference: two NodePools on two EC2NodeClasses that differ in maxPods and in their
kubelet reservations. One Solve on the catalogues catalog.build_catalogs assembles from kp_catalog_compile gives the
placements and NodeClaims of the Solve on the catalogues build_catalog makes one pair at a time, on the oracle and on
the device."""
import numpy as np
import pytest

import kpamd
from kpamd import catalog
from kpamd.model import NodePool, PodShape, Problem

pytestmark = pytest.mark.gpu

K = "karpenter.k8s.aws/"
NODECLASSES = [dict(max_pods=12),
               dict(max_pods=110, kubelet_cfg=dict(kube_reserved={"cpu": "500m", "memory": "2Gi"},
                                                   system_reserved={"cpu": "250m", "memory": "512Mi"}))]


def problem(cats):
    pools = [NodePool("few-pods", 10, 0, [("karpenter.sh/capacity-type", "In", ["on-demand", "spot"]),
                                          (K + "instance-category", "In", ["c", "m", "r"]),
                                          (K + "instance-generation", "Gt", ["4"])]),
             NodePool("reserved-heavy", 5, 1, [("karpenter.sh/capacity-type", "In", ["on-demand"]),
                                               (K + "instance-generation", "Gt", ["3"])])]
    shapes = [PodShape({"cpu": 250, "memory": 256 * 1048576 * 1000, "pods": 1000}),
              PodShape({"cpu": 1500, "memory": 3 * 1024 * 1048576 * 1000, "pods": 1000}),
              PodShape({"cpu": 100, "memory": 64 * 1048576 * 1000, "pods": 1000}, node_selector={"karpenter.sh/nodepool": "reserved-heavy"}),
              PodShape({"cpu": 3000, "memory": 1024 * 1048576 * 1000, "pods": 1000}, node_selector={"karpenter.sh/nodepool": "reserved-heavy"}),
              PodShape({"cpu": 500, "memory": 512 * 1048576 * 1000, "pods": 1000},
                       node_selector={"topology.kubernetes.io/zone": catalog.ZONES[1]})]
    rng = np.random.default_rng(18)
    n = 400
    shape = rng.integers(0, len(shapes), size=n).astype(np.uint32)
    creation = (1_750_000_000 + rng.integers(0, 600, size=n)).astype(np.int64)
    uid = rng.integers(0, np.iinfo(np.int64).max, size=n, dtype=np.int64).astype(np.uint64)
    return Problem(cats, pools, shapes, shape, creation, uid, name="catcomp-e2e")


def claims(res):
    return [(n["nodepool"], n["pods"], n["options"], n["requests"]) for n in res["nodeclaims"]]


@pytest.fixture(scope="module")
def catalogues(ctx, lib):
    rows = catalog.load_ec2_table()
    one_by_one = [catalog.build_catalog(lib, rows=rows, **kw) for kw in NODECLASSES]
    compiled = catalog.build_catalogs(ctx, NODECLASSES, rows=rows)
    return one_by_one, compiled


@pytest.mark.parametrize("backend", ["oracle", "device"])
def test_one_solve_on_either_catalogues(ctx, catalogues, backend):
    from oracle import pyoracle
    solve = pyoracle.solve if backend == "oracle" else (lambda prob: kpamd.Scheduler(ctx, prob).solve())
    one_by_one, compiled = catalogues
    want, got = solve(problem(one_by_one)), solve(problem(compiled))
    assert (got["placement"] == want["placement"]).all()
    assert claims(got) == claims(want)
    # the scenario reaches both NodeClasses, and their difference shows
    by_pool = {p: [c for c in claims(got) if c[0] == p] for p in (0, 1)}
    assert by_pool[0] and by_pool[1] and (got["placement"] >= 0).all()
    assert max(len(c[1]) for c in by_pool[0]) <= 12 < max(len(c[1]) for c in by_pool[1])
    cpu = {t.name: t.overhead["cpu"] for t in compiled[0]}
    assert all(t.overhead["cpu"] == 750 != cpu[t.name] for t in compiled[1])
