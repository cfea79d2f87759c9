"""Redundant-merge probe (requirement classes), CPU only: the oracle's placement of config 2, with uniform
creation times and with per-deployment bursts, replayed in Queue order. A first meeting is the first pod of a shape on a
NodeClaim: NodeClaim.Add runs in full there (a creation, or a merge). Counted: the first meetings, the creations among
them, and the first meetings whose requirement row (nodeSelector, required terms) the NodeClaim already carries from
an earlier pod of another shape, where the merge recomputes what the NodeClaim holds (Requirement.Intersection is
idempotent); also the distinct requirement rows, and the pods that could join a run-length batch (same NodeClaim and
request row as their predecessor, shape already there) with the runs they form. JSON to stdout, one line per variant."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "karpenter-provider-aws_amd"))
sys.path.insert(0, REPO)
import kpamd  # noqa: E402
from kpamd import catalog, synth  # noqa: E402
from runlength_probe import queue_order  # noqa: E402


def req_row(shape):
    """The shape's level-0 requirement set as a hashable row."""
    terms = tuple(tuple((k, op, tuple(v)) for k, op, v, *_ in t) for t in shape.required_terms)
    return (tuple(sorted(shape.node_selector.items())), terms)


def probe(prob, res):
    q = queue_order(prob)
    shp, pl = prob.pod_shape[q], res["placement"][q]
    rows = [req_row(s) for s in prob.shapes]
    reqs = [tuple(sorted(s.requests.items())) for s in prob.shapes]
    seen, on_nc = set(), {}  # (NodeClaim, shape) pairs so far; requirement rows per NodeClaim
    c = dict(first_meetings=0, creations=0, row_already_there=0, batchable_pods=0, batch_runs=0)
    in_run = False
    for i in range(len(q)):
        nc, s = int(pl[i]), int(shp[i])
        if nc < 0:
            in_run = False
            continue
        had = (nc, s) in seen
        if not had:
            c["first_meetings"] += 1
            if nc not in on_nc:
                c["creations"] += 1
            elif rows[s] in on_nc[nc]:
                c["row_already_there"] += 1
        joins = bool(i) and had and nc == int(pl[i - 1]) and reqs[s] == reqs[int(shp[i - 1])]
        if joins:
            c["batchable_pods"] += 1
            c["batch_runs"] += not in_run
        in_run = joins
        seen.add((nc, s))
        on_nc.setdefault(nc, set()).add(rows[s])
    c["requirement_rows"] = len(set(rows))
    c["shapes_without_requirements"] = sum(r == ((), ()) for r in rows)
    return c


def main():
    from oracle import pyoracle
    n = int(os.environ.get("RL_PODS", "50000"))
    cat = catalog.build_catalog(kpamd.load_lib())
    for burst in (False, True):
        prob = synth.config2(cat, n_pods=n, seed=2, burst=burst)
        out = {"burst": burst, "pods": n}
        out.update(probe(prob, pyoracle.solve(prob)))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
