"""Open-set probe (the fast lane's open set): replays the oracle's placement of config 2 in Queue order, on the
CPU, and counts what share of the pods land on the NodeClaim the previous pod joined, on one of the last 2 / 4 / 8
distinct NodeClaims committed to, on a NodeClaim that already holds their requirement class (the append path), and carry
the request row of the pod before them. It then emulates the reach of an open set of K NodeClaims (least recently
committed evicted): a pod is taken when the pod before it was committed on the append path, it has that pod's request
row, sits in the same 64-entry window, and lands on an open NodeClaim that already holds its requirement class. An
upper bound on the device's run_length_pods: the cursor, unknown-memo and sort cuts are not emulated, and the device
drops the set at a window's end. usage: open_set_probe.py [pods] [seed]; JSON to stdout."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "karpenter-provider-aws_amd"))
sys.path.insert(0, REPO)
import kpamd  # noqa: E402
from kpamd import catalog, synth  # noqa: E402
from runlength_probe import queue_order  # noqa: E402


def main():
    from oracle import pyoracle
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    cat = catalog.build_catalog(kpamd.load_lib())
    prob = synth.config2(cat, n_pods=n, seed=seed)
    res = pyoracle.solve(prob)
    q = queue_order(prob)
    shp, pl = prob.pod_shape[q], res["placement"][q]
    row = [tuple(sorted((k, v) for k, v in s.requests.items() if v)) for s in prob.shapes]
    rqc_ids = {}
    rqc = [rqc_ids.setdefault(repr((sorted(s.node_selector.items()), s.required_terms, s.preferred_terms,
                                    s.tolerations)), len(rqc_ids)) for s in prob.shapes]
    held = set()   # (NodeClaim, requirement class) placed so far
    recent = []    # distinct NodeClaims, least recently committed first
    c = dict(same_nodeclaim=0, last2=0, last4=0, last8=0, append_path=0, same_row=0)
    reach = {k: 0 for k in (1, 2, 4, 8)}
    sets = {k: [] for k in reach}
    prev_ok = False
    for i in range(len(q)):
        nc, s = int(pl[i]), int(shp[i])
        app = nc >= 0 and (nc, rqc[s]) in held
        srow = i > 0 and row[s] == row[int(shp[i - 1])]
        if nc >= 0:
            c["same_nodeclaim"] += bool(recent) and recent[-1] == nc
            for k in (2, 4, 8):
                c[f"last{k}"] += nc in recent[-k:]
            c["append_path"] += app
        c["same_row"] += srow
        for k, open_set in sets.items():
            if prev_ok and app and srow and i % 64 and nc in open_set:
                reach[k] += 1
            if app:
                if nc in open_set:
                    open_set.remove(nc)
                open_set.append(nc)
                del open_set[:-k]
            else:
                open_set.clear()
        prev_ok = app
        if nc >= 0:
            held.add((nc, rqc[s]))
            if nc in recent:
                recent.remove(nc)
            recent.append(nc)
    out = {"pods": n, "seed": seed, "nodeclaims": len(res["nodeclaims"]), "requirement_classes": len(rqc_ids),
           "request_rows": len(set(row))}
    out.update({"share_" + k: round(v / n, 4) for k, v in c.items()})
    out.update({f"reach_K{k}": round(v / n, 4) for k, v in reach.items()})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
