"""Mixed-run probe (the run-length commit across shapes of one request row): for config 2 with uniform
creation times and with per-deployment bursts, the share of pods in Queue order that land on the NodeClaim the previous
pod joined, that also carry its request row, and whose shape was placed on that NodeClaim before ("flagged": the
level is merged, so the commit could take the pod), split by whether the neighbour has the same shape (the single-level
commit's reach) or another one. An upper bound on the device's batched share: the cursor, sort-tie, Fits-threshold and
window cuts are not emulated. Oracle placement (CPU: --oracle) or the device's. JSON to stdout."""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "karpenter-provider-aws_amd"))
sys.path.insert(0, REPO)
import kpamd  # noqa: E402
from kpamd import catalog, synth  # noqa: E402
from runlength_probe import queue_order  # noqa: E402


def main():
    use_oracle = "--oracle" in sys.argv
    n = int(os.environ.get("RL_PODS", "50000"))
    lib = kpamd.load_lib()
    cat = catalog.build_catalog(lib)
    ctx = None if use_oracle else kpamd.Context(0)
    for burst in (False, True):
        prob = synth.config2(cat, n_pods=n, seed=2, burst=burst)
        if use_oracle:
            from oracle import pyoracle
            res = pyoracle.solve(prob)
        else:
            res = kpamd.Scheduler(ctx, prob).solve()
        q = queue_order(prob)
        shp = prob.pod_shape[q]
        pl = res["placement"][q]
        row = [tuple(sorted(s.requests.items())) for s in prob.shapes]
        seen = set()  # (NodeClaim, shape) pairs placed so far
        c = dict(same_nodeclaim=0, same_row=0, flagged=0, flagged_same_shape=0, flagged_other_shape=0)
        for i in range(len(q)):
            if i and pl[i] >= 0 and pl[i] == pl[i - 1]:
                c["same_nodeclaim"] += 1
                if row[shp[i]] == row[shp[i - 1]]:
                    c["same_row"] += 1
                    if (int(pl[i]), int(shp[i])) in seen:
                        c["flagged"] += 1
                        c["flagged_same_shape" if shp[i] == shp[i - 1] else "flagged_other_shape"] += 1
            if pl[i] >= 0:
                seen.add((int(pl[i]), int(shp[i])))
        out = {"burst": burst, "pods": n, "run_length_pods": res["stats"].get("run_length_pods")}
        out.update({k: v for k, v in c.items()})
        out.update({"share_" + k: round(v / n, 4) for k, v in c.items()})
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
