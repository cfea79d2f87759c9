"""Why the fast lane's open-set loop stops, from an OS_DIAG build: tools/build_variant.sh osdiag -DOS_DIAG=1,
then KP_LIB=tools/variants/osdiag/libkp.so python tools/open_set_stops.py [config] [pods]. One Solve; the calls of
fl_open_set by stop reason (stats[25..30], exported as fast_cycles in that build) and the pods it placed. JSON to stdout."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "karpenter-provider-aws_amd"))
import kpamd  # noqa: E402
from kpamd import catalog, synth  # noqa: E402

REASONS = ["another_class", "untagged_level", "nodeclaim_outside_set", "fits_empties_types", "literal_pdqsort",
           "window_end_or_pop_stop"]
cfg = sys.argv[1] if len(sys.argv) > 1 else "2"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 50000
cat = catalog.build_catalog(kpamd.load_lib())
prob = {"2": lambda: synth.config2(cat, n_pods=n, seed=2),
        "2b": lambda: synth.config2(cat, n_pods=n, seed=2, burst=True)}[cfg]()
ctx = kpamd.Context(0)
ctx.set_overrides(fast_lane=4)
st = kpamd.Scheduler(ctx, prob).solve()["stats"]
out = {"config": cfg, "pods": n, "fast_pods": int(st["fast_pods"]), "run_length_pods": int(st["run_length_pods"]),
       "calls_by_stop": {r: int(v) for r, v in zip(REASONS, st["fast_cycles"])}}
out["calls"] = sum(out["calls_by_stop"].values())
print(json.dumps(out))
ctx.close()
