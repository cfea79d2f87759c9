"""The reference's disruption-budget scenarios (R:test/suites/consolidation/suite_test.go:184-486) over the cluster model
of tests/e2e.py — TEST INFRASTRUCTURE.

What the budget suite adds to the environment, and how it is modelled here:
  testing finalizer   the suite puts a finalizer on every node, so a disrupted node stays (deleting) until the test lets
                      it go. Here a command is applied at once (tests/e2e.py), and its candidates are then "held": gone
                      from the snapshot, but still counted in their NodePool's total and deleting numbers through
                      allowed_disruptions' extra_deleting, until release().
  ConsistentlyExpectDisruptionsUntilNoneLeft
                      consolidate_budgeted(): start commands until the controller returns none (a wave), release the
                      held nodes, and repeat until a wave starts nothing. peak_held / peak_nodes record what the suite
                      watches (nodes disrupting at once, nodes present at once).
  NodeClaim labels    a node carries the single-valued In requirements of the NodeClaim it was launched from (the
                      "test-partition" label of the replace scenario).
  ForcePodsToSpread   keep_one_per_node(): every node keeps its oldest pod of the Deployment.
"""
import collections

import e2e


class BudgetEnv(e2e.Env):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.held = collections.Counter()  # NodePool index -> nodes disrupted and not yet released
        self.node_reqs = {}
        self.peak_held = 0
        self.peak_nodes = 0
        self.waves = []  # per wave: the commands started

    def _create(self, reqs, requests, options, pool):
        name = super()._create(reqs, requests, options, pool)
        if name is not None:
            self.node_reqs[name] = list(reqs)
        return name

    def labels(self, name):
        lab = super().labels(name)
        for k, op, vals, *_ in self.node_reqs.get(name, ()):
            if op == "In" and len(vals) == 1 and k not in lab:
                lab[k] = vals[0]
        return lab

    def keep_one_per_node(self, deployment):
        _, pods = self.deployments[deployment]
        for n in self.nodes:
            mine = sorted((p for p in pods if self.alive[p] and self.pod_node[p] == n), key=lambda p: self.pod_created[p])
            for p in mine[1:]:
                self.alive[p] = False
                self.pod_node[p] = None

    def release(self):
        self.held.clear()

    def consolidate_budgeted(self, now=0, max_waves=16, max_commands=64):
        """Waves of commands under the NodePools' budgets. Returns the waves started by this call."""
        from kpamd import disruption
        started = []
        for _ in range(max_waves):
            wave = []
            while len(wave) < max_commands:
                cl, names = self.cluster()
                plan = self._plan(cl)
                try:
                    cmd = disruption.Controller().compute_command(cl, plan, now=now, extra_deleting=dict(self.held))
                finally:
                    plan.close()
                if cmd is None:
                    break
                pools = [self.nodes[names[c]]["pool"] for c in cmd.candidates]
                self._apply(cl, names, cmd)
                self.held.update(pools)
                self.commands.append(cmd)
                wave.append(cmd)
                self.peak_held = max(self.peak_held, sum(self.held.values()))
                self.peak_nodes = max(self.peak_nodes, len(self.nodes) + sum(self.held.values()))
            else:
                raise AssertionError(f"a wave did not settle after {max_commands} commands")
            self.release()
            if not wave:
                return started
            self.waves.append(wave)
            started.append(wave)
        raise AssertionError(f"consolidation did not settle after {max_waves} waves")
