"""The e2e consolidation loop with upstream's last step in it - TEST INFRASTRUCTURE.

ValidatingEnv is test_e2e_commands.CommandEnv (commands applied straight from what the plan returns) whose consolidate()
validates every command against a FRESH snapshot before applying it, as SingleNodeConsolidation and
MultiNodeConsolidation do through Validation.IsValid: compute on snapshot A, let the world change (churn), snapshot B,
kpamd.disruption.Controller.validate(cmd, A, B, plan of B); a rejected command is not applied and the next pass
recomputes. What the model adds to e2e.Env for the churn:

  ICE               env.ice holds (type name, capacity type, zone) marks: those offerings are unavailable in every
                    catalogue built from then on (a new catalogue: the snapshot is one of current state)
  deletion          env.deleting holds node names marked for deletion: ClusterNode.deleting in the snapshot (never a
                    candidate, its pods join every simulation); finish_deletion() ends it (pods pending, node gone)
  after a rejection the provisioner runs (pods a churn left pending are scheduled) before the next disruption pass"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import e2e  # noqa: E402
import validate_ref  # noqa: E402
from test_e2e_commands import CommandEnv  # noqa: E402


class ValidatingEnv(CommandEnv):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.ice = set()
        self.deleting = set()
        self.validations = []  # per command computed: (method, candidate names, decision, ok, reason)
        self.rejected = []

    # ---- the catalogue, with the ICE marks ---------------------------------------------------------------------------
    def types(self):
        import collections
        used = collections.Counter(n["rid"] for n in self.nodes.values() if n["rid"])
        crs = [self.cmod.CapacityReservation(c.id, c.instance_type, c.availability_zone, c.reservation_type,
                                             max(0, c.available_count - used[c.id])) for c in self.crs.values()]
        key = (tuple((c.id, c.available_count) for c in crs), tuple(sorted(self.ice)))
        if self._types is None or key != self._key:
            types = self.cmod.build_catalog(self.lib, capacity_reservations=crs)
            for it in types:
                for o in it.offerings:
                    if (it.name, o.capacity_type, o.zone) in self.ice:
                        o.available = False
            self._types, self._key = types, key
            if self.backend == "device":
                import kpamd
                if self._cat is not None:
                    self._cat.close()
                self._seq += 1
                self._cat = kpamd.Catalog(self.ctx, self._types, seqnum=self._seq)
        return self._types

    # ---- the snapshot, with the deletion marks -----------------------------------------------------------------------
    def cluster(self):
        cl, names = super().cluster()
        for node, name in zip(cl.nodes, names):
            node.deleting = name in self.deleting
        return cl, names

    def finish_deletion(self, name):
        for p in self.pods_on(name):
            self.pod_node[p] = None
        del self.nodes[name]
        self.deleting.discard(name)

    def _plan(self, cl):
        if self.backend == "device":
            return e2e.Env._plan(self, cl)
        return validate_ref.OracleValidatePlan(cl)

    # ---- the disruption loop -----------------------------------------------------------------------------------------
    def consolidate(self, max_commands=64, churn=None):
        """The disruption controller until it finds nothing to do, every command validated before it is applied.
        churn(env, cluster, names, cmd): called between compute and validate for each command until it acts; it
        returns None (did nothing) or a callable run after the command's rejection. Returns the commands applied."""
        from kpamd import disruption
        done = []
        self.consolidating = True
        try:
            for _ in range(max_commands):
                cl, names = self.cluster()
                plan = self._plan(cl)
                try:
                    cmd = disruption.Controller(materialize=True).compute_command(cl, plan)
                finally:
                    plan.close()
                if cmd is None:
                    return done
                after = None
                if churn is not None:
                    after = churn(self, cl, names, cmd)
                    if after is not None:
                        churn = None
                cl2, _ = self.cluster()
                plan2 = self._plan(cl2)
                try:
                    ok, why = disruption.Controller().validate(cmd, cl, cl2, plan2)
                finally:
                    plan2.close()
                self.validations.append((cmd.method, [names[c] for c in cmd.candidates], cmd.decision, ok, why))
                if not ok:
                    self.rejected.append(cmd)
                    if after is not None:
                        after()
                    self.consolidating = False
                    self.provision()
                    self.consolidating = True
                    continue
                assert not self.deleting, "a command applied next to nodes still terminating"
                self._apply(cl, names, cmd)
                done.append(cmd)
                self.commands.append(cmd)
        finally:
            self.consolidating = False
        raise AssertionError(f"consolidation did not settle after {max_commands} commands: {self.validations[-4:]}")
