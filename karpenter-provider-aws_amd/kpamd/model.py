"""Python mirror of the reference objects on the hot path (names follow the reference).

  InstanceType / Offering   <- sigs.k8s.io/karpenter pkg/cloudprovider types, built by
                               R:pkg/providers/instancetype/types.go:123-155 and offering.go:101-150
  NodePool                  <- karpv1.NodePool (the fields NewNodeClaimTemplate reads)
  PodShape / pods           <- corev1.Pod fields the scheduler reads (requests, nodeSelector, node
                               affinity, tolerations); pods are (shape, creationTimestamp, uid)
  ExistingNode              <- state.StateNode as seen by upstream scheduling.ExistingNode

Requirements are lists of tuples (key, operator, values[, minValues]) exactly like
scheduling.NewRequirementWithFlexibility's arguments. Quantities are int milli-units.
"""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

Req = Tuple  # (key, op, [values], minValues|None)


@dataclass
class Offering:
    capacity_type: str
    zone: str
    zone_id: Optional[str]
    price: float
    available: bool
    reservation_id: Optional[str] = None
    reservation_type: Optional[str] = None
    reservation_capacity: int = 0


@dataclass
class InstanceType:
    name: str
    requirements: List[Req]
    capacity: Dict[str, int]
    overhead: Dict[str, int]
    offerings: List[Offering] = field(default_factory=list)

    def allocatable(self):
        out = dict(self.capacity)
        for k, v in self.overhead.items():
            if k in out:
                out[k] -= v
        return out


@dataclass
class Budget:
    """One entry of NodePool spec.disruption.budgets (R:pkg/apis/crds/karpenter.sh_nodepools.yaml:95-135): nodes is
    "p%" or an integer string, reasons a list out of Underutilized / Empty / Drifted (None: every reason), schedule a
    five-field cron expression or @macro (UTC) that opens a window of duration_s seconds (both or neither)."""
    nodes: str
    reasons: Optional[List[str]] = None
    schedule: Optional[str] = None
    duration_s: Optional[int] = None


@dataclass
class NodePool:
    name: str
    weight: int = 0
    catalog: int = 0
    requirements: List[Req] = field(default_factory=list)
    labels: Dict[str, str] = field(default_factory=dict)
    taints: List[Tuple[str, str, str]] = field(default_factory=list)  # (key, value, effect)
    limits: Dict[str, int] = field(default_factory=dict)
    daemon_requests: Dict[str, int] = field(default_factory=dict)
    budgets: Optional[List[Budget]] = None  # None: not modelled (unlimited); the API server's default is [Budget("10%")]


@dataclass
class LabelSelector:
    """metav1.LabelSelector; match_expressions are (key, "In"|"NotIn"|"Exists"|"DoesNotExist", [values])."""
    match_labels: Dict[str, str] = field(default_factory=dict)
    match_expressions: List[Tuple[str, str, List[str]]] = field(default_factory=list)


@dataclass
class TopologySpread:
    """corev1.TopologySpreadConstraint. selector None = nil (selects nothing)."""
    topology_key: str
    max_skew: int = 1
    selector: Optional[LabelSelector] = None
    when_unsatisfiable: str = "DoNotSchedule"
    min_domains: Optional[int] = None
    node_affinity_policy: Optional[str] = None  # None = Honor
    node_taints_policy: Optional[str] = None    # None = Ignore


@dataclass
class PodAffinityTerm:
    """corev1.PodAffinityTerm (+ weight for a WeightedPodAffinityTerm). namespaces empty and no namespace_selector =
    the pod's namespace; a namespace_selector (LabelSelector; empty = every namespace) adds the problem's namespaces
    whose labels it matches (Problem.namespaces / Cluster.namespaces)."""
    topology_key: str
    selector: Optional[LabelSelector] = None
    namespaces: List[str] = field(default_factory=list)
    weight: int = 0
    namespace_selector: Optional[LabelSelector] = None


@dataclass
class PodShape:
    requests: Dict[str, int]
    node_selector: Dict[str, str] = field(default_factory=dict)
    required_terms: List[List[Req]] = field(default_factory=list)
    preferred_terms: List[Tuple[int, List[Req]]] = field(default_factory=list)
    tolerations: List[Tuple[str, str, str, str]] = field(default_factory=list)  # (key, op, value, effect)
    topology_spread: List[TopologySpread] = field(default_factory=list)
    labels: Dict[str, str] = field(default_factory=dict)
    namespace: str = "default"
    host_ports: List[Tuple[str, int, str]] = field(default_factory=list)  # GetHostPorts: (hostIP, hostPort, protocol)
    volume_requirements: List[Req] = field(default_factory=list)         # VolumeTopology.Inject input
    required_anti_affinity: List[PodAffinityTerm] = field(default_factory=list)
    preferred_anti_affinity: List[PodAffinityTerm] = field(default_factory=list)
    required_affinity: List[PodAffinityTerm] = field(default_factory=list)   # unsupported on the device path
    preferred_affinity: List[PodAffinityTerm] = field(default_factory=list)


@dataclass
class ExistingNode:
    name: str
    labels: Dict[str, str]
    available: Dict[str, int]
    requests: Dict[str, int] = field(default_factory=dict)
    taints: List[Tuple[str, str, str]] = field(default_factory=list)
    initialized: bool = True
    host_ports: List[Tuple[str, int, str]] = field(default_factory=list)  # HostPortUsage of its bound pods


@dataclass
class ClusterNode:
    """state.StateNode as disruption sees it: an existing node + its instance type + reschedulable pods."""
    node: ExistingNode
    catalog: int
    instance_type: int
    pods: List[int] = field(default_factory=list)   # indices into Cluster.pod_*
    deleting: bool = False                           # MarkedForDeletion: its pods join every simulation
    drifted: Optional[float] = None                  # transition time of its Drifted condition (None: not drifted)
    provider_id: Optional[str] = None                # the NodeClaim's status.providerID (kpamd.interruption reads it)


@dataclass
class PodDisruptionBudget:
    """policyv1.PodDisruptionBudget as disruption reads it: selector None = nil (selects nothing), LabelSelector() =
    every pod of the namespace; disruptions_allowed is status.disruptionsAllowed (0 blocks the pods it selects)."""
    namespace: str
    name: str
    selector: Optional[LabelSelector] = None
    disruptions_allowed: int = 0


@dataclass
class PoolControls:
    """NodePool spec.disruption: consolidationPolicy and consolidateAfter in seconds (None: Never)."""
    policy: str = "WhenEmptyOrUnderutilized"  # or "WhenEmpty"
    consolidate_after: Optional[int] = 0


@dataclass
class NodeControls:
    """What disruption reads of a node and its NodeClaim beyond the snapshot (times in unix seconds)."""
    do_not_disrupt: bool = False              # the node's karpenter.sh/do-not-disrupt annotation
    nominated: bool = False                   # nominated for a pending pod
    termination_grace_period: bool = False    # the NodeClaim has a terminationGracePeriod
    created: int = 0                          # creationTimestamp
    expire_after: Optional[int] = None        # expireAfter in seconds (None: Never)
    last_pod_event: int = 0                   # status.lastPodEventTime
    drifted: Optional[int] = None             # transition time of the Drifted condition (None: not drifted)


@dataclass
class DisruptionControls:
    """The inputs of candidate selection (kp_cluster_candidates): pools indexed like Cluster.nodepools, nodes like
    Cluster.nodes, the pod arrays like Cluster.pod_shape."""
    pools: List[PoolControls]
    nodes: List[NodeControls]
    pod_priority: np.ndarray                  # int32 [P] spec.priority (nil: 0)
    pod_deletion_cost: np.ndarray             # int32 [P] controller.kubernetes.io/pod-deletion-cost (absent: 0)
    pod_do_not_disrupt: np.ndarray            # bool [P] the pod's karpenter.sh/do-not-disrupt annotation
    pdbs: List[PodDisruptionBudget] = field(default_factory=list)

    @classmethod
    def default(cls, cluster):
        """Nothing set: every pod at the default priority and deletion cost, no expiry, consolidateAfter 0s; the
        Drifted times are taken from ClusterNode.drifted."""
        P = len(cluster.pod_shape)
        return cls([PoolControls() for _ in cluster.nodepools],
                   [NodeControls(drifted=None if n.drifted is None else int(n.drifted)) for n in cluster.nodes],
                   np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, bool))


@dataclass
class AMI:
    """One entry of EC2NodeClass status.amis: the image id and the requirements an instance type must be compatible with."""
    id: str
    requirements: List[Req] = field(default_factory=list)


@dataclass
class NodeClassStatus:
    """EC2NodeClass as drift detection reads it (R:pkg/cloudprovider/drift.go): the ec2nodeclass-hash annotations
    (None: absent) and the status lists, amis in status order."""
    amis: List[AMI] = field(default_factory=list)
    subnets: List[str] = field(default_factory=list)
    security_groups: List[str] = field(default_factory=list)
    capacity_reservations: List[str] = field(default_factory=list)
    hash: Optional[str] = None
    hash_version: Optional[str] = None


@dataclass
class InstanceInfo:
    """The EC2 instance behind a NodeClaim's provider id."""
    image_id: str
    subnet_id: str
    security_groups: List[str] = field(default_factory=list)
    capacity_reservation_id: Optional[str] = None


@dataclass
class PoolDrift:
    """A NodePool's side of drift detection: the index of its EC2NodeClass in DriftInputs.nodeclasses (-1: no
    nodeClassRef, or unresolved) and its karpenter.sh/nodepool-hash annotations (None: absent)."""
    nodeclass: int = -1
    hash: Optional[str] = None
    hash_version: Optional[str] = None


@dataclass
class NodeDrift:
    """A NodeClaim's side: its four hash annotations (None: absent) and its instance (None: no provider id / no record)."""
    nodepool_hash: Optional[str] = None
    nodepool_hash_version: Optional[str] = None
    nodeclass_hash: Optional[str] = None
    nodeclass_hash_version: Optional[str] = None
    instance: Optional[InstanceInfo] = None


@dataclass
class DriftInputs:
    """The inputs of drift detection (kp_cluster_detect_drift): pools indexed like Cluster.nodepools, nodes like
    Cluster.nodes."""
    nodeclasses: List[NodeClassStatus]
    pools: List[PoolDrift]
    nodes: List[NodeDrift]


@dataclass
class SchedNode:
    """A node as kp_scheduler_inputs reads it: labels and taints as an ExistingNode carries them, status.allocatable
    and status.capacity, and the pods bound to it as (requests, a DaemonSet owns it)."""
    name: str
    labels: Dict[str, str]
    taints: List[Tuple[str, str, str]] = field(default_factory=list)
    allocatable: Dict[str, int] = field(default_factory=dict)
    capacity: Dict[str, int] = field(default_factory=dict)
    pods: List[Tuple[Dict[str, int], bool]] = field(default_factory=list)


@dataclass
class SchedulerState:
    """The inputs of kp_scheduler_inputs: the NodePools with spec.limits in `limits` (daemon_requests is ignored), the
    DaemonSets' pod templates, and the nodes (in the order of Problem.existing / Cluster.nodes where the result is
    applied to one)."""
    nodepools: List[NodePool]
    daemonsets: List["PodShape"]
    nodes: List[SchedNode]


@dataclass
class Cluster:
    catalogs: List[List[InstanceType]]
    nodepools: List[NodePool]
    nodes: List[ClusterNode]
    shapes: List[PodShape]
    pod_shape: np.ndarray
    pod_creation: np.ndarray
    pod_uid: np.ndarray
    candidates: List[int] = field(default_factory=list)  # disruption-cost order
    name: str = ""
    pending: List[int] = field(default_factory=list)  # provisionable pods bound to no node (indices into pod_*)
    spot_to_spot: bool = False                         # SpotToSpotConsolidation feature gate
    namespaces: Dict[str, Dict[str, str]] = field(default_factory=dict)  # cluster namespaces: name -> labels
    pod_uid_str: Optional[List[str]] = None  # metadata.uid per pod (kp_cluster.pod_uids): the exact Queue tie-break
    controls: Optional[DisruptionControls] = None  # None: not modelled (candidate_order / drift_order decide)
    drift_inputs: Optional[DriftInputs] = None     # None: not modelled (ClusterNode.drifted is given)


@dataclass
class Problem:
    catalogs: List[List[InstanceType]]
    nodepools: List[NodePool]
    shapes: List[PodShape]
    pod_shape: np.ndarray           # uint32 [P]
    pod_creation: np.ndarray        # int64 [P]
    pod_uid: np.ndarray             # uint64 [P] (order-preserving UID key)
    existing: List[ExistingNode] = field(default_factory=list)
    max_instance_types: int = 100
    name: str = ""
    bound_pods: List[Tuple[str, Dict[str, str], int]] = field(default_factory=list)  # (namespace, labels, existing idx)
    namespaces: Dict[str, Dict[str, str]] = field(default_factory=dict)  # cluster namespaces: name -> labels
    reserved_offering_mode: int = 0  # 0 fallback (scheduler default), 1 strict (provisioner: DisableReservedCapacityFallback)
    pod_uid_str: Optional[List[str]] = None  # metadata.uid per pod (kp_solve_in.pod_uids): NewQueue's exact UID tie-break

    @property
    def n_pods(self):
        return int(len(self.pod_shape))


MI = 1 << 20
GI = 1 << 30


def cpu(m):
    return int(m)


def mem_mi(x):
    return int(x) * MI * 1000
