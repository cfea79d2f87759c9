/*
 * kp_abi.h — C ABI of the MI355X-native Karpenter bin-packing hot path.
 *
 * This is the drop-in boundary a Go cgo shim binds. Every entry point
 * replaces one reference surface:
 *
 *   kp_catalog_upload      <- cloudprovider.CloudProvider.GetInstanceTypes result
 *                             (R:pkg/cloudprovider/cloudprovider.go:177-193 -> instancetype.DefaultProvider.List
 *                              R:pkg/providers/instancetype/instancetype.go:129-171 + offering.InjectOfferings
 *                              R:pkg/providers/instancetype/offering/offering.go:68-98), resident on device
 *                             until its seqnum changes (R:instancetype.go:225-237 cacheKey).
 *   kp_instance_type_resolve <- instancetype.NewInstanceType (R:pkg/providers/instancetype/types.go:123-155)
 *   kp_catalog_compile     <- the capacity / overhead and offering halves of that result for every EC2NodeClass in one
 *                             call (NewInstanceType + createOfferings per (NodeClass, type) pair, on the device)
 *   kp_filter_compatible_available <- filter.CompatibleAvailableFilter
 *                             (R:pkg/providers/instance/filter/filter.go:39-64), batched: many
 *                             (requirements, requests) rows × one catalogue on the GPU.
 *   kp_launch_select       <- instance.DefaultProvider.Create's launch-side selection
 *                             (R:pkg/providers/instance/instance.go:117-125 Create -> filterInstanceTypes :242-270,
 *                              getCapacityType :504-518, checkODFallback :336-355, getOverrides :392-439), batched:
 *                             one row per NodeClaim being launched.
 *   kp_launch_templates    <- the same followed by getLaunchTemplateConfigs (R:instance.go:356-388): the grouping of
 *                             MapToInstanceTypes (R:pkg/providers/amifamily/ami.go:222-235) and DefaultResolver.Resolve
 *                             (R:pkg/providers/amifamily/resolver.go:126-188) with each template's overrides.
 *   kp_solve               <- upstream scheduling.Scheduler.Solve (sigs.k8s.io/karpenter
 *                             pkg/controllers/provisioning/scheduling/scheduler.go), reached from
 *                             R:pkg/providers/instancetype/suite_test.go:93,279 (NewProvisioner/ExpectProvisioned),
 *                             followed by Results.TruncateInstanceTypes(MaxInstanceTypes).
 *   kp_cluster_simulate / kp_consolidate_argmin <- upstream disruption computeConsolidation over candidate subsets
 *                             (R:website/content/en/preview/concepts/disruption.md:89-128); the _budgeted forms also
 *                             apply the NodePools' disruption budgets (disruption.md:274-333) per subset on the device.
 *   kp_cluster_command     <- the Command computeConsolidation returns: the replacement NodeClaim (options after the
 *                             price filters, requirements, requests, pods) and where every rescheduled pod went.
 *   kp_cluster_validate    <- upstream Validation.ValidateCommand: the command re-simulated on a plan of current state
 *                             and accepted only if the new simulation agrees with it.
 *   kp_cluster_candidates  <- upstream disruption GetCandidates: which nodes a method may disrupt, why not the others
 *                             (do-not-disrupt, PDBs, consolidateAfter, ...), and the disruption-cost order.
 *   kp_cluster_simulate_explained <- the exits of computeConsolidation behind the Unconsolidatable events: the
 *                             decisions of kp_cluster_simulate_budgeted plus, per subset, which exit made it a no-op.
 *
 * Conventions
 *   - Every function returns int32: KP_OK (0) or a negative KP_E_* code. kp_last_error() gives text.
 *     KP_E_UNSUPPORTED means the input uses a feature the device path does not implement; the Go
 *     shim then runs the original CPU path.
 *   - Caller owns every input buffer; nothing is retained after a call returns (catalogues copy).
 *   - Quantities are int64 milli-units (resource.Quantity.MilliValue()): cpu "1" = 1000,
 *     memory "1Mi" = 1048576000. kp_resource_list.present marks which resources are set; it
 *     matters only for NodePool limits (R: upstream filterByRemainingResources iterates limit keys).
 *   - No C++ exceptions and no torch types cross this boundary.
 */
#ifndef KP_ABI_H
#define KP_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KP_ABI_VERSION 13

enum kp_status {
  KP_OK = 0,
  KP_E_INVAL = -1,
  KP_E_NOMEM = -2,
  KP_E_DEVICE = -3,
  KP_E_UNSUPPORTED = -4,
  KP_E_NOTFOUND = -5,
  KP_E_CANCELED = -6, /* ABI v11: the caller's kp_cancel token was set while the call ran (ctx.Done) */
};

/* Resource axis, fixed (R:pkg/providers/instancetype/types.go:317-329,151-153; R:pkg/apis/v1/labels.go:69-81). */
enum kp_resource {
  KP_RES_CPU = 0,
  KP_RES_MEMORY = 1,
  KP_RES_EPHEMERAL_STORAGE = 2,
  KP_RES_PODS = 3,
  KP_RES_POD_ENI = 4,        /* vpc.amazonaws.com/pod-eni */
  KP_RES_EFA = 5,            /* vpc.amazonaws.com/efa */
  KP_RES_NVIDIA_GPU = 6,     /* nvidia.com/gpu */
  KP_RES_AMD_GPU = 7,        /* amd.com/gpu */
  KP_RES_NEURON = 8,         /* aws.amazon.com/neuron */
  KP_RES_NEURONCORE = 9,     /* aws.amazon.com/neuroncore */
  KP_RES_GAUDI = 10,         /* habana.ai/gaudi */
  KP_RES_PRIVATE_IPV4 = 11,  /* vpc.amazonaws.com/PrivateIPv4Address */
  KP_NUM_RESOURCES = 12
};

typedef struct kp_resource_list {
  int64_t milli[KP_NUM_RESOURCES];
  uint32_t present; /* bit r set <=> resource r present in the ResourceList */
  uint32_t reserved_;
} kp_resource_list;

/* corev1.NodeSelectorOperator */
enum kp_operator {
  KP_OP_IN = 0,
  KP_OP_NOT_IN = 1,
  KP_OP_EXISTS = 2,
  KP_OP_DOES_NOT_EXIST = 3,
  KP_OP_GT = 4,
  KP_OP_LT = 5
};

/* scheduling.NewRequirementWithFlexibility(key, op, minValues, values...) */
typedef struct kp_requirement {
  const char* key;
  int32_t op;          /* enum kp_operator */
  int32_t min_values;  /* < 0: nil */
  const char* const* values;
  uint32_t n_values;
  uint32_t reserved_;
} kp_requirement;

typedef struct kp_requirements {
  const kp_requirement* items;
  uint32_t n;
  uint32_t reserved_;
} kp_requirements;

typedef struct kp_label {
  const char* key;
  const char* value;
} kp_label;

enum kp_taint_effect {
  KP_EFFECT_ANY = 0, /* tolerations only: empty effect matches all */
  KP_EFFECT_NO_SCHEDULE = 1,
  KP_EFFECT_PREFER_NO_SCHEDULE = 2,
  KP_EFFECT_NO_EXECUTE = 3
};

typedef struct kp_taint {
  const char* key;
  const char* value;
  int32_t effect;
  int32_t reserved_;
} kp_taint;

enum kp_toleration_operator { KP_TOL_EQUAL = 0, KP_TOL_EXISTS = 1 };

typedef struct kp_toleration {
  const char* key;   /* "" or NULL: any key (requires KP_TOL_EXISTS) */
  const char* value;
  int32_t op;        /* enum kp_toleration_operator */
  int32_t effect;    /* enum kp_taint_effect; KP_EFFECT_ANY = all effects */
} kp_toleration;

/* cloudprovider.Offering as built by createOfferings (R:offering.go:115-147). */
typedef struct kp_offering {
  const char* capacity_type; /* karpenter.sh/capacity-type In {capacity_type} */
  const char* zone;          /* topology.kubernetes.io/zone In {zone}; NULL: no zone requirement */
  const char* zone_id;       /* topology.k8s.aws/zone-id In {zone_id}; NULL: no zone-id requirement */
  const char* reservation_id;   /* capacity-reservation-id In {id}; NULL: DoesNotExist (R:offering.go:136) */
  const char* reservation_type; /* capacity-reservation-type In {type}; NULL: DoesNotExist (R:offering.go:137) */
  double price;              /* a number >= 0 (+inf allowed): a negative or NaN price is refused with KP_E_INVAL by
                                kp_catalog_upload and kp_catalog_update_offerings, -0.0 is stored as +0.0. The device
                                orders prices by their bit patterns, which equals < on this domain only. */
  int32_t available;
  int32_t reservation_capacity; /* Offering.ReservationCapacity (R:offering.go:178): read by ReservedOfferingFilter.
                                   Filter and launch plans take reserved offerings (ABI v7), Solve plans too (ABI
                                   v9: NodeClaim.reserveOfferings against each reservation's capacity, see
                                   kp_solve_in.reserved_offering_mode), cluster plans too (ABI v10: every simulation
                                   reserves strictly, as SimulateScheduling's DisableReservedCapacityFallback) */
} kp_offering;

/* cloudprovider.InstanceType after InjectOfferings. */
typedef struct kp_instance_type {
  const char* name;
  kp_requirements requirements;
  kp_resource_list capacity;
  kp_resource_list overhead; /* Overhead.Total() = kube-reserved + system-reserved + eviction */
  const kp_offering* offerings;
  uint32_t n_offerings;
  uint32_t reserved_;
} kp_instance_type;

typedef struct kp_catalog_desc {
  const kp_instance_type* types;
  uint32_t n_types;
  uint32_t reserved_;
} kp_catalog_desc;

/* NodePool -> NodeClaimTemplate (upstream NewNodeClaimTemplate). Order does not matter: the solver
 * orders pools by weight desc then name asc (upstream nodepoolutils.OrderByWeight). */
typedef struct kp_nodepool {
  const char* name;
  int32_t weight;
  uint32_t catalog; /* index into kp_solve_in.catalogs / catalog_descs: GetInstanceTypes(nodePool) */
  kp_requirements requirements;  /* spec.template.spec.requirements (minValues allowed) */
  const kp_label* labels;        /* spec.template.metadata.labels (karpenter.sh/nodepool is added) */
  uint32_t n_labels;
  uint32_t n_taints;
  const kp_taint* taints;        /* spec.template.spec.taints */
  kp_resource_list limits;       /* remaining limits (spec.limits minus existing capacity); present = limited */
  kp_resource_list daemon_requests; /* daemonset overhead for this template */
} kp_nodepool;

typedef struct kp_preferred_term {
  int32_t weight;
  int32_t reserved_;
  kp_requirements preference;
} kp_preferred_term;

/* metav1.LabelSelector: matchLabels AND matchExpressions (In / NotIn / Exists / DoesNotExist). A nil selector
 * (is_nil != 0) selects nothing; an empty one selects everything (metav1.LabelSelectorAsSelector). */
enum kp_selector_operator { KP_SEL_IN = 0, KP_SEL_NOT_IN = 1, KP_SEL_EXISTS = 2, KP_SEL_DOES_NOT_EXIST = 3 };
typedef struct kp_selector_requirement {
  const char* key;
  int32_t op;        /* enum kp_selector_operator */
  uint32_t n_values;
  const char* const* values;
} kp_selector_requirement;
typedef struct kp_label_selector {
  const kp_label* match_labels;
  uint32_t n_match_labels;
  uint32_t n_match_expressions;
  const kp_selector_requirement* match_expressions;
  int32_t is_nil;
  int32_t reserved_;
} kp_label_selector;

/* corev1.TopologySpreadConstraint (upstream scheduling.TopologyGroup of TopologyTypeSpread). */
enum kp_when_unsatisfiable { KP_DO_NOT_SCHEDULE = 0, KP_SCHEDULE_ANYWAY = 1 };
enum kp_inclusion_policy { KP_POLICY_UNSET = 0, KP_POLICY_HONOR = 1, KP_POLICY_IGNORE = 2 };
typedef struct kp_topology_spread {
  const char* topology_key;
  int32_t max_skew;
  int32_t min_domains;          /* <= 0: nil */
  int32_t when_unsatisfiable;   /* ScheduleAnyway constraints are dropped one by one by Preferences.Relax */
  int32_t node_affinity_policy; /* UNSET = Honor */
  int32_t node_taints_policy;   /* UNSET = Ignore */
  int32_t reserved_;
  kp_label_selector selector;
} kp_topology_spread;

/* corev1.PodAffinityTerm (ABI v6): pod affinity / anti-affinity on the hostname or a label key (upstream
 * TopologyGroup of TopologyTypePodAffinity / TopologyTypePodAntiAffinity, and the inverse groups bound pods' required
 * anti-affinity terms create). The namespaces a term selects (upstream Topology.buildNamespaceList): no namespaces
 * and no namespaceSelector -> the pod's own namespace; else `namespaces` plus every namespace of
 * kp_solve_in.namespaces / kp_cluster.namespaces whose labels namespace_selector matches (ABI v8; an empty
 * selector matches them all). */
typedef struct kp_pod_affinity_term {
  const char* topology_key;
  kp_label_selector selector;
  const char* const* namespaces;  /* n_namespaces == 0 and no namespace selector: the pod's own namespace */
  uint32_t n_namespaces;
  int32_t weight;                 /* preferred terms: WeightedPodAffinityTerm.weight */
  int32_t has_namespace_selector; /* != 0: namespaceSelector set (namespace_selector) */
  int32_t reserved_;
  kp_label_selector namespace_selector;
} kp_pod_affinity_term;

/* A namespace of the cluster and its labels (ABI v8): what a namespaceSelector lists (corev1.NamespaceList). */
typedef struct kp_namespace {
  const char* name;
  const kp_label* labels;
  uint32_t n_labels;
  uint32_t reserved_;
} kp_namespace;

/* A container port with hostPort != 0, as upstream scheduling.GetHostPorts reads it (HostPortUsage). Two entries
 * conflict when protocol and port are equal and either IP is unspecified (0.0.0.0 / ::) or both IPs are equal. */
enum kp_protocol { KP_PROTO_TCP = 0, KP_PROTO_UDP = 1, KP_PROTO_SCTP = 2 };
typedef struct kp_host_port {
  const char* ip;     /* hostIP; NULL or "" = 0.0.0.0 (corev1 default) */
  int32_t port;       /* hostPort, 1..65535 */
  int32_t protocol;   /* enum kp_protocol; corev1 default TCP */
} kp_host_port;

/* A pod "shape": everything the scheduler reads from a pod except its identity. */
typedef struct kp_pod_shape {
  kp_resource_list requests;                 /* resources.RequestsForPods(pod) */
  const kp_label* node_selector;
  uint32_t n_node_selector;
  uint32_t n_required_terms;
  const kp_requirements* required_terms;     /* nodeAffinity required NodeSelectorTerms (ORed) */
  const kp_preferred_term* preferred_terms;  /* nodeAffinity preferred terms */
  uint32_t n_preferred_terms;
  uint32_t n_tolerations;
  const kp_toleration* tolerations;
  uint32_t n_topology_spread;
  uint32_t n_labels;
  const kp_topology_spread* topology_spread; /* spec.topologySpreadConstraints, in spec order */
  const char* namespace_;                    /* metadata.namespace (topology selectors are namespaced) */
  const kp_label* labels;                    /* metadata.labels (matched by topology selectors) */
  /* ABI v6 */
  const kp_host_port* host_ports;            /* GetHostPorts(pod): NodeClaim.Add / ExistingNode.CanAdd conflicts */
  uint32_t n_host_ports;
  uint32_t n_volume_requirements;
  /* VolumeTopology.Inject: the topology requirements of the pod's volumes (PV node affinity / StorageClass
   * allowedTopologies, resolved by the caller), appended to every required node-affinity term (one term is
   * created when the pod has none) before scheduling. */
  const kp_requirement* volume_requirements;
  /* podAntiAffinity and podAffinity required / preferred terms. Preferred terms act as required until
   * Preferences.Relax removes them, heaviest first (affinity terms before anti-affinity terms). */
  const kp_pod_affinity_term* required_anti_affinity;
  const kp_pod_affinity_term* preferred_anti_affinity;
  const kp_pod_affinity_term* required_affinity;
  const kp_pod_affinity_term* preferred_affinity;
  uint32_t n_required_anti_affinity;
  uint32_t n_preferred_anti_affinity;
  uint32_t n_required_affinity;
  uint32_t n_preferred_affinity;
} kp_pod_shape;

/* A pod already bound to a node of the cluster: what upstream Topology.countDomains lists (through the
 * kube client) to seed the domain counts of every topology group whose selector matches it. */
typedef struct kp_bound_pod {
  const char* namespace_;
  const kp_label* labels;
  uint32_t n_labels;
  uint32_t node;  /* index into kp_solve_in.existing */
  /* ABI v6: its required podAntiAffinity terms (Topology.updateInverseAntiAffinity: pods the selector selects
   * avoid the bound pod's domain) */
  const kp_pod_affinity_term* anti_affinity;
  uint32_t n_anti_affinity;
  uint32_t reserved_;
} kp_bound_pod;

typedef struct kp_pod {
  uint32_t shape;
  uint32_t reserved_;
  int64_t creation_unix;  /* metadata.creationTimestamp (1 s resolution, as in the API) */
  uint64_t uid_key;       /* order-preserving key of metadata.uid (string order of UIDs); ignored when the batch
                             passes the UIDs themselves (kp_solve_in.pod_uids / kp_cluster.pod_uids, ABI v10) */
} kp_pod;

/* In-flight or real node already in the cluster (upstream ExistingNode). */
typedef struct kp_existing_node {
  const char* name;
  const kp_label* labels;   /* node labels -> NewLabelRequirements */
  uint32_t n_labels;
  uint32_t n_taints;
  const kp_taint* taints;
  kp_resource_list available;  /* cachedAvailable: allocatable minus bound pods' requests */
  kp_resource_list requests;   /* initial requests: daemonset pods expected but not yet bound */
  int32_t initialized;
  int32_t reserved_;
  /* ABI v6: HostPortUsage of the pods bound to the node (in a kp_cluster: every bound pod, reschedulable or not) */
  const kp_host_port* host_ports;
  uint32_t n_host_ports;
  uint32_t reserved2_;
} kp_existing_node;

typedef struct kp_ctx kp_ctx;
typedef struct kp_catalog kp_catalog;
typedef struct kp_solve_result kp_solve_result;
typedef struct kp_solve_plan kp_solve_plan;

typedef struct kp_solve_in {
  const kp_catalog* const* catalogs;      /* device path: resident catalogue handles */
  const kp_catalog_desc* catalog_descs;   /* CPU oracle path: the same catalogues as plain arrays */
  uint32_t n_catalogs;
  uint32_t n_nodepools;
  const kp_nodepool* nodepools;
  const kp_existing_node* existing;
  uint32_t n_existing;
  uint32_t n_shapes;
  const kp_pod_shape* shapes;
  const kp_pod* pods;
  uint32_t n_pods;
  uint32_t max_instance_types;  /* scheduling.MaxInstanceTypes = 100; 0 = no truncation */
  const kp_bound_pod* bound_pods;  /* pods running on existing nodes (topology domain counts) */
  uint32_t n_bound_pods;
  uint32_t n_namespaces;           /* ABI v8: the cluster's namespaces (pod affinity namespaceSelector) */
  const kp_namespace* namespaces;
  /* ABI v9: capacity reservations inside the Solve (upstream NodeClaim.Add reserveOfferings + ReservationManager,
   * designed in R:designs/odcr.md:248-256): KP_RESERVED_FALLBACK (0, the scheduler's default) never fails an Add for
   * want of reservation capacity; KP_RESERVED_STRICT (1, the provisioner's DisableReservedCapacityFallback) fails an
   * Add whose NodeClaim is compatible with reserved offerings it cannot reserve, and does not relax the pod then. */
  uint32_t reserved_offering_mode;
  uint32_t reserved2_;
  /* ABI v10: metadata.uid of every pod (n_pods strings), or NULL. Given, the Queue's last tie-break (upstream NewQueue:
   * creationTimestamp, then UID) compares the UIDs as strings, exactly; kp_pod.uid_key is then ignored. */
  const char* const* pod_uids;
} kp_solve_in;

#define KP_RESERVED_FALLBACK 0
#define KP_RESERVED_STRICT 1

typedef struct kp_nodeclaim_info {
  uint32_t nodepool;        /* index into kp_solve_in.nodepools */
  uint32_t n_pods;
  uint32_t n_remaining;     /* InstanceTypeOptions before truncation */
  uint32_t n_options;       /* after OrderByPrice + Truncate */
  const uint32_t* pods;     /* pod indices in the order they were added */
  const uint32_t* options;  /* catalogue indices, cheapest-compatible-offering price asc then name asc */
  kp_resource_list requests;
  /* the NodeClaim's Requirements after FinalizeScheduling (hostname placeholder removed) as upstream
   * Requirements.NodeSelectorRequirements() renders them (Gt/Lt win over NotIn values): keys in byte order,
   * values sorted. Owned by the result. Topology spread narrows keys here (e.g. zone In {one zone}). */
  kp_requirements requirements;
} kp_nodeclaim_info;

typedef struct kp_solve_stats {
  double device_ms;         /* solve + finalize kernel time, HIP events on the solve stream */
  double host_ms;           /* kp_solve_run wall time (restore state, kernels, result copy-back) */
  double prepare_ms;        /* kp_solve_prepare wall time (compile + upload) */
  double solve_kernel_ms;   /* solve_kernel alone */
  double finalize_kernel_ms;
  uint64_t attempts;        /* NodeClaim.Add / ExistingNode.CanAdd evaluations */
  uint64_t bytes_algorithmic; /* bytes the device algorithm reads+writes */
  uint64_t pops;            /* queue pops */
  uint64_t phase_cycles[8]; /* diagnostic (KP_TIMING=1): per-phase shader cycles of the solve loop */
  uint64_t scanned;         /* diagnostic: in-flight NodeClaim positions the candidate pre-pass visited */
  uint64_t cursor_starts;   /* diagnostic: sum of first-fit cursor start positions (positions skipped) */
  uint64_t attempt_cycles[8]; /* diagnostic (KP_TIMING=1): wave 0's in-flight attempt split (merge, pod keys,
                                 Fits, offerings, minValues; [5] = attempts timed) */
  double catalog_ms;        /* part of prepare_ms spent compiling the catalogue half (dictionary, catalogue SoA,
                               NodeClaimTemplates); 0 when it came resident from the kp_ctx cache */
  uint32_t catalog_cached;  /* 1: the catalogue half was resident (same catalogues + NodePools; seqnums equal, or
                               re-applied in place: catalog_refreshed) */
  uint32_t catalog_refreshed; /* 1: the catalogues' seqnums had changed (ICE marks, prices) and the resident half's
                                 offerings and template options were re-applied in place, not recompiled */
  uint64_t fast_pods;       /* pods placed by solve_kernel's single-wave fast lane (no requirement merge) */
  uint64_t fast_cycles[6];  /* diagnostic (KP_TIMING=1): fast-lane cycles: pop, stage, sort, pre-pass, attempts, commit */
  uint64_t slow_sorts;      /* sort.Slice replays that ran the literal pdqsort (no stable-move shortcut) */
  uint64_t fast_bails[8];   /* pods the fast lane handed to the full path: ineligible (topology / existing nodes),
                               spilled sort arrays, long sort shift, long scan, requirement merge, minValues,
                               no in-flight NodeClaim took it, reserved */
  uint64_t reserved_offering_errors; /* ABI v9: pops whose addToNewNodeClaim failed on a ReservedOfferingError (strict
                                        mode; upstream Results.ReservedOfferingErrors: deferred, not relaxed) */
  uint64_t run_length_pods; /* ABI v11: pods the fast lane committed as part of a run (queue runs of one shape-level
                               onto one NodeClaim, committed k at a time: solve_kernel's run-length commit; with the
                               open set, the pods its loop placed on the NodeClaim of the pod before them: those it
                               places on another open NodeClaim are not counted, so the figure stays bounded by the
                               queue neighbours of one request row on one NodeClaim) */
  uint64_t order_chunks[5]; /* ABI v10, diagnostic: the chunked newNodeClaims order past the LDS sort capacity: peak
                               chunks, chunk splits, emptied chunks, directory (re)builds, final order mode (1 LDS,
                               2 chunked, 0 flat global) */
} kp_solve_stats;

/* ---- context ---------------------------------------------------------------------------- */
typedef struct kp_options {
  double vm_memory_overhead_percent; /* R:pkg/operator/options/options.go:53 default 0.075 */
  int32_t reserved_enis;             /* R:pkg/operator/options/options.go:55 default 0 */
  int32_t device;                    /* HIP device ordinal */
} kp_options;

int32_t kp_ctx_create(const kp_options* opts, kp_ctx** out);
/* ABI v12: test and measurement overrides of the library's kernel and path choices. Every field 0 (the state a context
 * is created in) is the production choice; no environment variable changes a path (a stray variable in the
 * controller's environment cannot pick another kernel). Cross-check tests and benchmarks set them per context,
 * between calls (not while a call on the context runs). ABI v13 appends sim_slots and general_launch, which shrink a
 * launch so that small inputs reach the states a full-size sweep runs in (a wave reusing its slot across subsets, a
 * general-path launch reusing a dirty arena). Both are read from the context by each simulate / argmin call, not when
 * the plan was prepared: setting them takes effect on the next call on any existing plan. */
typedef struct kp_overrides {
  int32_t fast_lane;           /* 0 auto (the run-length-commit variant where most queue neighbours share their shape),
                                  1 the plain variant, 2 the run-length-commit variant with the continuation round,
                                  3 the run-length-commit variant without it, 4 (the one auto picks for queue runs of
                                  different shapes with one request row) variant 3 with the open set in place of
                                  the closed-form commit: the entries after an append are placed one at a time on the
                                  last few NodeClaims committed to, from state held on chip. Solves for which 2, 3 or
                                  4 is not built (topology, existing nodes, a spilled order) run the plain variant */
  int32_t sort_capacity;       /* 0: 8192 NodeClaims in the LDS order; n > 0: the chunked order past n NodeClaims */
  int32_t chunk_capacity;      /* 0: the chunked order's full directory; n > 0: at most n chunks (then the flat order);
                                  n < 0: no chunks (the flat order past sort_capacity) */
  int32_t template_table;      /* 0: Solve reads the template-options table; 1: it re-filters per template attempt */
  uint64_t table_shard_min;    /* 0: 1 << 20 (shape-level, template) pairs before a communicator shards the table */
  int32_t general_batch;       /* 0: batched general simulations (superset Solve); 1: every subset compiled alone */
  int32_t feasibility_kernel;  /* 0 by catalogue size (quad <= 1024 types, else bits); 1 the per-type global-gather
                                  kernel; 2 the one-row bits kernel at any size */
  int32_t feasibility_blocks;  /* 0: by row count; n > 0: n blocks */
  int32_t feasibility_temporal;/* 0: cheapest-price rows as non-temporal stores; 1: temporal stores */
  int32_t timing;              /* 1: solve_kernel phase probes (kp_solve_stats phase_cycles / fast_cycles) */
  int32_t host_timing;         /* 1: host compile / general-path phases on stderr */
  int32_t sim_slots;           /* ABI v13. 0: the batched sweep's grid by CU count; n > 0: at most ceil(n / 4) workgroups
                                  (4 wave slots each), never more than the production grid */
  int32_t general_launch;      /* ABI v13. 0: general-path simulations per launch by free memory (at most 4096);
                                  n > 0: at most n per launch */
} kp_overrides;
int32_t kp_ctx_set_overrides(kp_ctx* ctx, const kp_overrides* ov); /* NULL: back to all 0 */
int32_t kp_ctx_get_overrides(const kp_ctx* ctx, kp_overrides* out);
/* Drops the caller's reference. Catalogues, plans and communicators created on the context hold their own, so they
 * may be destroyed before or after it (a garbage collector finalizes in any order); the context's stream, events and
 * spare arena are freed with the last reference. */
void kp_ctx_destroy(kp_ctx* ctx);
const char* kp_last_error(void);
int32_t kp_abi_version(void);

/* ---- catalogue ---------------------------------------------------------------------------- */
/* ctx may be NULL for a host-only catalogue (kp_solve_validate); device entry points need a ctx one. */
int32_t kp_catalog_upload(kp_ctx* ctx, const kp_catalog_desc* desc, uint64_t seqnum, kp_catalog** out);
uint64_t kp_catalog_seqnum(const kp_catalog* cat);
uint32_t kp_catalog_size(const kp_catalog* cat);
void kp_catalog_destroy(kp_catalog* cat);

/* Offering availability / price change on a resident catalogue: the UnavailableOfferings.MarkUnavailable ->
 * SeqNum bump -> InjectOfferings rebuild of the reference (R:pkg/cache/unavailableofferings.go:66-92,
 * R:pkg/providers/instancetype/offering/offering.go:68-147, cache key R:offering.go:189-207) without re-parsing
 * the types. An update names an existing offering by (type index, capacity type, zone): every offering of that
 * type with that capacity type and zone (NULL zone: the offerings without a zone requirement) takes `available`
 * and, when price is not NaN, `price`. All-or-nothing: KP_E_INVAL (nothing changed) if any update names no
 * offering. On success the catalogue's seqnum becomes `seqnum`. */
typedef struct kp_offering_update {
  uint32_t type;              /* index into the uploaded types */
  int32_t available;          /* 0: ICE / unavailable, 1: available */
  const char* capacity_type;
  const char* zone;
  double price;               /* NaN: keep (so a NaN price cannot be set); else kp_offering.price's domain */
  /* ABI v7: capacity reservations (capacityreservation.Provider.MarkUnavailable / GetAvailableInstanceCount,
   * R:pkg/providers/instance/instance.go:470-484): a non-NULL reservation_id narrows the match to that
   * reservation's offerings; reservation_capacity >= 0 sets ReservationCapacity (-1: keep). */
  const char* reservation_id;
  int32_t reservation_capacity;
  int32_t reserved_;
} kp_offering_update;
int32_t kp_catalog_update_offerings(kp_catalog* cat, const kp_offering_update* updates, uint32_t n, uint64_t seqnum);

/* EC2 facts the reference reads from ec2types.InstanceTypeInfo (+ the static tables it joins). */
typedef struct kp_ec2_info {
  const char* name;
  int32_t vcpu;
  int32_t reserved0_;
  int64_t memory_mib;
  const char* arch;               /* "amd64" | "arm64" (already mapped via AWSToKubeArchitectures) */
  const char* hypervisor;
  int32_t encryption_in_transit;
  int32_t clock_mhz;              /* 0: no ProcessorInfo clock */
  const char* cpu_manufacturer;   /* "" : none */
  int64_t ebs_bandwidth_mbps;     /* 0: not EBS-optimized by default */
  int64_t network_bandwidth_mbps; /* 0: not in the bandwidth table */
  int64_t local_nvme_gb;          /* 0: none */
  const char* gpu_name;           /* "" : no GPU */
  const char* gpu_manufacturer;
  int32_t gpu_count;
  int32_t reserved1_;
  int64_t gpu_memory_mib;
  const char* accel_name;         /* "" : none */
  const char* accel_manufacturer;
  int32_t accel_count;
  int32_t neuron_devices;         /* NeuronInfo */
  int32_t neuron_cores_per_device;
  int32_t efa;
  int32_t max_enis;               /* NetworkCards[DefaultNetworkCardIndex].MaximumNetworkInterfaces */
  int32_t ipv4_per_eni;
  int32_t trunking;               /* Limits[name].IsTrunkingCompatible */
  int32_t branch_enis;            /* Limits[name].BranchInterface */
  int32_t in_limits_table;        /* name present in zz_generated.vpclimits.go */
  int32_t instance_storage_gb;    /* ABI v10: InstanceStorageInfo.TotalSizeInGB (any disk type); 0: local_nvme_gb */
} kp_ec2_info;

/* One kubelet eviction-signal value (memory.available / nodefs.available): a quantity or a percentage of the
 * node's capacity (R:pkg/providers/instancetype/types.go:571-598, computeEvictionSignal / mustParsePercentage). */
typedef struct kp_eviction_value {
  int32_t set;                   /* 0: the key is absent from the map */
  int32_t is_percent;            /* 1: "<p>%" (percent holds p; 100 disables the threshold) */
  double percent;
  int64_t milli;                 /* quantity in milli-units (resource.Quantity.MilliValue) when !is_percent */
} kp_eviction_value;

/* EC2NodeClass.spec.kubelet overrides (R:pkg/apis/v1/ec2nodeclass.go KubeletConfiguration). Resource maps carry
 * the keys the user set (present bits); eviction maps are nil unless has_* is set. */
typedef struct kp_kubelet {
  kp_resource_list kube_reserved;
  kp_resource_list system_reserved;
  int32_t has_eviction_hard;
  int32_t has_eviction_soft;
  kp_eviction_value hard_memory_available, hard_nodefs_available;
  kp_eviction_value soft_memory_available, soft_nodefs_available;
} kp_kubelet;

/* EC2NodeClass.spec.blockDeviceMappings entry (ABI v10): the fields ephemeralStorage reads
 * (R:pkg/providers/instancetype/types.go:349-385). */
typedef struct kp_block_device_mapping {
  const char* device_name;  /* deviceName; NULL: unset */
  int64_t volume_size;      /* ebs.volumeSize in bytes; < 0: nil */
  int32_t root_volume;      /* rootVolume */
  int32_t reserved_;
} kp_block_device_mapping;

/* EC2NodeClass.spec.instanceStorePolicy (ABI v10) */
#define KP_INSTANCE_STORE_NONE 0
#define KP_INSTANCE_STORE_RAID0 1

/* EC2NodeClass subset that changes results (AMI family, kubelet overrides, block devices). */
typedef struct kp_nodeclass {
  const char* region;
  const char* const* zones;      /* subnet zones (ZoneInfo) */
  const char* const* zone_ids;   /* parallel to zones; NULL entries allowed */
  uint32_t n_zones;
  int32_t max_pods;              /* < 0: nil */
  int32_t pods_per_core;         /* <= 0: nil */
  int32_t ami_family;            /* ABI v9: KP_AMI_* (EC2NodeClass.AMIFamily(); 0 = AL2023, the default alias) */
  const kp_kubelet* kubelet;     /* NULL: no kubelet block (defaults) */
  /* ABI v10: ephemeral-storage capacity (R:types.go:349-385): RAID0 -> the instance store's total size; else the
   * root-volume BDM's size, else (Custom) the last BDM's size or the 20Gi EBS default, else the BDM on the family's
   * ephemeral device; else the family's default ephemeral volume */
  const kp_block_device_mapping* block_device_mappings;
  uint32_t n_block_device_mappings;
  int32_t instance_store_policy; /* KP_INSTANCE_STORE_* */
} kp_nodeclass;

/* AMI families (R:pkg/providers/amifamily): their FeatureFlags (R:resolver.go:110-117, bottlerocket.go:126-132,
 * windows.go:101-108) and default ephemeral block device (al2023.go:98-108, al2.go:107-116, bottlerocket.go:95-112,
 * windows.go:88-99, custom.go:48-58) shape pods, kube-reserved memory, eviction and ephemeral storage. */
#define KP_AMI_AL2023 0
#define KP_AMI_AL2 1
#define KP_AMI_BOTTLEROCKET 2
#define KP_AMI_WINDOWS2019 3
#define KP_AMI_WINDOWS2022 4
#define KP_AMI_CUSTOM 5

/* instancetype.NewInstanceType capacity + Overhead.Total() (R:types.go:123-155, 313-598) for the nodeclass's AMI
 * family: Windows families add vpc.amazonaws.com/PrivateIPv4Address (IPv4 addresses per ENI - 1, types in the VPC
 * limits table, amd64 only: R:types.go:151-153, 477-484). The label half (computeRequirements, R:types.go:158-292)
 * is plain string marshalling and stays with the caller (kpamd/catalog.py mirrors it). */
int32_t kp_instance_type_resolve(const kp_options* opts, const kp_ec2_info* info, const kp_nodeclass* nc,
                                 kp_resource_list* capacity, kp_resource_list* overhead);

/* The three InstanceTypeOverhead lists NewInstanceType builds (R:types.go:145-149): kubeReservedResources
 * (R:types.go:500-533, overrides win), systemReservedResources (R:types.go:494-498) and evictionThreshold
 * (R:types.go:535-564: defaults, then the max over evictionHard and evictionSoft — soft honoured for AL2023's
 * EvictionSoftEnabled — of each signal, assigned over the defaults). kp_instance_type_resolve's overhead is
 * their sum (Overhead.Total()). */
int32_t kp_instance_type_overhead(const kp_options* opts, const kp_ec2_info* info, const kp_nodeclass* nc,
                                  kp_resource_list* kube_reserved, kp_resource_list* system_reserved,
                                  kp_resource_list* eviction_threshold);

/* ---- feasibility (CompatibleAvailableFilter, batched) ------------------------------------- */
typedef struct kp_feasibility_query {
  kp_requirements requirements;
  kp_resource_list requests;
} kp_feasibility_query;

/* For each query q: bit t of out_mask[q*words + t/64] <=> instance type t is compatible, fits and has
 * a compatible available offering (R:filter.go:51-64; AllowUndefinedWellKnownLabels). out_cheapest
 * (optional, n_queries × n_types) = cheapest compatible available offering price, +inf if none.
 * words = (n_types + 63) / 64. */
int32_t kp_filter_compatible_available(kp_ctx* ctx, const kp_catalog* cat, const kp_feasibility_query* queries,
                                       uint32_t n_queries, uint64_t* out_mask, double* out_cheapest,
                                       kp_solve_stats* stats);

/* Same split into prepare (compile + upload the rows, resident) and run (one launch; copy-out only into
 * non-NULL buffers) so many runs — or a benchmark — reuse resident inputs. stats (filter runs; computed by the
 * host): phase_cycles[0] the kernel the run launched: 1 feasibility_kernel (per type), 2 feasibility_bits_kernel,
 * 3 feasibility_quad_kernel with a copy wave (price rows), 4 feasibility_quad_kernel with every wave evaluating
 * (mask only, compact); 0 when there were no rows and nothing was launched. */
typedef struct kp_filter_plan kp_filter_plan;
int32_t kp_filter_prepare(kp_ctx* ctx, const kp_catalog* cat, const kp_feasibility_query* queries, uint32_t n_queries,
                          int32_t with_cheapest, kp_filter_plan** out);
int32_t kp_filter_run(kp_filter_plan* plan, uint64_t* out_mask, double* out_cheapest, kp_solve_stats* stats);
/* ABI v11, the compact result (prepare with with_cheapest = KP_FILTER_COMPACT): per query the mask and the set of
 * offering classes its requirements admit (out_classes[q], bit c = class c of kp_filter_class_prices), instead of n_types
 * prices. The cheapest compatible available offering price of type t for query q is then
 *   min over c in out_classes[q] of prices[c * n_types + t]   (+inf: none)
 * which equals kp_filter_run's out_cheapest bit for bit for every type, whether its mask bit is set or not (both are
 * the cheapest available offering among the query's compatible classes; the mask adds the type's requirements and Fits):
 * a class's price row is the cheapest available offering of the type in that class. kp_filter_class_prices copies the
 * plan's resident [C][n_types] table (C <= 64 classes) and its class count; the consumer reads it once per catalogue
 * seqnum, not per query, and a plan whose catalogue seqnum moved refuses it (KP_E_INVAL) until kp_filter_refresh. */
enum { KP_FILTER_MASK_ONLY = 0, KP_FILTER_CHEAPEST = 1, KP_FILTER_COMPACT = 2 };
int32_t kp_filter_run_compact(kp_filter_plan* plan, uint64_t* out_mask, uint64_t* out_classes, kp_solve_stats* stats);
int32_t kp_filter_class_prices(kp_filter_plan* plan, double* out, uint32_t capacity, uint32_t* n_classes);
void kp_filter_plan_destroy(kp_filter_plan* plan);
/* Re-apply the catalogue's current offerings to a prepared plan: only the offering section of the resident
 * catalogue (available-class masks, per-(type, class) prices; ~C*T*16 bytes) is rebuilt and copied to the
 * device, the rows stay resident. `cat` must be the catalogue the plan was prepared on (KP_E_INVAL otherwise). */
int32_t kp_filter_refresh(kp_filter_plan* plan, const kp_catalog* cat);

/* ---- launch-side selection (instance.DefaultProvider.Create) -------------------------------------
 * For each NodeClaim: filterInstanceTypes (R:pkg/providers/instance/instance.go:242-270) =
 *   CompatibleAvailableFilter (R:filter.go:39-64) -> CapacityReservationTypeFilter / CapacityBlockFilter /
 *   ReservedOfferingFilter (R:filter.go:66-274: they replace a type's offerings; offerings equal in every label form
 *   one class, so a replaced slice keeps whole classes) ->
 *   ExoticInstanceTypeFilter (R:filter.go:279-318) -> SpotInstanceFilter (R:filter.go:328-386), each filter that
 *   empties the set failing the launch with InsufficientCapacityError; then InstanceTypes.Truncate(reqs,
 *   max_types) = OrderByPrice + cut + SatisfiesMinValues (error -> CreateError "InstanceTypeFilteringFailed");
 * getCapacityType (R:instance.go:504-518): reserved, then spot, if the requirements allow it and some remaining
 *   type has an available compatible offering of it (in its replaced offering slice), else on-demand;
 * checkODFallback (R:instance.go:336-355): on-demand launch while flexible to spot with < 5 types (a warning);
 * getOverrides (R:instance.go:392-439): per remaining type (in truncated order) its available offerings compatible
 *   with the requirements narrowed to the chosen capacity type, in the type's offering order, whose zone has a
 *   subnet (subnet_zones stands for ZonalSubnetsForLaunch). Grouping the types and overrides into launch-template
 *   configs by AMI, max-pods, EFA count and reservation is kp_launch_templates (below); creating the EC2 launch
 *   template and hashing its name are AWS I/O, out of scope. */
typedef struct kp_launch_request {
  kp_requirements requirements;   /* NodeClaim.Spec.Requirements (minValues allowed) */
  kp_resource_list requests;      /* NodeClaim.Spec.Resources.Requests */
  const uint32_t* instance_types; /* the instance types Create receives: catalogue indices, any order */
  uint32_t n_instance_types;      /* <= 1024 on the device path */
  uint32_t reserved_;
} kp_launch_request;

enum kp_launch_status {
  KP_LAUNCH_OK = 0,
  KP_LAUNCH_INSUFFICIENT_CAPACITY = 1, /* a filter left no instance type (failed_filter says which) */
  KP_LAUNCH_MINVALUES = 2              /* Truncate: the cheapest max_types types do not satisfy minValues */
};
enum kp_launch_filter { KP_FILTER_COMPATIBLE_AVAILABLE = 0, KP_FILTER_EXOTIC = 4, KP_FILTER_SPOT = 5 };

typedef struct kp_launch_result {
  int32_t status;             /* enum kp_launch_status */
  int32_t capacity_type;      /* 0 on-demand, 1 spot, 2 reserved (KP_LAUNCH_OK only) */
  uint32_t n_types;           /* types written to out_types (after filters + Truncate) */
  uint32_t n_overrides;       /* overrides written to out_overrides */
  int32_t failed_filter;      /* enum kp_launch_filter when INSUFFICIENT_CAPACITY, else -1 */
  uint32_t n_compatible;      /* types kept by CompatibleAvailableFilter */
  uint32_t rejected_exotic;   /* types removed by ExoticInstanceTypeFilter */
  uint32_t rejected_spot;     /* types removed by SpotInstanceFilter */
  int32_t od_fallback_warning;/* checkODFallback would log its error */
  int32_t reservation_type;   /* capacity_type 2: getCapacityReservationType (R:instance.go:520-530), 0 default,
                                 1 capacity-block, -1 none; else -1 */
  uint32_t rejected_reservation; /* types removed by the three reservation filters */
  int32_t reserved_;
} kp_launch_result;

/* out_types: [n][max_types] catalogue indices in launch order; out_overrides: [n][max_types * n_subnet_zones]
 * entries (type_index << 8) | zone, zone = index into subnet_zones. max_types = 60 in the reference
  * (maxInstanceTypes, R:instance.go:60). */
int32_t kp_launch_select(kp_ctx* ctx, const kp_catalog* cat, const kp_launch_request* reqs, uint32_t n,
                         const char* const* subnet_zones, uint32_t n_subnet_zones, uint32_t max_types,
                         kp_launch_result* out, uint32_t* out_types, uint32_t* out_overrides, kp_solve_stats* stats);
typedef struct kp_launch_plan kp_launch_plan;
int32_t kp_launch_prepare(kp_ctx* ctx, const kp_catalog* cat, const kp_launch_request* reqs, uint32_t n,
                          const char* const* subnet_zones, uint32_t n_subnet_zones, uint32_t max_types,
                          kp_launch_plan** out);
int32_t kp_launch_run(kp_launch_plan* plan, kp_launch_result* out, uint32_t* out_types, uint32_t* out_overrides,
                      kp_solve_stats* stats);
/* ICE / price refresh of a prepared launch plan from its catalogue (see kp_filter_refresh). */
int32_t kp_launch_refresh(kp_launch_plan* plan, const kp_catalog* cat);
void kp_launch_plan_destroy(kp_launch_plan* plan);

/* ---- Solve -------------------------------------------------------------------------------- */
/* kp_solve = kp_solve_prepare + kp_solve_run + kp_solve_plan_destroy. prepare compiles the batch (string
 * dictionaries -> bitsets, catalogue SoA, NodeClaimTemplates, pod queue order) and uploads it; run
 * executes Solve on the resident inputs and may be repeated (state is restored on device each run). */
int32_t kp_solve(kp_ctx* ctx, const kp_solve_in* in, kp_solve_result** out);
/* Host-side compile of the batch only (no device, catalogues may come from kp_catalog_upload(NULL, ...)):
 * KP_OK when kp_solve would accept it, else the KP_E_UNSUPPORTED / KP_E_INVAL it would return. */
int32_t kp_solve_validate(const kp_solve_in* in);
int32_t kp_solve_prepare(kp_ctx* ctx, const kp_solve_in* in, kp_solve_plan** out);
/* kp_solve_prepare as a collective over a communicator (kp_comm_init; NULL = this process alone): the per-Solve
 * table of template options per (shape-level, NodePool template) — addToNewNodeClaim's Compatible + Add +
 * filterInstanceTypesByRequirements for a fresh NodeClaim, SURVEY §8e "feasibility precompute" — is computed in
 * shape-level row ranges, one per rank, and all-gathered (ncclAllGather over xGMI); solve_kernel then reads one
 * entry per template attempt instead of re-filtering the template's types. Every rank passes the same batch; each
 * can then run the Solve (replicas) or only the committing rank does. */
struct kp_comm;
int32_t kp_solve_prepare_comm(kp_ctx* ctx, const kp_solve_in* in, struct kp_comm* comm, kp_solve_plan** out);
int32_t kp_solve_run(kp_solve_plan* plan, kp_solve_result** out);
/* ABI v11: cancellation (upstream Solve observes ctx.Done() between pods; SURVEY §5 failure handling). A kp_cancel
 * is a flag in host-mapped memory that solve_kernel polls about every 1,024 Queue pops; kp_cancel_set is lock-free
 * and may be called from any thread while a call runs (the cgo shim calls it when ctx.Done() fires). A run that sees
 * it set stops placing pods and returns KP_E_CANCELED with no result; the plan stays usable (every run restores its
 * state). The token stays set until kp_cancel_reset. One token may serve many calls, one at a time. */
typedef struct kp_cancel kp_cancel;
int32_t kp_cancel_create(kp_ctx* ctx, kp_cancel** out);
int32_t kp_cancel_set(kp_cancel* c);
int32_t kp_cancel_reset(kp_cancel* c);
void kp_cancel_destroy(kp_cancel* c);
/* kp_solve_run / kp_solve with a cancellation token (NULL: not cancellable, as kp_solve_run). */
int32_t kp_solve_run_cancellable(kp_solve_plan* plan, kp_cancel* cancel, kp_solve_result** out);
int32_t kp_solve_cancellable(kp_ctx* ctx, const kp_solve_in* in, kp_cancel* cancel, kp_solve_result** out);
/* A prepared plan after kp_catalog_update_offerings (UnavailableOfferings.MarkUnavailable + SeqNum,
 * R:pkg/cache/unavailableofferings.go:66-92): re-applies the catalogues' current availability and prices to the
 * resident catalogue half (offering masks, class prices and subset minima, the NodeClaimTemplates' options) and the
 * plan's template-options table, in place. kp_solve_run refuses a plan whose catalogues changed until this ran.
 * KP_E_INVAL when the update changed which NodePools keep any instance type (prepare again). A new kp_solve on the
 * same catalogues does the same on its own (stats.catalog_refreshed). */
int32_t kp_solve_refresh(kp_solve_plan* plan);
void kp_solve_plan_destroy(kp_solve_plan* plan);
uint32_t kp_result_nodeclaim_count(const kp_solve_result* res);
/* out[p] for every input pod: >= 0 new NodeClaim index; -1 pod error; <= -2 existing node -(2+i) */
int32_t kp_result_pod_placements(const kp_solve_result* res, int32_t* out, uint32_t n_pods);
int32_t kp_result_nodeclaim(const kp_solve_result* res, uint32_t i, kp_nodeclaim_info* out);
int32_t kp_result_stats(const kp_solve_result* res, kp_solve_stats* out);
void kp_result_destroy(kp_solve_result* res);

/* ---- Why a pod is unschedulable (entry points added under ABI v13) ------------------------------
 * Upstream Scheduler.add returns, for a pod it cannot place, one error per NodeClaimTemplate ("incompatible with
 * nodepool ..."); the controller publishes them as the pod's FailedScheduling event. An explained Solve returns their
 * causes: for every pod it left unscheduled (placement -1), one kp_pool_reason per template, in the Solve's template
 * order (weight descending, name ascending; NodePools whose own requirements leave no instance type have no template
 * and no entry). An entry is what addToNewNodeClaim reports at the state the Solve ENDED in: the pod at its final
 * relaxation level, the remaining limits and topology counts as the Solve left them, a fresh NodeClaim. (The queue
 * stops only after a full cycle without a placement, so every failed pod's last attempt ran against that state; the
 * one exception is a topology group another pod's later relaxation made live, see DESIGN.) Errors from existing nodes
 * and in-flight NodeClaims are discarded, as upstream discards them.
 * Per template the first cause that holds is `code`, in the order of enum kp_why. The library returns no message
 * strings beyond the label keys: the shim builds the text.
 * Not covered (KP_E_UNSUPPORTED from the explained entry points): Solves over capacity reservations (a
 * ReservedOfferingError depends on reservation capacities that do not outlive the Solve). The cluster plans and the
 * general consolidation path have no explained form. */
enum kp_why {
  KP_WHY_NONE = 0,           /* the attempt would succeed at the final state (legal; see above) */
  KP_WHY_LIMITS = 1,         /* the NodePool has limits and filterByRemainingResources leaves no option */
  KP_WHY_TAINT = 2,          /* the final level's tolerations do not tolerate the template's taints */
  KP_WHY_REQUIREMENTS = 3,   /* Compatible(template requirements, pod requirements, allow undefined well-known) fails */
  KP_WHY_TOPOLOGY = 4,       /* Topology.AddRequirements, its Compatible with the merged requirements, or the pod-affinity
                                bootstrap rule of a fresh NodeClaim fails */
  KP_WHY_INSTANCE_TYPES = 5, /* filterInstanceTypesByRequirements: no option passes all three criteria */
  KP_WHY_MIN_VALUES = 6      /* n_remaining options pass them, but the set breaks a minValues requirement */
};
typedef struct kp_pool_reason {
  uint32_t nodepool;            /* index into kp_solve_in.nodepools */
  int32_t code;                 /* enum kp_why */
  int32_t taint;                /* KP_WHY_TAINT: index in the NodePool's taints of the first one not tolerated; else -1 */
  uint32_t n_types;             /* the template's options after the limits (filled from KP_WHY_TAINT on; 0 for LIMITS) */
  /* KP_WHY_INSTANCE_TYPES / KP_WHY_MIN_VALUES (0 otherwise): of those n_types options, how many pass each criterion of
   * filterInstanceTypesByRequirements on its own, against the merged requirements and daemon + pod requests:
   * Intersects(type, merged); Fits(total, allocatable); some available offering Compatible with merged. Upstream's
   * six booleans (requirementsMet, fits, hasOffering and their pairs) are these counts compared with 0. */
  uint32_t n_requirements, n_fits, n_offering;
  uint32_t n_requirements_fits, n_requirements_offering, n_fits_offering;
  uint32_t n_remaining;         /* options passing all three (> 0 exactly for KP_WHY_MIN_VALUES) */
  uint32_t n_keys;              /* KP_WHY_REQUIREMENTS: the label keys Compatible fails on ... */
  const char* const* keys;      /* ... in byte order; owned by the result */
} kp_pool_reason;
/* kp_solve_cancellable / kp_solve_run_cancellable (cancel may be NULL) with the explanation step behind the Solve, on
 * the same stream, before the copy-back: same placements, NodeClaims and stats. kp_solve / kp_solve_run never run it. */
int32_t kp_solve_explained(kp_ctx* ctx, const kp_solve_in* in, kp_cancel* cancel, kp_solve_result** out);
int32_t kp_solve_run_explained(kp_solve_plan* plan, kp_cancel* cancel, kp_solve_result** out);
/* 1: the result came from an explained entry point */
int32_t kp_result_explained(const kp_solve_result* res);
/* entries kp_result_pod_reasons has for `pod`: the template count for an unscheduled pod of an explained result, else 0
 * (a pod that lost its NodeClaim to Truncate's minValues check on the host was placed by the Solve and has none) */
uint32_t kp_result_reason_count(const kp_solve_result* res, uint32_t pod);
/* writes min(n, count) entries. KP_E_INVAL: pod out of range, or the result was not explained */
int32_t kp_result_pod_reasons(const kp_solve_result* res, uint32_t pod, kp_pool_reason* out, uint32_t n);

/* ---- Disruption: batched consolidation simulations ---------------------------------------------
 * Cluster snapshot as the disruption controller sees it (state.Cluster nodes + their reschedulable pods),
 * and a batch of candidate subsets. For each subset S, kp_simulate_batch computes what upstream
 * computeConsolidation(S...) decides (docs R:website/content/en/preview/concepts/disruption.md:89-128):
 * SimulateScheduling = Solve(pending pods + pods of the deleting nodes + pods of S, existing = every node that is
 * neither in S nor deleting) + TruncateInstanceTypes(100), with the NodePools' remaining limits; a pod of S placed
 * on an uninitialized node is an error (pods of deleting nodes are exempt); not all non-pending pods scheduled ->
 * no-op; 0 NodeClaims -> delete; > 1 -> no-op; 1 -> replace if some option's worst launch price is below the
 * summed candidate price (and, for multi-node, filterOutSameType keeps one). Spot-to-spot (feature gate, default
 * off) -> no-op. Subsets must not name deleting nodes. */
typedef struct kp_cluster_node {
  kp_existing_node node;      /* labels, taints, available (allocatable - bound pods), requests, initialized */
  uint32_t catalog;           /* catalogue of its instance type */
  uint32_t instance_type;     /* index of its instance type in that catalogue */
  const uint32_t* pods;       /* reschedulable pods on this node: indices into kp_cluster.pods */
  uint32_t n_pods;
  uint32_t deleting;          /* MarkedForDeletion: never a destination; its pods join every simulation */
} kp_cluster_node;

typedef struct kp_cluster {
  const kp_catalog* const* catalogs;      /* device path */
  const kp_catalog_desc* catalog_descs;   /* CPU oracle path */
  uint32_t n_catalogs;
  uint32_t n_nodepools;
  const kp_nodepool* nodepools;
  const kp_cluster_node* nodes;
  uint32_t n_nodes;
  uint32_t n_shapes;
  const kp_pod_shape* shapes;
  const kp_pod* pods;
  uint32_t n_pods;
  uint32_t spot_to_spot;      /* SpotToSpotConsolidation feature gate (default off; 1: spot candidates may be replaced
                                 by cheaper spot capacity, R:website/content/en/preview/concepts/disruption.md:110-128) */
  const uint32_t* pending_pods;  /* provisionable pods not bound to any node (indices into pods): they join every
                                    simulation, but their own scheduling errors do not block a decision */
  uint32_t n_pending;
  uint32_t n_namespaces;         /* ABI v8: the cluster's namespaces (pod affinity namespaceSelector) */
  const kp_namespace* namespaces;
  const char* const* pod_uids;   /* ABI v10: metadata.uid of every pod, or NULL (see kp_solve_in.pod_uids) */
} kp_cluster;

enum kp_decision { KP_DECISION_NOOP = 0, KP_DECISION_DELETE = 1, KP_DECISION_REPLACE = 2 };

typedef struct kp_sim_result {
  int32_t decision;           /* enum kp_decision */
  uint32_t replacement_nodepool;
  double candidate_price;     /* getCandidatePrices: sum of each candidate's cheapest label-compatible offering */
  double replacement_price;   /* REPLACE: min worst-launch price over the remaining replacement options */
  double savings;             /* DELETE: candidate_price; REPLACE: candidate_price - replacement_price; else 0 */
  uint32_t n_options;         /* REPLACE: replacement options left after the price filters */
  uint32_t n_pods;            /* pods rescheduled by the simulation */
} kp_sim_result;

/* subsets in CSR form: subset i = nodes[offsets[i] .. offsets[i+1]) (indices into cluster->nodes), in
 * candidate order. multi_node != 0 applies MultiNodeConsolidation's filterOutSameType to replacements. */
int32_t kp_simulate_batch(kp_ctx* ctx, const kp_cluster* cluster, const uint32_t* offsets, const uint32_t* nodes,
                          uint32_t n_subsets, int32_t multi_node, kp_sim_result* out, kp_solve_stats* stats);

/* Same, split so that one cluster snapshot serves many batches (the disruption loop re-probes one
 * snapshot: SingleNodeConsolidation, MultiNodeConsolidation's binary search, the sweep). prepare
 * compiles and uploads the snapshot and precomputes, per pod shape, the existing nodes it can ever use
 * and its NodeClaimTemplate outcome; simulate runs one batch of subsets on the resident snapshot.
 * NodePool limits, pending pods, deleting nodes, spot-to-spot and host ports run in the batched kernels; topology
 * spread, pod (anti-)affinity and a pod NotIn/DoesNotExist requirement on a label key some node lacks take the general
 * path (each subset a whole device Solve). Returns KP_E_UNSUPPORTED (the Go path then runs) for > 65535 pods in one
 * subset. Catalogues holding capacity reservations take the general path too (ABI v10): every simulation's Solve reserves
 * offerings strictly (SimulateScheduling's DisableReservedCapacityFallback); a candidate in a reservation is priced by
 * its reserved offering (on-demand / 1e7, R:pkg/providers/instancetype/offering/offering.go:160-166).
 * The general path compiles the cluster once as a superset Solve (every node not being deleted existing, every pod
 * a simulation can queue in its pod list) and runs the subsets' Solves batched, one workgroup each; a subset that
 * would remove every owner of an inverse anti-affinity term (and every subset of a cluster whose superset compile is
 * unsupported, or with kp_overrides.general_batch = 1) is compiled on its own. stats (general path): phase_cycles[0] simulations
 * batched, phase_cycles[1] simulations compiled per subset, phase_cycles[2] batched solve_kernel launches. stats
 * (batched sweep, ABI v13; computed by the host): phase_cycles[1] wave slots launched (each wave runs subsets slot,
 * slot + slots, ...), phase_cycles[2] the most subsets any wave ran, ceil(simulated / slots); a budgeted call counts the
 * admissible subsets only (both 0 when every subset is blocked). */
typedef struct kp_cluster_plan kp_cluster_plan;
int32_t kp_cluster_prepare(kp_ctx* ctx, const kp_cluster* cluster, kp_cluster_plan** out);
int32_t kp_cluster_simulate(kp_cluster_plan* plan, const uint32_t* offsets, const uint32_t* nodes, uint32_t n_subsets,
                            int32_t multi_node, kp_sim_result* out, kp_solve_stats* stats);
/* ABI v12: kp_cluster_simulate with a cancellation token (NULL: as kp_cluster_simulate). Upstream runs consolidation
 * under a timeout and counts the ones that expire (karpenter_voluntary_disruption_consolidation_timeouts_total,
 * R:website/content/en/preview/reference/metrics.md:186-187); the disruption shim sets the token when its context
 * expires. The batched kernel reads the flag between a wave's subsets, the general path before each launch and inside
 * each simulation's Solve (every ~1,024 pops): the call returns KP_E_CANCELED with no result within about one
 * simulation's time, and the plan stays usable. */
int32_t kp_cluster_simulate_cancellable(kp_cluster_plan* plan, kp_cancel* cancel, const uint32_t* offsets,
                                        const uint32_t* nodes, uint32_t n_subsets, int32_t multi_node, kp_sim_result* out,
                                        kp_solve_stats* stats);
/* kp_solve_refresh for a cluster snapshot: after kp_catalog_update_offerings the catalogues' availability and
 * prices, the templates' options and the candidates' prices are re-applied in place and the per shape-level template
 * outcomes recomputed; kp_cluster_simulate / kp_consolidate_argmin refuse the plan until then. */
int32_t kp_cluster_refresh(kp_cluster_plan* plan);
void kp_cluster_plan_destroy(kp_cluster_plan* plan);

/* ---- Multi-GPU consolidation: RCCL over xGMI -----------------------------------------------------------------
 * One rank per GPU (one process per GPU, or one thread per GPU/kp_ctx in a single process): rank 0 calls
 * kp_comm_unique_id and hands the 128 bytes to every rank out of band; each rank calls kp_comm_init on its own
 * kp_ctx (collective: it returns once all n_ranks joined). SURVEY §8e: the subsets of a sweep shard by contiguous
 * index range; the snapshot is replicated (each rank prepares its own kp_cluster_plan from the same kp_cluster). */
#define KP_COMM_ID_BYTES 128
typedef struct kp_comm kp_comm;
int32_t kp_comm_unique_id(uint8_t* id /* KP_COMM_ID_BYTES */);
int32_t kp_comm_init(kp_ctx* ctx, const uint8_t* id, int32_t n_ranks, int32_t rank, kp_comm** out);
/* Single-process multi-GPU (the Karpenter controller is one leader-elected process): one kp_ctx per GPU, created by
 * the caller, and one call that builds their n communicators at once (ncclCommInitAll; rank i = ctxs[i], distinct
 * GPUs). Each rank is then driven by its own OS thread (one goroutine per GPU, runtime.LockOSThread): every
 * collective entry point (kp_solve_prepare_comm, kp_consolidate_argmin) must be called by all n threads for the
 * same step. out: n communicators. No unique-id transport is needed. */
int32_t kp_comm_init_all(kp_ctx* const* ctxs, int32_t n, kp_comm** out);
/* A communicator whose exchange step is a caller-supplied host all-gather: fn(user, rank, send, recv, bytes) must
 * block until every rank contributed `bytes` and fill recv with n_ranks * bytes in rank order, returning 0 (non-zero:
 * the step fails with KP_E_DEVICE). For transports other than RCCL (a gRPC stream between controller replicas, Go
 * channels between goroutines, a test harness); the records exchanged are small (status words, 88-byte choices, and
 * the template-options table only when it is sharded). */
typedef int32_t (*kp_allgather_fn)(void* user, int32_t rank, const void* send, void* recv, size_t bytes);
int32_t kp_comm_init_host(kp_ctx* ctx, int32_t n_ranks, int32_t rank, kp_allgather_fn fn, void* user, kp_comm** out);
int32_t kp_comm_rank(const kp_comm* comm, int32_t* rank, int32_t* n_ranks);
void kp_comm_destroy(kp_comm* comm);
/* Collective steps never leave a peer waiting: a rank whose local part fails still takes part in the exchange with
 * a failure record (kp_choice.subset = KP_CHOICE_FAILED, counts[0] = its error code; a status word in
 * kp_solve_prepare_comm), and then every rank returns an error. */
#define KP_CHOICE_FAILED (-2)

typedef struct kp_choice {
  int64_t subset;         /* global subset index of the best decision; -1: every subset of every rank is a no-op */
  uint64_t counts[3];     /* no-op / delete / replace decisions over all ranks' subsets */
  uint64_t overflowed;    /* subsets whose pods overflowed the device queue (kp_consolidate_argmin then fails) */
  kp_sim_result result;   /* computeConsolidation(subset) (decision, prices, savings, ...) */
} kp_choice;

/* The consolidation sweep step of one rank: simulate this rank's subsets (global indices base_index + i), reduce them
 * on the device to the best non-no-op decision (max savings, ties to the lowest global subset index), then one
 * RCCL all-gather of the ranks' 80-byte records over xGMI; every rank returns the same choice. comm NULL: this GPU
 * alone (n_ranks = 1). out (optional, n_subsets entries): the per-subset results, as kp_cluster_simulate.
 * Replaces the multi-node sweep the reference runs serially on one CPU (disruption.md:89-128). */
int32_t kp_consolidate_argmin(kp_cluster_plan* plan, kp_comm* comm, const uint32_t* offsets, const uint32_t* nodes,
                              uint32_t n_subsets, uint64_t base_index, int32_t multi_node, kp_sim_result* out,
                              kp_choice* best, kp_solve_stats* stats);
/* ABI v12: the sweep step with a cancellation token (see kp_cluster_simulate_cancellable). A rank whose token fires
 * still takes part in the all-gather (a KP_CHOICE_FAILED record holding KP_E_CANCELED), so no peer waits; every rank
 * then returns an error. */
int32_t kp_consolidate_argmin_cancellable(kp_cluster_plan* plan, kp_comm* comm, kp_cancel* cancel,
                                          const uint32_t* offsets, const uint32_t* nodes, uint32_t n_subsets,
                                          uint64_t base_index, int32_t multi_node, kp_sim_result* out, kp_choice* best,
                                          kp_solve_stats* stats);
/* NodePool disruption budgets (spec.disruption.budgets; R:website/content/en/preview/concepts/disruption.md:274-333,
 * R:pkg/apis/crds/karpenter.sh_nodepools.yaml:95-135), additive to ABI v12. allowed[p] is the caller's allowed
 * disruptions of cluster->nodepools[p] for the reason it asks with (Underutilized for consolidation):
 *   max(0, min over the active budgets listing the reason or none of value(budget, total) - deleting - not_ready),
 * KP_BUDGET_UNLIMITED where no budget applies. A subset is admissible iff, for every NodePool, the number of its
 * members owned by that pool (the node's karpenter.sh/nodepool label) is <= allowed[pool]; this is upstream's candidate
 * walk generalised to arbitrary subsets, decided on the device where the subsets are (budget_gate_kernel, before the
 * simulations). A blocked subset is not simulated: its out entry is all zero (KP_DECISION_NOOP), it counts in
 * kp_choice.counts[0] and in *n_blocked, and it can never be the best. With a communicator *n_blocked is the calling
 * rank's own count only (the ranks' records carry no such field). allowed == NULL: exactly the cancellable call.
 * Errors: KP_E_INVAL when n_allowed differs from the cluster's NodePool count, or when a subset names a node whose
 * karpenter.sh/nodepool label is missing or names no NodePool of the cluster (the message names subset and node);
 * KP_E_UNSUPPORTED for more than 256 NodePools (the Go path then runs). Cancellation, stale-plan refusal and the
 * collective's "no peer is left waiting" rule hold as for the cancellable calls; a failure of the gate is a
 * KP_CHOICE_FAILED record. stats (general path): phase_cycles[0] + phase_cycles[1] count the admissible subsets only. */
#define KP_BUDGET_UNLIMITED 0xFFFFFFFFu
int32_t kp_cluster_simulate_budgeted(kp_cluster_plan* plan, kp_cancel* cancel, const uint32_t* offsets,
                                     const uint32_t* nodes, uint32_t n_subsets, int32_t multi_node,
                                     const uint32_t* allowed, uint32_t n_allowed, kp_sim_result* out, uint64_t* n_blocked,
                                     kp_solve_stats* stats);
int32_t kp_consolidate_argmin_budgeted(kp_cluster_plan* plan, kp_comm* comm, kp_cancel* cancel, const uint32_t* offsets,
                                       const uint32_t* nodes, uint32_t n_subsets, uint64_t base_index, int32_t multi_node,
                                       const uint32_t* allowed, uint32_t n_allowed, kp_sim_result* out, kp_choice* best,
                                       uint64_t* n_blocked, kp_solve_stats* stats);
/* Drift (R:website/content/en/preview/concepts/disruption.md:131-175; upstream disruption/drift.go), additive to ABI
 * v13. Each CSR subset (Drift passes singletons; larger subsets are legal) is one SimulateScheduling - the simulation
 * kp_cluster_simulate builds: the queue is the pending pods, the pods of the nodes being deleted and the subset's pods;
 * every node that is neither in the subset nor being deleted is an existing node; strict reservations, 100 instance
 * types, the NodePools' remaining limits - run as a whole device Solve: it does not stop at a second NodeClaim, and no
 * consolidation decision (price, same-type, spot-to-spot) is taken. out[s] is AllNonPendingPodsScheduled with the
 * uninitialized-node rule (drift_verdict_kernel on the device); *first is the lowest subset index that is admissible and
 * feasible (-1: none), and *replacements the Solve result of that subset, owned by the caller (kp_result_destroy) and
 * read with the kp_result_* accessors: kp_result_pod_placements is indexed by the simulation's input order (pending
 * pods, the deleting nodes' pods in node order, the subset's pods in subset order), a placement <= -2 names existing
 * node -2 - placement among the nodes neither in the subset nor being deleted, in cluster order. No NodeClaim: the
 * subset's nodes are simply deleted. *replacements is NULL when *first is -1.
 * allowed / n_allowed / *n_blocked: the budget rule of kp_cluster_simulate_budgeted (reason Drifted); allowed == NULL:
 * no budgets. A blocked subset is neither batched nor compiled: blocked = 1, feasible = 0, never *first. Errors,
 * stale-plan refusal and cancellation (the plan stays usable) are those of kp_cluster_simulate_budgeted. A plan
 * kp_cluster_prepare made for the batched simulation kernel builds its superset Solve on the first drift call and keeps
 * it; kp_cluster_simulate on that plan is unchanged. stats: as the general path reports (phase_cycles[0..2]:
 * simulations batched, simulations compiled per subset, launches). */
typedef struct kp_drift_result {
  int32_t feasible;          /* AllNonPendingPodsScheduled; 0 for a budget-blocked subset */
  uint32_t n_nodeclaims;     /* new NodeClaims of the simulation's Solve (the whole Solve: no early stop) */
  uint32_t n_pods;           /* pods queued */
  uint32_t n_unscheduled;    /* non-pending pods in error or on an uninitialized node */
  int32_t first_unscheduled; /* cluster pod index of the first such pod in queue order, -1: none */
  uint32_t blocked;          /* 1: not simulated (budget) */
} kp_drift_result;
int32_t kp_cluster_drift(kp_cluster_plan* plan, kp_cancel* cancel, const uint32_t* offsets, const uint32_t* nodes,
                         uint32_t n_subsets, const uint32_t* allowed, uint32_t n_allowed, kp_drift_result* out,
                         int64_t* first, kp_solve_result** replacements, uint64_t* n_blocked, kp_solve_stats* stats);
/* The consolidation command (upstream computeConsolidation's Command and its scheduling results: the replacement
 * NodeClaim the disruption controller launches, R:website/content/en/preview/concepts/disruption.md:89-128; upstream
 * disruption/consolidation.go computeConsolidation, filterByPrice, filterOutSameType and the spot-to-spot branch),
 * additive to ABI v13. Inputs, the budget rule and the errors are those of kp_cluster_simulate_budgeted, and out[s] is
 * exactly what that call writes for subset s. commands[s] (n_subsets entries) is the decision's command, owned by the
 * caller (kp_result_destroy) and read with the kp_result_* accessors:
 *   NOOP, or blocked by a budget: NULL.
 *   DELETE: a result with no NodeClaim and the placements.
 *   REPLACE: exactly one NodeClaim. options: the command's InstanceTypeOptions - of the NodeClaim's truncated,
 *     price-ordered options (cheapest compatible offering ascending, then name) those that survived filterByPrice and,
 *     with multi_node, filterOutSameType; for a single spot candidate under the spot-to-spot gate the first 15 of them
 *     (the first 100 when the requirements carry minValues); n_options equals out[s].n_options. n_remaining: the
 *     NodeClaim's options before truncation, as in a Solve. requirements: rendered as kp_solve_run renders them; when
 *     the decision was taken as spot-to-spot (every candidate spot, the replacement admits spot)
 *     karpenter.sh/capacity-type In [spot] replaces any other capacity-type requirement. requests, nodepool and pods
 *     (in add order) as in a Solve.
 *   Placements follow kp_cluster_drift's convention: indexed by the simulation's input order (pending pods, the
 *     deleting nodes' pods in node order, the subset's pods in subset order); >= 0 the NodeClaim, <= -2 existing node
 *     -2 - placement among the nodes neither in the subset nor being deleted, in cluster order, -1 unscheduled.
 * The command comes from the run that takes the decision: on a plan of the batched simulation kernel the emitting
 * sim_kernel instantiation writes one record per simulation (sized from the batch; a call whose records would pass
 * 4 GiB returns KP_E_UNSUPPORTED); on a general-path plan it is read from the simulation's arena of the batched launch,
 * or from the Solve of a subset compiled on its own (stats as kp_cluster_simulate reports them). The call is meant for
 * the few subsets a pass ends on (the firstN pick, the first single-node hit, the sweep's argmax). On any error every
 * commands[s] is NULL. */
int32_t kp_cluster_command(kp_cluster_plan* plan, kp_cancel* cancel, const uint32_t* offsets, const uint32_t* nodes,
                           uint32_t n_subsets, int32_t multi_node, const uint32_t* allowed, uint32_t n_allowed,
                           kp_sim_result* out, kp_solve_result** commands, uint64_t* n_blocked, kp_solve_stats* stats);
/* Command validation (upstream disruption/validation.go, v1.5.1: Validation.IsValid / ValidateCommand, the step
 * SingleNodeConsolidation and MultiNodeConsolidation run between computing a command and executing it), additive to ABI
 * v13. The upstream file is not among this project's references: the rule below is RESTATED here, only the 15 s
 * consolidation TTL is documented (R:website/content/en/v0.32/upgrading/v1beta1-migration.md:404), and parity beyond
 * the rule is unpinned. The plan is one prepared from CURRENT state; subset s holds the command's candidates and
 * checks[s] what the command decided. Let r be SimulateScheduling of the candidates on the plan - the simulation
 * kp_cluster_simulate builds (pending pods, the deleting nodes' pods and the candidates' pods queued; every other
 * non-deleting node existing; strict reservations; Truncate(100) with its minValues check; the NodePools' remaining
 * limits). In this order:
 *   1. some non-pending pod of r is unscheduled, or a candidate pod sits on an uninitialized node (a NodeClaim whose
 *      truncated options break minValues has lost its pods):                          KP_INVALID_UNSCHEDULED
 *   2. r makes no NodeClaim: a command without replacement is KP_VALID, one with a replacement
 *      KP_INVALID_NO_REPLACEMENT_NEEDED (upstream: "scheduling simulation produced new results")
 *   3. r makes more than one NodeClaim:                                                KP_INVALID_MULTIPLE
 *   4. r makes one NodeClaim and the command has no replacement:                       KP_INVALID_NEEDS_REPLACEMENT
 *   5. r makes one NodeClaim and the command has one: the command's options must be a subset, as a set of
 *      instance-type names, of the new NodeClaim's options - its whole price-ordered list after Truncate, NOT the ones
 *      a price filter would keep: KP_VALID, else KP_INVALID_NOT_SUBSET with n_missing the names that are absent.
 * Validation applies no price filter, no same-type filter and no spot-to-spot rule, so there is no multi_node input.
 * r stops at its second NodeClaim, as every consolidation simulation here does: the pods it had not reached are in no
 * state yet, so a simulation that needs more than one NodeClaim reports rule 3 (n_nodeclaims 2, n_unscheduled 0)
 * whether or not rule 1 would also have held of the finished Solve; both are invalid.
 * Names are a set (duplicates count once); a name the new NodeClaim's catalogue does not hold counts as missing.
 * A subset the budget rule of kp_cluster_simulate_budgeted blocks (the caller asks with the command's reason) is not
 * simulated: KP_INVALID_BUDGET, blocked = 1, every count 0; it counts in *n_blocked. allowed == NULL: no budgets.
 * Errors: KP_E_INVAL for a decision other than KP_DECISION_DELETE / KP_DECISION_REPLACE, a REPLACE without options and
 * a NULL name; otherwise those of kp_cluster_simulate_budgeted (a deleting node in a subset, the pool label,
 * n_allowed), with its stale-plan refusal (kp_catalog_update_offerings until kp_cluster_refresh), cancellation (the
 * plan stays usable) and stats words. On a plan of the batched simulation kernel the checking sim_kernel instantiation
 * writes the records; on a general-path plan validate_verdict_kernel writes them behind the batched launches'
 * solve_kernel and finalize_kernel (Truncate's minValues check on the device), and a subset compiled on its own takes
 * the rule on the host from that Solve's result (every subset does when the cluster has both capacity reservations and
 * minValues: the held reservation ids join the requirements before the minValues check, which only the host does).
 * NodePool limits on a batched-kernel plan: the kernel judges a second NodeClaim by the limits the pass began with,
 * while the first NodeClaim has taken its largest option out of them (subtractMax), so a subset it reports as MULTIPLE
 * is run once more as its own whole Solve and the record is that Solve's (UNSCHEDULED with one NodeClaim where the
 * limits admit no second); the caller pays one compile and Solve per such subset. stats: as kp_cluster_simulate reports
 * them on either kind of plan. */
enum kp_validity {
  KP_VALID = 0,
  KP_INVALID_UNSCHEDULED = 1,
  KP_INVALID_NO_REPLACEMENT_NEEDED = 2,
  KP_INVALID_MULTIPLE = 3,
  KP_INVALID_NEEDS_REPLACEMENT = 4,
  KP_INVALID_NOT_SUBSET = 5,
  KP_INVALID_BUDGET = 6
};
typedef struct kp_command_check {
  int32_t decision;             /* KP_DECISION_DELETE (no replacement) or KP_DECISION_REPLACE */
  const char* const* options;   /* REPLACE: the command's InstanceTypeOptions, by instance-type name */
  uint32_t n_options;
} kp_command_check;
typedef struct kp_validation {
  int32_t  verdict;         /* enum kp_validity */
  uint32_t n_nodeclaims;    /* 0, 1, or 2 = more than one */
  uint32_t n_pods;          /* pods queued */
  uint32_t n_unscheduled;   /* rule 1: non-pending pods unscheduled or on an uninitialized node */
  uint32_t n_missing;       /* NOT_SUBSET: command options absent from the new NodeClaim's options */
  uint32_t blocked;         /* 1: not simulated (budget) */
} kp_validation;
int32_t kp_cluster_validate(kp_cluster_plan* plan, kp_cancel* cancel, const uint32_t* offsets, const uint32_t* nodes,
                            uint32_t n_subsets, const kp_command_check* checks, const uint32_t* allowed,
                            uint32_t n_allowed, kp_validation* out, uint64_t* n_blocked, kp_solve_stats* stats);
/* Why a subset cannot be consolidated (upstream disruption/consolidation.go, v1.5.1: the exits of
 * computeConsolidation, each of which publishes an Unconsolidatable event), additive to ABI v13. The upstream file is
 * not among this project's references: the rule below is RESTATED here from what kp_cluster_simulate already decides,
 * only the events' two documented texts are pinned (R:website/content/en/preview/concepts/disruption.md:105-113, "pdb
 * default/inflate-pdb prevents pod evictions" - that one comes from kp_cluster_candidates - and "can't replace with a
 * lower-priced node"; :119-128 for the spot-to-spot rule and its 15 options), and parity beyond the rule is unpinned.
 * Inputs, the budget rule, the errors, the stale-plan refusal and cancellation are those of
 * kp_cluster_simulate_budgeted, and out[s] is bit for bit what that call writes. why[s] is the first line that holds
 * of subset s's simulation r, in the enum's order:
 *   NONE                 r decided DELETE or REPLACE
 *   BUDGET               the budget rule blocked the subset: not simulated, every count 0
 *   MULTIPLE_NODECLAIMS  r needs a second NodeClaim
 *   UNSCHEDULABLE        some non-pending pod of r is unscheduled, or a candidate pod sits on an uninitialized node, or
 *                        the one NodeClaim's truncated options break minValues (Truncate belongs to the Solve: its pods
 *                        fail) - decided before the candidates' prices and before the spot-to-spot gate are looked at
 *   UNPRICED             one NodeClaim, and some candidate has no label-compatible offering (getCandidatePrices fails)
 *   SPOT_TO_SPOT_DISABLED  every candidate is spot, the replacement may launch spot, and the feature gate is off
 *   NOT_CHEAPER          filterByPrice (worst launch price < the candidates' price) keeps nothing
 *   SAME_TYPE            multi_node: filterOutSameType keeps nothing
 *   SPOT_FLEXIBILITY     spot-to-spot with a single candidate and fewer than 15 options left
 *   MIN_VALUES           a NON-EMPTY filtered set breaks minValues; stage: 1 after filterByPrice, 2 after
 *                        filterOutSameType (an empty set is NOT_CHEAPER / SAME_TYPE, never MIN_VALUES)
 * One stated difference from upstream's message order: upstream checks "all pods scheduled" before it counts
 * NodeClaims. Every consolidation simulation here stops at its second NodeClaim - the pods it had not reached are in no
 * state yet - so MULTIPLE_NODECLAIMS comes first and carries no unscheduled count (n_nodeclaims 2, n_unscheduled 0,
 * first_unscheduled -1), the convention kp_cluster_validate documents for its rule 3.
 * Field rule: a field that belongs to a stage r did not reach is 0 (-1 for the two index fields); every field is
 * written for every simulation. The stages are the Solve (n_nodeclaims, n_unscheduled, first_unscheduled), Truncate
 * with minValues held on a fully scheduled r with one NodeClaim (n_truncated, cheapest_launch - whatever the prices and
 * the gate then say), filterByPrice (n_cheaper; not reached by UNPRICED and SPOT_TO_SPOT_DISABLED) and
 * filterOutSameType (n_same_type; reached when filterByPrice kept a set that holds minValues; without multi_node it
 * passes that set on). REPLACE under the spot-to-spot cut reports n_same_type before the cut, out[s].n_options after.
 * counts (may be NULL): the KP_UNCONS_COUNT-word histogram of why[0 .. n_subsets).reason. why may be NULL when counts
 * is not: the histogram alone comes back and, on a batched-kernel plan without limits, the records are never read
 * from the device (a 1M-subset sweep: 80 bytes instead of 48 MB).
 * On a plan of the batched simulation kernel a fifth sim_kernel instantiation writes out[] and why[] (48 bytes per
 * simulation) and why_count_kernel the histogram, so a sweep is explained without reading its records back. NodePool
 * limits on such a plan: the kernel judges a second NodeClaim by the limits the pass began with, while the first
 * NodeClaim has taken its largest option out of them (subtractMax); the difference between MULTIPLE_NODECLAIMS and
 * UNSCHEDULABLE is this call's answer, so when some NodePool has limits every record the kernel reports as
 * MULTIPLE_NODECLAIMS is settled by the subset's own whole Solve: the caller pays one compile and one Solve per such
 * subset, one after the other on the host (stats->phase_cycles[3] counts them): a sweep over a cluster with limits
 * whose subsets mostly need a second NodeClaim pays that for most of them, and is better asked for a sample. The record
 * stays the kernel's where that Solve would change out[s].
 * On a general-path plan the launches and per-subset Solves of kp_cluster_simulate run, and the decision code fills
 * the record on the host from each Solve's placements and options. */
enum kp_unconsolidatable {      /* first that holds, in this order */
  KP_UNCONS_NONE = 0,                 /* DELETE or REPLACE */
  KP_UNCONS_BUDGET = 1,               /* blocked by the budget rule: not simulated */
  KP_UNCONS_MULTIPLE_NODECLAIMS = 2,  /* the simulation needs a second NodeClaim */
  KP_UNCONS_UNSCHEDULABLE = 3,        /* a non-pending pod is unscheduled, a candidate pod sits on an uninitialized
                                         node, or the NodeClaim's truncated options break minValues (its pods fail) */
  KP_UNCONS_UNPRICED = 4,             /* one NodeClaim; some candidate has no label-compatible offering */
  KP_UNCONS_SPOT_TO_SPOT_DISABLED = 5,
  KP_UNCONS_NOT_CHEAPER = 6,          /* filterByPrice keeps nothing: "can't replace with a lower-priced node" */
  KP_UNCONS_SAME_TYPE = 7,            /* multi_node: filterOutSameType keeps nothing */
  KP_UNCONS_SPOT_FLEXIBILITY = 8,     /* single spot candidate, fewer than 15 options left */
  KP_UNCONS_MIN_VALUES = 9,           /* a non-empty filtered set breaks minValues; stage says after which filter */
  KP_UNCONS_COUNT = 10
};
typedef struct kp_sim_why {
  int32_t  reason;             /* enum kp_unconsolidatable */
  int32_t  stage;              /* MIN_VALUES: 1 after filterByPrice, 2 after filterOutSameType; else 0 */
  uint32_t n_nodeclaims;       /* 0, 1, or 2 = more than one */
  uint32_t n_unscheduled;      /* as kp_validation.n_unscheduled; 0 for MULTIPLE and BUDGET */
  int32_t  first_unscheduled;  /* cluster pod index of the first such pod in queue order (kp_drift_result's rule), -1 */
  int32_t  unpriced;           /* UNPRICED: position in the subset of the first unpriced candidate; else -1 */
  uint32_t n_truncated;        /* options of the one NodeClaim after Truncate (minValues held); 0 before that stage */
  uint32_t n_cheaper;          /* of those, worst launch price < candidate price */
  uint32_t n_same_type;        /* left after filterOutSameType (= n_cheaper when !multi_node) */
  uint32_t reserved_;
  double   cheapest_launch;    /* min worst launch price over the n_truncated options; 0 when n_truncated == 0 */
} kp_sim_why;
int32_t kp_cluster_simulate_explained(kp_cluster_plan* plan, kp_cancel* cancel, const uint32_t* offsets,
                                      const uint32_t* nodes, uint32_t n_subsets, int32_t multi_node,
                                      const uint32_t* allowed, uint32_t n_allowed, kp_sim_result* out, kp_sim_why* why,
                                      uint64_t* counts /* KP_UNCONS_COUNT words, may be NULL */, uint64_t* n_blocked,
                                      kp_solve_stats* stats);
/* Disruption candidates (upstream disruption.GetCandidates: NewCandidate per node, pdb.Limits, utils/disruption
 * ReschedulingCost / LifetimeRemaining / DisruptionCost, then the methods' sort), additive to ABI v13. Those upstream
 * files are not among this project's references: the rule is RESTATED here from
 * R:website/content/en/preview/concepts/disruption.md (:84-86 policy and consolidateAfter, :99-103 the ordering
 * preferences, :105-113 the Unconsolidatable events, :259-267 terminationGracePeriod, :335-396 PDBs and do-not-disrupt)
 * and parity beyond it is unpinned: the upstream pod-list order behind `detail`, the name tie-break, and whatever
 * NewCandidate checks beyond this text. Every input is per snapshot; the plan is one kp_cluster_prepare made of it.
 *
 * Eviction cost of a pod, exact in fixed point (units of 2^-27):
 *   fx = clamp(2^27 + deletion_cost + 4 * priority, -10 * 2^27, +10 * 2^27)
 * which is upstream's 1.0 + deletionCost / 2^27 + priority / 2^25 clamped to [-10, 10]; an absent annotation or a nil
 * priority is 0. ReschedulingCost(node) = the int64 sum of fx over the node's reschedulable pods (kp_cluster_node.pods):
 * every term is a multiple of 2^-27 and the sum stays far below 2^53, so its value as a double is exact and does not
 * depend on the order of summation. The device sums integers.
 *   LifetimeRemaining = 1.0 when expire_after_s < 0 (Never), 0.0 when expire_after_s == 0, else
 *                       clamp(double(expire_after_s - (now - created)) / double(expire_after_s), 0, 1)
 *   DisruptionCost    = (double(sum fx) * 2^-27) * LifetimeRemaining, in IEEE double (both are reported for every node)
 * Times are unix seconds; differences of two of them must fit int64.
 *
 * Reason of a node: the first line that applies; KP_CANDIDATE (0) makes it a candidate. detail is the reason's argument
 * (0 where it has none).
 *    1 KP_NOT_MANAGED             no karpenter.sh/nodepool label, or it names no NodePool of the cluster
 *    2 KP_NODE_DO_NOT_DISRUPT     KP_NODE_DO_NOT_DISRUPT set (the node's karpenter.sh/do-not-disrupt annotation)
 *    3 KP_NOT_INITIALIZED         kp_existing_node.initialized == 0
 *    4 KP_DELETING                kp_cluster_node.deleting
 *    5 KP_NOMINATED               KP_NODE_NOMINATED set (nominated for a pending pod)
 *    6 KP_POD_DO_NOT_DISRUPT      some pod of the node has KP_POD_DO_NOT_DISRUPT; detail = the cluster pod index of the
 *                                 first such pod in the node's `pods` order
 *    7 KP_PDB_BLOCKED             some pod has a PDB of its namespace whose selector matches its labels and whose
 *                                 disruptions_allowed == 0; detail = the PDB index: the lowest blocking PDB of the first
 *                                 blocked pod in `pods` order. Every pod is checked for 6 before any for 7.
 *    8 KP_CONSOLIDATION_DISABLED  Emptiness / SingleNode / MultiNode, and the pool's consolidate_after_s < 0 (Never)
 *    9 KP_POLICY_WHEN_EMPTY       SingleNode / MultiNode, and the pool's policy is KP_WHEN_EMPTY
 *   10 KP_NOT_CONSOLIDATABLE      Emptiness / SingleNode / MultiNode, and now - last_pod_event < consolidate_after_s
 *   11 KP_NOT_EMPTY               Emptiness, and the node has a reschedulable pod
 *   12 KP_NOT_DRIFTED             Drift, and KP_NODE_DRIFTED is not set
 * 6 and 7 are skipped for Drift on a node with KP_NODE_TERMINATION_GRACE_PERIOD (disruption.md:259). A nil selector
 * matches nothing, an empty one every pod of the PDB's namespace; a pod matching several PDBs is blocked if any blocks.
 *
 * Order: the candidates ascend by DisruptionCost compared as Go compares float64 (-0.0 and +0.0 tie; the cost is never
 * NaN), for Drift by drifted_unix instead; ties go by node name bytes, then node index (the project's convention).
 * order[0 .. *n_candidates) holds their node indices; out[i] is node i's record whatever its reason.
 *
 * Errors: KP_E_INVAL for a count that differs from the plan's snapshot (n_pools, n_nodes, n_pods), a NULL array whose
 * count is not 0, a NULL out / order / n_candidates, an unknown method or selector operator, a NULL selector key, and a
 * node of the snapshot listing a pod or a pod naming a shape out of range; the stale-plan refusal of
 * kp_cluster_simulate (kp_catalog_update_offerings until kp_cluster_refresh, a destroyed catalogue). KP_E_UNSUPPORTED
 * (the Go path then runs) for 65,535 or more NodePools (the node -> pool table is 16 bits wide), 2^28 or more distinct
 * labels and label keys over the shapes, and 2^31 or more selector terms; no cap on PDBs, nodes or pods beyond those of
 * kp_cluster_prepare. The call reads the snapshot's names, labels, namespaces and pod lists only: it works on plans of
 * both simulation paths, compiles them on its first use and keeps them resident, and leaves kp_cluster_simulate* and
 * every other call on the plan untouched. stats: device_ms (the kernels), host_ms (the call). */
enum kp_disruption_method {
  KP_METHOD_EMPTINESS = 0,
  KP_METHOD_SINGLE_NODE = 1,
  KP_METHOD_MULTI_NODE = 2,
  KP_METHOD_DRIFT = 3
};
enum kp_consolidation_policy { KP_WHEN_EMPTY_OR_UNDERUTILIZED = 0, KP_WHEN_EMPTY = 1 };
enum kp_candidate_reason {
  KP_CANDIDATE = 0,
  KP_NOT_MANAGED = 1,
  KP_NODE_DO_NOT_DISRUPT_REASON = 2,
  KP_NOT_INITIALIZED = 3,
  KP_DELETING = 4,
  KP_NOMINATED = 5,
  KP_POD_DO_NOT_DISRUPT_REASON = 6,
  KP_PDB_BLOCKED = 7,
  KP_CONSOLIDATION_DISABLED = 8,
  KP_POLICY_WHEN_EMPTY = 9,
  KP_NOT_CONSOLIDATABLE = 10,
  KP_NOT_EMPTY = 11,
  KP_NOT_DRIFTED = 12
};
typedef struct kp_pool_disruption {   /* NodePool spec.disruption, indexed like kp_cluster.nodepools */
  int32_t policy;                     /* enum kp_consolidation_policy */
  int32_t reserved_;
  int64_t consolidate_after_s;        /* < 0: Never */
} kp_pool_disruption;
#define KP_NODE_DO_NOT_DISRUPT 1u
#define KP_NODE_NOMINATED 2u
#define KP_NODE_TERMINATION_GRACE_PERIOD 4u
#define KP_NODE_DRIFTED 8u
typedef struct kp_node_disruption {   /* indexed like kp_cluster.nodes */
  uint32_t flags;                     /* KP_NODE_* */
  uint32_t reserved_;
  int64_t created_unix;               /* the NodeClaim's creationTimestamp */
  int64_t expire_after_s;             /* < 0: Never */
  int64_t last_pod_event_unix;        /* status.lastPodEventTime */
  int64_t drifted_unix;               /* transition time of the Drifted condition (read when KP_NODE_DRIFTED) */
} kp_node_disruption;
#define KP_POD_DO_NOT_DISRUPT 1u
typedef struct kp_pod_disruption {    /* indexed like kp_cluster.pods */
  int32_t priority;                   /* spec.priority; nil: 0 */
  int32_t deletion_cost;              /* controller.kubernetes.io/pod-deletion-cost; absent: 0 */
  uint32_t flags;                     /* KP_POD_* */
  uint32_t reserved_;
} kp_pod_disruption;
typedef struct kp_pdb {
  const char* namespace_;
  const char* name;                   /* for the caller's events; not read */
  kp_label_selector selector;
  int32_t disruptions_allowed;        /* status.disruptionsAllowed: 0 blocks every pod the PDB selects */
  int32_t reserved_;
} kp_pdb;
typedef struct kp_candidates_in {
  const kp_pool_disruption* pools;
  const kp_node_disruption* nodes;
  const kp_pod_disruption* pods;
  const kp_pdb* pdbs;
  uint32_t n_pools;                   /* == kp_cluster.n_nodepools */
  uint32_t n_nodes;                   /* == kp_cluster.n_nodes */
  uint32_t n_pods;                    /* == kp_cluster.n_pods */
  uint32_t n_pdbs;
  int64_t now_unix;
  int32_t method;                     /* enum kp_disruption_method */
  int32_t reserved_;
} kp_candidates_in;
typedef struct kp_candidate {
  int32_t reason;                     /* enum kp_candidate_reason */
  uint32_t detail;
  int64_t rescheduling_cost_fx;       /* sum of fx, units of 2^-27 */
  double disruption_cost;
} kp_candidate;
int32_t kp_cluster_candidates(kp_cluster_plan* plan, const kp_candidates_in* in, kp_candidate* out /* n_nodes */,
                              uint32_t* order /* n_nodes */, uint32_t* n_candidates, kp_solve_stats* stats);
/* Drift detection (R:pkg/cloudprovider/drift.go:43-157 CloudProvider.IsDrifted's EC2NodeClass half, R:pkg/providers/
 * amifamily/ami.go:222-235 MapToInstanceTypes, pinned by R:pkg/cloudprovider/suite_test.go:654-1190; the NodePool hash and
 * requirement drift of upstream core RESTATED from R:website/content/en/preview/concepts/disruption.md:131-164, parity
 * unpinned), additive to ABI v13. One call answers IsDrifted for every node of the plan's snapshot.
 * kp_cluster_drift is §10's simulation and is another call.
 *
 * Per node the first line that applies decides; reason is non-zero only when status is KP_DRIFT_OK.
 * Status, in this order:
 *   1 KP_DRIFT_SKIP_NOT_MANAGED        no karpenter.sh/nodepool label, or it names no NodePool of the cluster (upstream: ""
 *                                      and a nil error); the plan's node -> pool table
 *   2 KP_DRIFT_SKIP_NO_NODECLASS       the pool's kp_pool_drift.nodeclass is -1 (no nodeClassRef, or unresolved)
 *     reasons 1, 2 and 3 below are judged here: before any instance lookup and before any error
 *   3 KP_DRIFT_ERR_INSTANCE            KP_DRIFT_HAS_INSTANCE not set (no provider id, or no instance record)
 *   4 KP_DRIFT_ERR_INSTANCE_TYPE       the node's type is not in its pool's catalogue (looked up by name when the node's
 *                                      catalogue is another one)
 *   5 KP_DRIFT_ERR_NO_AMIS             the nodeclass's status.amis is empty
 *   6 KP_DRIFT_ERR_NO_SECURITY_GROUPS  its status.securityGroups is empty
 *   7 KP_DRIFT_ERR_NO_SUBNETS          its status.subnets is empty
 * An error ends the node with reason 0 even where an earlier dynamic check (4, 5) would have drifted: upstream returns
 * the error.
 * Reason, the first that applies:
 *   1 KP_DRIFT_NODEPOOL              the pool's and the NodeClaim's karpenter.sh/nodepool-hash and -hash-version are all
 *                                    present, the versions equal, the hashes different
 *   2 KP_DRIFT_REQUIREMENTS          NewLabelRequirements(node labels).Compatible(pool spec.template.spec.requirements)
 *                                    fails, undefined well-known labels not allowed (minValues and the template's labels
 *                                    play no part); detail = the index, in the pool's list, of the first requirement
 *                                    whose key fails
 *   3 KP_DRIFT_NODECLASS             areStaticFieldsDrifted: the EC2NodeClass's and the NodeClaim's ec2nodeclass-hash and
 *                                    -hash-version all present, versions equal, hashes different
 *   4 KP_DRIFT_AMI                   the type's AMI is the first of status.amis, in order, with
 *                                    type.Requirements.Compatible(ami requirements) (undefined keys not allowed); drifted
 *                                    iff there is none or its id differs from the instance's image id. detail = that
 *                                    AMI's index in status.amis, or 0xFFFFFFFF
 *   5 KP_DRIFT_SECURITY_GROUP        the set of status.securityGroups ids differs from the set of the instance's
 *   6 KP_DRIFT_SUBNET                the instance's subnet id is not among status.subnets
 *   7 KP_DRIFT_CAPACITY_RESERVATION  the instance has a reservation id that is not among status.capacityReservations
 * detail is 0 where the line gives it no meaning. The hash strings are inputs: computing them stays with the caller.
 *
 * counts[r] = the number of nodes with reason r (index 0: not drifted or not judged). out == NULL reads back the
 * histogram only; out and counts both NULL is refused.
 *
 * Errors: KP_E_INVAL for n_pools / n_nodes that differ from the plan's snapshot, a NULL array whose count is not 0, a
 * nodeclass index outside [-1, n_nodeclasses), an unknown requirement operator, a NULL requirement key or value, a NULL
 * AMI / subnet / security-group / reservation id in a list, an instance (KP_DRIFT_HAS_INSTANCE) with a NULL image or
 * subnet id; the stale-plan refusal of kp_cluster_candidates. KP_E_UNSUPPORTED (the Go path then runs) for 65,535 or
 * more NodePools, a NodePool whose requirements name more than 65,535 distinct keys, 2^28 or more distinct label keys, and a
 * catalogue type that some node runs carrying a NotIn / Exists / Gt / Lt requirement (the provider builds In and
 * DoesNotExist only, R:pkg/providers/instancetype/types.go:158-292); no cap on nodes, AMIs, ids or nodeclasses beyond 2^31
 * entries per array. Works on plans of both simulation paths, compiles the snapshot's half on its first use and keeps
 * it resident, and leaves every other call on the plan untouched. stats: device_ms (the kernels), host_ms (the call). */
enum kp_drift_status {
  KP_DRIFT_OK = 0,
  KP_DRIFT_SKIP_NOT_MANAGED = 1,
  KP_DRIFT_SKIP_NO_NODECLASS = 2,
  KP_DRIFT_ERR_INSTANCE = 3,
  KP_DRIFT_ERR_INSTANCE_TYPE = 4,
  KP_DRIFT_ERR_NO_AMIS = 5,
  KP_DRIFT_ERR_NO_SECURITY_GROUPS = 6,
  KP_DRIFT_ERR_NO_SUBNETS = 7
};
enum kp_drift_reason {
  KP_DRIFT_NONE = 0,
  KP_DRIFT_NODEPOOL = 1,
  KP_DRIFT_REQUIREMENTS = 2,
  KP_DRIFT_NODECLASS = 3,
  KP_DRIFT_AMI = 4,
  KP_DRIFT_SECURITY_GROUP = 5,
  KP_DRIFT_SUBNET = 6,
  KP_DRIFT_CAPACITY_RESERVATION = 7,
  KP_DRIFT_REASON_COUNT = 8
};
typedef struct kp_ami {               /* one entry of EC2NodeClass status.amis */
  const char* id;
  kp_requirements requirements;
} kp_ami;
typedef struct kp_nodeclass_status {  /* EC2NodeClass annotations + status, as drift reads them */
  const char* hash;                   /* karpenter.k8s.aws/ec2nodeclass-hash; NULL: absent */
  const char* hash_version;           /* ...-hash-version; NULL: absent */
  const kp_ami* amis;                 /* in status order */
  const char* const* subnets;         /* status.subnets[].id */
  const char* const* security_groups; /* status.securityGroups[].id */
  const char* const* capacity_reservations; /* status.capacityReservations[].id */
  uint32_t n_amis;
  uint32_t n_subnets;
  uint32_t n_security_groups;
  uint32_t n_capacity_reservations;
} kp_nodeclass_status;
typedef struct kp_pool_drift {        /* indexed like kp_cluster.nodepools */
  int32_t nodeclass;                  /* index into kp_drift_in.nodeclasses, or -1 */
  int32_t reserved_;
  const char* hash;                   /* the NodePool's karpenter.sh/nodepool-hash; NULL: absent */
  const char* hash_version;
} kp_pool_drift;
#define KP_DRIFT_HAS_INSTANCE 1u
typedef struct kp_node_drift_in {     /* indexed like kp_cluster.nodes: the NodeClaim's annotations and its instance */
  uint32_t flags;                     /* KP_DRIFT_HAS_INSTANCE: a provider id that resolves to an instance record */
  uint32_t n_security_groups;
  const char* nodepool_hash;          /* the NodeClaim's four annotations; NULL: absent */
  const char* nodepool_hash_version;
  const char* nodeclass_hash;
  const char* nodeclass_hash_version;
  const char* image_id;               /* the instance's; read when KP_DRIFT_HAS_INSTANCE */
  const char* subnet_id;
  const char* const* security_groups;
  const char* capacity_reservation_id; /* NULL: none */
} kp_node_drift_in;
typedef struct kp_drift_in {
  const kp_nodeclass_status* nodeclasses;
  const kp_pool_drift* pools;
  const kp_node_drift_in* nodes;
  uint32_t n_nodeclasses;
  uint32_t n_pools;                   /* == kp_cluster.n_nodepools */
  uint32_t n_nodes;                   /* == kp_cluster.n_nodes */
  uint32_t reserved_;
} kp_drift_in;
typedef struct kp_node_drift {
  int32_t reason;                     /* enum kp_drift_reason */
  int32_t status;                     /* enum kp_drift_status */
  uint32_t detail;
  uint32_t reserved_;
} kp_node_drift;
int32_t kp_cluster_detect_drift(kp_cluster_plan* plan, const kp_drift_in* in, kp_node_drift* out /* n_nodes */,
                                uint64_t* counts /* KP_DRIFT_REASON_COUNT words, may be NULL */,
                                kp_solve_stats* stats);

/* The scheduler's inputs (upstream NewScheduler's getDaemonOverhead, remainingResources, StateNode.Available() and the
 * ExistingNode's remaining daemonset requests), additive to ABI v13. One call computes, from cluster
 * state, the four inputs every Solve and cluster plan takes: kp_nodepool.daemon_requests, kp_nodepool.limits (the
 * remainder), kp_existing_node.available and kp_existing_node.requests. Upstream core (scheduler.go, existingnode.go,
 * statenode.go) is not among the references: the rule below is RESTATED and parity beyond it is unpinned. The pinned
 * piece is the per-template rule where a daemonset has at most one required term, no preferred term, and the template
 * no PreferNoSchedule taint: there it equals R:test/pkg/environment/common/expectations.go:1100-1140 ("the same logic
 * as the scheduler"; documented at R:website/content/en/preview/faq.md:105-108).
 *
 * Inputs. nodepools are kp_nodepool as a Solve takes them, except that limits holds spec.limits (not the remainder)
 * and daemon_requests is ignored. daemonsets are the DaemonSets' pod templates; of a kp_pod_shape only requests,
 * node_selector, required_terms, preferred_terms (ignored: strict requirements hold no preferences), tolerations and
 * volume_requirements are read. nodes carry labels, taints, allocatable and capacity; pod_offsets is the CSR of the
 * pods bound to each node, each pod an index into request_rows (the distinct request lists, `pods` included as
 * kp_pod_shape.requests has it) and KP_SCHED_POD_DAEMON when a DaemonSet owns it. The caller decides which nodes and
 * pods it lists (upstream: the active nodes; a node being deleted is not listed).
 *
 * strict(d, i) = d's node selector + its i-th required term + its volume requirements (NewStrictPodRequirements is
 * strict(d, 0); with no required term, the selector and the volume requirements alone).
 *
 * A template d is compatible with a NODE when every taint of the node is tolerated by some toleration of d
 * (Toleration.ToleratesTaint; PreferNoSchedule taints count), and NewLabelRequirements(node labels).Compatible(
 * strict(d, 0)) holds, undefined well-known labels NOT allowed: a key the node does not carry passes only under NotIn
 * or DoesNotExist.
 * A template d is compatible with a NodePool's TEMPLATE (upstream isDaemonPodCompatible) when every taint of the
 * NodePool other than PreferNoSchedule ones is tolerated by d, and for some i, tried in order (Preferences.Relax drops
 * the first required term on each failure), template.Requirements.Compatible(strict(d, i)) holds with undefined
 * well-known labels allowed. The template's requirements are NewNodeClaimTemplate's: the pool's requirements, its
 * labels, and karpenter.sh/nodepool In {name}.
 *
 * Per node:  available    = allocatable - sum of the requests of every bound pod, for the resources present in
 *                           allocatable (resources.Subtract keeps the left side's keys); may be negative
 *            requests     = for each resource present in some compatible template:
 *                           max(0, sum over compatible templates - sum over the bound pods with KP_SCHED_POD_DAEMON)
 *            n_compatible = the number of compatible templates; compat (optional) holds them as bits, template d at
 *                           bit d % 64 of word d / 64, max(1, ceil(n_daemonsets / 64)) words per node
 * Per pool:  daemon_requests = sum over the templates compatible with the pool's template (present: their union)
 *            remaining    = limits - sum of capacity over the nodes whose karpenter.sh/nodepool label names the pool
 *                           (the first pool of that name), for the resources present in limits; may be negative; a
 *                           pool without limits stays unlimited (present = 0); a node naming no pool counts nowhere
 *            n_compatible
 * A resource absent from a list counts 0. Sums are int64 milli-units and wrap on overflow.
 *
 * ctx == NULL validates the state on the host and writes nothing (kp_solve_validate's convention). Errors: KP_E_INVAL
 * for a NULL state or out, a NULL array whose count is not 0, NULL out->nodes / out->pools with n_nodes / n_nodepools
 * not 0, pod_offsets that do not start at 0, decrease, or end elsewhere than n_pods, a request row >= n_request_rows,
 * an unknown requirement / toleration operator, a NULL NodePool name, label key, taint key or requirement key or
 * value. KP_E_UNSUPPORTED for 65,535 or more NodePools and 2^31 or more request rows. stats: device_ms (the kernels),
 * host_ms (the call), prepare_ms (the host compile, part of host_ms). */
#define KP_SCHED_POD_DAEMON 1u
typedef struct kp_sched_pod {
  uint32_t requests;                  /* index into kp_sched_state.request_rows */
  uint32_t flags;                     /* KP_SCHED_POD_DAEMON */
} kp_sched_pod;
typedef struct kp_sched_node {
  const kp_label* labels;
  const kp_taint* taints;
  uint32_t n_labels;
  uint32_t n_taints;
  kp_resource_list allocatable;
  kp_resource_list capacity;
} kp_sched_node;
typedef struct kp_sched_state {
  const kp_nodepool* nodepools;
  const kp_pod_shape* daemonsets;
  const kp_sched_node* nodes;
  const uint32_t* pod_offsets;        /* n_nodes + 1 */
  const kp_sched_pod* pods;
  const kp_resource_list* request_rows;
  uint32_t n_nodepools;
  uint32_t n_daemonsets;
  uint32_t n_nodes;
  uint32_t n_pods;
  uint32_t n_request_rows;
  uint32_t reserved_;
} kp_sched_state;
typedef struct kp_sched_node_out {
  kp_resource_list available;         /* -> kp_existing_node.available */
  kp_resource_list requests;          /* -> kp_existing_node.requests */
  uint32_t n_compatible;
  uint32_t reserved_;
} kp_sched_node_out;
typedef struct kp_sched_pool_out {
  kp_resource_list daemon_requests;   /* -> kp_nodepool.daemon_requests */
  kp_resource_list remaining;         /* -> kp_nodepool.limits */
  uint32_t n_compatible;
  uint32_t reserved_;
} kp_sched_pool_out;
typedef struct kp_sched_out {         /* caller-allocated */
  kp_sched_node_out* nodes;           /* n_nodes */
  kp_sched_pool_out* pools;           /* n_nodepools */
  uint64_t* compat;                   /* n_nodes * max(1, ceil(n_daemonsets / 64)) words, or NULL */
} kp_sched_out;
int32_t kp_scheduler_inputs(kp_ctx* ctx, const kp_sched_state* state, kp_sched_out* out, kp_solve_stats* stats);

/* ---- catalogue compile (additive, ABI v13) ---------------------------------------------------------------------
 * kp_catalog_compile <- the resource half and the offering half of CloudProvider.GetInstanceTypes for EVERY
 * EC2NodeClass in one call (instancetype.DefaultProvider.List, R:pkg/providers/instancetype/instancetype.go:129-171:
 * NewInstanceType per (NodeClass, type), R:types.go:123-155; UpdateInstanceTypeCapacityFromNode's discovered memory,
 * R:instancetype.go:213-215,330-355; offering.InjectOfferings -> createOfferings, R:offering/offering.go:101-187).
 * The label half (computeRequirements) stays with the caller, as for kp_instance_type_resolve; the caller assembles
 * kp_instance_type lists for kp_catalog_upload from these tables.
 *
 * Inputs. types and nodeclasses are kp_ec2_info / kp_nodeclass as kp_instance_type_resolve takes them, opts likewise.
 * all_zones is the provider's allZones (at most 64, distinct); type_zones[t] has bit z set when type t is offered in
 * all_zones[z] (instanceTypesOfferings). od_price[t] and spot_price[t * n_all_zones + z] are what OnDemandPrice(type)
 * and SpotPrice(type, zone) return (R:pkg/providers/pricing/pricing.go:145-170: the caller resolves spot's default
 * price before spotPricingUpdated): NaN = no price (hasPrice false, price 0.0), else kp_offering.price's domain.
 * unavailable lists the UnavailableOfferings entries (R:pkg/cache/unavailableofferings.go:58-63); an entry names
 *   a (capacity type, type, zone) triple:  capacity_type and zone set, type >= 0
 *   a capacity type alone:                 capacity_type set, zone NULL, type < 0
 *   a zone alone:                          zone set, capacity_type NULL, type < 0
 * with capacity types "on-demand" and "spot". Capacity reservations are per NodeClass: reservation_offsets
 * (n_nodeclasses + 1 entries) is the CSR of nodeclass -> reservations. reserved_capacity is the ReservedCapacity
 * feature gate: with it 0, or with no reservation listed, there are no reserved offerings (the list is still
 * validated, out->reserved is not written). discovered_memory[n * n_types + t] (may be NULL) is the memory capacity in
 * bytes a real node of that pair reported; negative: none.
 *
 * Outputs, pair index i = n * n_types + t. Each array may be NULL to skip it; all NULL is KP_E_INVAL.
 *   capacity[i], overhead[i]  exactly kp_instance_type_resolve(opts, &types[t], &nodeclasses[n]), present masks
 *                             included, except that a discovered memory replaces capacity.milli[KP_RES_MEMORY] alone
 *                             (bytes * 1000); the overhead is still computed from memory()
 *   kube_reserved[i], system_reserved[i], eviction_threshold[i]  exactly kp_instance_type_overhead's lists
 *   it_zones[i]   type_zones[t] AND {z : all_zones[z] is a subnet zone of nodeclass n}: the values of the type's zone
 *                 requirement. A subnet zone that is not in all_zones takes no part.
 *   price[(t * n_all_zones + z) * 2 + c]   capacity type c: 0 on-demand, 1 spot (KP_CT_*); 0.0 without a price.
 *                 It does not depend on the NodeClass.
 *   available[i * 2 + c]   bit z = !IsUnavailable(type, zone, capacity type) AND hasPrice AND z in it_zones
 *                 (R:offering.go:121-141). An offering in a zone outside the NodeClass's subnets exists (createOfferings
 *                 iterates allZones), is never available and carries no zone id.
 *   reserved[r]   one record per input reservation, in input order: price = od / 10,000,000.0 (0.0 without an
 *                 on-demand price), available = count != 0 AND zone in it_zones of its (NodeClass, type),
 *                 capacity = the count (R:offering.go:155-185)
 *
 * ctx == NULL validates on the host and writes nothing. Errors: KP_E_INVAL for a NULL in / out, all outputs NULL, a
 * NULL array whose count is not 0 (types, nodeclasses, all_zones, type_zones, od_price, spot_price, unavailable,
 * reservations with reservation_offsets; a nodeclass's zones or block_device_mappings), a NULL or repeated zone name,
 * a type_zones bit at or past n_all_zones, a negative price, a discovered memory above INT64_MAX / 1000 bytes, an
 * unavailable entry of none of the three forms or naming an unknown capacity type, a zone not in all_zones or a type out of range, reservation_offsets that do not start at
 * 0, decrease, or end elsewhere than n_reservations, a reservation with a NULL id, a type out of range or a zone not
 * in all_zones. KP_E_UNSUPPORTED for more than 64 zones and for n_nodeclasses * n_types or n_types * n_all_zones * 2
 * of 2^31 or more (checked before any array is read). stats: device_ms (the kernels), host_ms (the call), prepare_ms
 * (the host compile, part of host_ms). */
#define KP_CT_ON_DEMAND 0
#define KP_CT_SPOT 1
typedef struct kp_unavailable {
  const char* capacity_type;          /* "on-demand" | "spot"; NULL: the entry names a zone alone */
  const char* zone;                   /* NULL: the entry names a capacity type alone */
  int32_t type;                       /* index into types; < 0: none */
  int32_t reserved_;
} kp_unavailable;
typedef struct kp_compile_reservation { /* EC2NodeClass.status.capacityReservations entry + its available count */
  const char* id;
  const char* zone;                   /* availabilityZone */
  const char* reservation_type;       /* "default" | "capacity-block": not read, it belongs to the label half */
  uint32_t type;                      /* index into types (the reservation's instanceType) */
  int32_t available_count;            /* capacityReservationProvider.GetAvailableInstanceCount(id) */
} kp_compile_reservation;
typedef struct kp_reserved_offering {
  double price;
  int32_t available;
  int32_t capacity;                   /* -> kp_offering.reservation_capacity */
} kp_reserved_offering;
typedef struct kp_compile_in {
  kp_options opts;
  const kp_ec2_info* types;
  const kp_nodeclass* nodeclasses;
  const char* const* all_zones;
  const uint64_t* type_zones;         /* n_types */
  const double* od_price;             /* n_types */
  const double* spot_price;           /* n_types * n_all_zones */
  const kp_unavailable* unavailable;
  const uint32_t* reservation_offsets; /* n_nodeclasses + 1, or NULL with n_reservations 0 */
  const kp_compile_reservation* reservations;
  const int64_t* discovered_memory;   /* n_nodeclasses * n_types, or NULL */
  uint32_t n_types;
  uint32_t n_nodeclasses;
  uint32_t n_all_zones;
  uint32_t n_unavailable;
  uint32_t n_reservations;
  int32_t reserved_capacity;          /* the ReservedCapacity feature gate */
} kp_compile_in;
typedef struct kp_compile_out {       /* caller-allocated; any may be NULL */
  kp_resource_list* capacity;         /* n_nodeclasses * n_types */
  kp_resource_list* overhead;
  kp_resource_list* kube_reserved;
  kp_resource_list* system_reserved;
  kp_resource_list* eviction_threshold;
  uint64_t* it_zones;                 /* n_nodeclasses * n_types */
  double* price;                      /* n_types * n_all_zones * 2 */
  uint64_t* available;                /* n_nodeclasses * n_types * 2 */
  kp_reserved_offering* reserved;     /* n_reservations */
} kp_compile_out;
int32_t kp_catalog_compile(kp_ctx* ctx, const kp_compile_in* in, const kp_compile_out* out, kp_solve_stats* stats);

/* ---- launch-template configs (the CreateFleet LaunchTemplateConfigs of a burst of NodeClaims) ----------------
 * kp_launch_templates = kp_launch_select followed, on the device, by the grouping that decides which launch templates
 * a NodeClaim needs and which overrides each carries: amifamily.MapToInstanceTypes (R:pkg/providers/amifamily/
 * ami.go:222-235), DefaultResolver.Resolve's grouping (R:pkg/providers/amifamily/resolver.go:126-188, 265-302) and
 * getLaunchTemplateConfigs / getOverrides (R:pkg/providers/instance/instance.go:356-439). `amis` is the
 * EC2NodeClass's status.amis in status order; one call covers one catalogue, that is one NodeClass.
 *
 * The rule, per request whose launch status is KP_LAUNCH_OK:
 *  1. For each selected type, in truncated launch order, ami(t) is the first AMI in list order for which
 *     type.Requirements.Compatible(NewNodeSelectorRequirements(ami.requirements...)) holds, with no well-known-label
 *     allowance (kp_cluster_detect_drift's AMI judgement). A type no AMI takes belongs to no template (n_unmapped).
 *  2. The group key is (ami(t), maxPods, efaCount, reservation part): maxPods = Capacity.Pods().Value(); efaCount =
 *     Capacity[vpc.amazonaws.com/efa].Value() when the request's resource list carries that key (a present zero
 *     counts: Go tests the key), else 0; the reservation part is empty unless the chosen capacity type is reserved.
 *  3. Not reserved: one config per group. Its types are the group's members in launch order; its overrides are, for
 *     each member in that order, the type's available offerings compatible with the requirements narrowed to the
 *     capacity type, in the type's offering order, whose zone has a subnet: the type's entries of kp_launch_run's list.
 *  4. Reserved: the reservation part is the reserved offerings of the type's offering slice as the launch filters left
 *     it (one per zone after ReservedOfferingFilter), so every type is a group of its own (reservation ids are not
 *     shared across instance types, the invariant resolver.go:174-176 relies on), and there is one config per (type,
 *     reservation) in the type's offering order. Its overrides are only that reservation's offering: available,
 *     compatible, zone with a subnet. reservation_type is that of the slice's reserved offerings.
 *  5. A config without overrides is dropped (n_dropped). If none is left the status is KP_LT_NO_OFFERINGS, Go's "no
 *     capacity offerings are currently available given the constraints".
 *  6. Config order. Go iterates two maps here, so upstream's order is random and CreateFleet does not depend on it.
 *     The order written here is canonical, not upstream's: by the launch-order position of a config's first type,
 *     then by reservation in the type's offering order.
 * The launch template's name (a hash of its options), user data, block-device and metadata defaults and
 * ensureLaunchTemplate are AWS I/O and stay with the caller, which keys its template cache by the config record.
 *
 * Outputs, per request i (stride = max_types * max(1, n_subnet_zones), the override stride of kp_launch_run; it bounds
 * the config count, every config that is kept having at least one override):
 *   out, out_types                   exactly what kp_launch_run writes, bit for bit
 *   lt_out[i]                        status, configs kept, selected types no AMI took, configs dropped
 *   out_type_config[i][max_types]    per selected type (launch order) its first config, or -1 (unmapped, or every
 *                                    config of it dropped); -1 past n_types
 *   out_configs[i][stride]           n_configs records in canonical order
 *   out_overrides[i][stride]         (type_index << 8) | zone as kp_launch_run; each config's entries are contiguous
 *                                    [first_override, + n_overrides) and in getOverrides order. Not the list
 *                                    kp_launch_run writes: that one is flat, in launch order
 * A config's types: reservation_offering < 0: the selected types whose out_type_config is the config, in launch
 * order; else the one type of its override. Entries past the counts are unspecified. Any output may be NULL.
 *
 * Errors: KP_E_INVAL for a NULL array whose count is not 0, an AMI with a NULL id, NULL requirement items, keys, value
 * arrays or values, an operator outside kp_operator; those of kp_launch_select / kp_launch_run, the stale-plan refusal
 * after kp_catalog_update_offerings until kp_launch_refresh among them. KP_E_UNSUPPORTED (the Go path then runs) for
 * more than 65,535 AMIs (decided from the count before any array is read) and, for an instance type some
 * request lists with a NotIn / Exists / Gt / Lt requirement, a pods capacity outside [0, 2^31) or an EFA capacity
 * outside [0, 65535]. kp_launch_templates_validate checks `amis` alone, on the host, without a context. stats as
 * kp_launch_run, device_ms covering launch_kernel and the two template kernels; prepare_ms is this call's host compile of the AMIs. */
enum kp_lt_status {
  KP_LT_OK = 0,
  KP_LT_SKIPPED = 1,           /* the launch status is not KP_LAUNCH_OK: the launch result passes through, no configs */
  KP_LT_NO_AMIS = 2,           /* n_amis == 0: "no amis exist given constraints" */
  KP_LT_NO_COMPATIBLE_AMI = 3, /* no selected type maps to an AMI: "no instance types satisfy requirements of amis" */
  KP_LT_NO_OFFERINGS = 4       /* every config was dropped */
};
typedef struct kp_lt_result {
  int32_t status;              /* enum kp_lt_status */
  uint32_t n_configs;
  uint32_t n_unmapped;         /* selected types no AMI took */
  uint32_t n_dropped;          /* configs dropped for having no override */
} kp_lt_result;
typedef struct kp_lt_config {
  int32_t ami;                 /* index into amis */
  int32_t max_pods;
  int32_t efa_count;
  int32_t reservation_offering;/* reserved launch: index of the reservation's offering in the type's
                                  kp_instance_type.offerings (its reservation_id names the launch template's
                                  CapacityReservationID); else -1 */
  int32_t reservation_type;    /* reserved launch: 0 default, 1 capacity-block, -1 none; else -1 */
  uint32_t first_override;     /* into out_overrides[i] */
  uint32_t n_overrides;        /* > 0 */
  uint32_t n_types;            /* > 0; 1 on a reserved launch */
} kp_lt_config;
int32_t kp_launch_templates_validate(const kp_ami* amis, uint32_t n_amis);
int32_t kp_launch_run_templates(kp_launch_plan* plan, const kp_ami* amis, uint32_t n_amis, kp_launch_result* out,
                                uint32_t* out_types, kp_lt_result* lt_out, int32_t* out_type_config,
                                kp_lt_config* out_configs, uint32_t* out_overrides, kp_solve_stats* stats);
int32_t kp_launch_templates(kp_ctx* ctx, const kp_catalog* cat, const kp_launch_request* reqs, uint32_t n,
                            const char* const* subnet_zones, uint32_t n_subnet_zones, uint32_t max_types,
                            const kp_ami* amis, uint32_t n_amis, kp_launch_result* out, uint32_t* out_types,
                            kp_lt_result* lt_out, int32_t* out_type_config, kp_lt_config* out_configs,
                            uint32_t* out_overrides, kp_solve_stats* stats);

/* ---- interruption messages (which NodeClaims a batch of queue messages deletes, which spot offerings it marks) ----
 * kp_cluster_interruptions resolves a whole batch of parsed interruption-queue messages against a prepared cluster
 * plan's snapshot in one call: the interruption controller's handleMessage / handleNodeClaim / deleteNodeClaim
 * (R:pkg/controllers/interruption/controller.go:160-248) for every message at once, where upstream does one List per
 * instance id. Receiving, parsing and deleting the SQS messages, events, latency metrics and the API delete stay with
 * the caller.
 *
 * Messages. A message is a kind (enum kp_message_kind) and a list of EC2 instance ids; only scheduled_change carries
 * several. Kinds 2-5 act (actionForMessage, :272-279: CordonAndDrain), kind 1 only notifies, kind 0 is ignored before
 * its ids are read (:164-166): its entries match nothing.
 *
 * Match. A (message, id) entry matches every node of the snapshot whose instance id (node_ids[n], the last path
 * segment of the provider id, R:pkg/utils/utils.go:36-52) equals the id byte for byte. Several NodeClaims may share
 * one id (handleMessage loops over Items); a node whose node_ids entry is NULL matches nothing.
 *
 * Per node, over its matching entries of kinds 1-5:
 *   kinds          the OR of 1 << kind
 *   n_messages     the number of entries: a message that names the id twice counts twice
 *   first_message  the lowest message index among the matches of kinds 2-5, or -1. Upstream handles ten messages at a
 *                  time, so which message deletes a NodeClaim hit by several is random there; the lowest index is the
 *                  canonical choice.
 *   flags          KP_INTERRUPT_DELETE            first_message >= 0 and kp_cluster_node.deleting == 0
 *                  KP_INTERRUPT_ALREADY_DELETING  first_message >= 0 and the node is deleting: deleteNodeClaim returns
 *                                                 early (:234-236), nothing is deleted or counted
 *                  KP_INTERRUPT_ICE               the node carries an ICE mark, see below
 *
 * ICE marks (:218-225). A spot_interrupted match on a node whose labels node.kubernetes.io/instance-type and
 * topology.kubernetes.io/zone are both present and non-empty marks (type label, zone label) unavailable for capacity
 * type spot, whatever the node's own capacity type and whether or not it is deleting. Such a node carries the mark.
 * Marks are de-duplicated by the two label strings (type names repeat across catalogues, and the reference's cache is
 * keyed by name). A mark is returned as the lowest node index that carries it and the number of nodes that carry it;
 * the caller reads the two labels from that node.
 *
 * Outputs (each of out_nodes, out_matches, deletes, marks, counts may be NULL to skip it):
 *   out_nodes[n_nodes]    the per-node record above
 *   out_matches[n_ids]    per (message, id) entry how many nodes it matched; 0: the id named no NodeClaim
 *   deletes[<= n_nodes]   one record per node with KP_INTERRUPT_DELETE, in node order: the node, its first_message and
 *                         that message's kind. *n_deletes receives the count
 *   marks[<= n_nodes]     one record per distinct mark, in order of `node`. *n_marks receives the count
 *   counts[6]             deletes per kind of first_message (NodeClaimsDisruptedTotal's reason)
 *   stats                 device_ms (the kernels), host_ms (the call)
 * Two calls with equal inputs on one plan write identical bytes.
 *
 * Inputs. kinds[n_messages]; the CSR id_offsets[n_messages + 1] over ids[n_ids] (id_offsets may be NULL when
 * n_messages is 0); node_ids[n_nodes]. table_log2 0 lets the library size the join's hash table; any other value
 * forces 1 << table_log2 slots, which must exceed the number of nodes that have an id (tests force long probe runs).
 *
 * Errors. KP_E_UNSUPPORTED for 2^31 or more messages or ids (decided from the counts before any array is read) and for
 * an id longer than 31 bytes (EC2's are 19). KP_E_INVAL for a NULL argument, a NULL array whose count is not 0, a NULL
 * message id, a kind outside 0-5, offsets that do not start at 0, decrease, or end elsewhere than n_ids, table_log2
 * above 30 or a forced table that is too small; kp_interruptions_validate checks all of these on the host without a
 * context. With a plan also: n_nodes different from the snapshot's node count, NULL n_deletes or n_marks, and the
 * stale-plan refusal of kp_cluster_candidates. */
enum kp_message_kind {
  KP_MSG_NO_OP = 0,
  KP_MSG_REBALANCE_RECOMMENDATION = 1,
  KP_MSG_SCHEDULED_CHANGE = 2,
  KP_MSG_SPOT_INTERRUPTED = 3,
  KP_MSG_INSTANCE_STOPPED = 4,
  KP_MSG_INSTANCE_TERMINATED = 5
};
#define KP_MESSAGE_KIND_COUNT 6
#define KP_INTERRUPT_DELETE 1u
#define KP_INTERRUPT_ALREADY_DELETING 2u
#define KP_INTERRUPT_ICE 4u
typedef struct kp_interrupt_node {
  int32_t first_message;
  uint32_t kinds;
  uint32_t n_messages;
  uint32_t flags;                     /* KP_INTERRUPT_* */
} kp_interrupt_node;
typedef struct kp_interrupt_delete {
  uint32_t node;
  uint32_t message;                   /* the node's first_message */
  int32_t kind;                       /* enum kp_message_kind of that message */
  uint32_t reserved;
} kp_interrupt_delete;
typedef struct kp_interrupt_mark {
  uint32_t node;                      /* the lowest node that carries the mark */
  uint32_t n_nodes;                   /* nodes that carry it */
} kp_interrupt_mark;
typedef struct kp_interrupt_in {
  const int32_t* kinds;               /* n_messages, enum kp_message_kind */
  const uint32_t* id_offsets;         /* n_messages + 1 */
  const char* const* ids;             /* n_ids */
  const char* const* node_ids;        /* n_nodes; NULL entry: the node has no provider id */
  uint32_t n_messages;
  uint32_t n_ids;
  uint32_t n_nodes;
  uint32_t table_log2;
} kp_interrupt_in;
int32_t kp_interruptions_validate(const kp_interrupt_in* in);
int32_t kp_cluster_interruptions(kp_cluster_plan* plan, const kp_interrupt_in* in, kp_interrupt_node* out_nodes,
                                 uint32_t* out_matches, kp_interrupt_delete* deletes, uint32_t* n_deletes,
                                 kp_interrupt_mark* marks, uint32_t* n_marks, uint64_t* counts, kp_solve_stats* stats);

/* The reduction kp_consolidate_argmin applies to the gathered per-rank records (host-only; exposed for callers that
 * reduce over another transport, and for tests): counts are summed, the best record wins. */
int32_t kp_choice_reduce(const kp_choice* per_rank, uint32_t n, kp_choice* out);

#ifdef __cplusplus
}
#endif
#endif /* KP_ABI_H */
