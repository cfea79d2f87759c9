// kp_schedin.h — device data model of kp_scheduler_inputs (kp_schedin.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kp/kp_abi.h"

#define SI_NONE 0xFFFFFFFFu

// Strings never reach the device. A label key some daemonset template names is a row of node_val (key-major, as
// kp_driftdet.h's), a node's value under it an id of the key's dictionary. A template's strict requirement on a key
// is one bitset over that dictionary (Gt / Lt evaluated on the host against each distinct value) plus
// SI_ABSENT_PASSES: its operator is NotIn or DoesNotExist, which alone passes a node without the label. A node's
// taints are the id of its distinct taint set; tol_bits holds, per set, the templates that tolerate every taint of it.
#define SI_ABSENT_PASSES 0x80000000u  // tk_key
#define SI_POD_DAEMON 0x80000000u     // pod: the request row's index | this flag (a DaemonSet owns the pod)

#define SI_WAVES 4          // waves per block of the compat and node kernels; the compat kernel gives a node a wave
#define SI_GROUP 16         // lanes the node kernel gives a node: four nodes per wave
#define SI_POOL_THREADS 256
#define SI_POOL_CHUNKS 8    // partial sums per pool: its node list is cut into at most this many slices

struct SiNodeOut {  // kp_sched_node_out
  kp_resource_list available, requests;
  uint32_t n_compatible, reserved;
};
struct SiPoolOut {  // kp_sched_pool_out
  kp_resource_list daemon_requests, remaining;
  uint32_t n_compatible, reserved;
};

struct SchedInArgs {
  int n_nodes, n_tmpl, n_pools, words;  // words = max(1, ceil(n_tmpl / 64))
  // nodes
  const uint32_t* node_val;    // [n_keys][n_nodes] value id, SI_NONE: no such label
  const uint32_t* node_tset;   // [n_nodes] taint-set id
  const kp_resource_list* alloc;  // [n_nodes]
  const kp_resource_list* cap;    // [n_nodes]
  const uint32_t* pod_off;     // [n_nodes + 1]
  const uint32_t* pod;         // request row | SI_POD_DAEMON
  const kp_resource_list* rows;
  // daemonset templates
  const uint64_t* tol_bits;    // [n_tsets][words]
  const uint32_t* tk_off;      // [n_tmpl + 1] the keys of each template's strict requirements
  const uint32_t* tk_key;      // row of node_val | SI_ABSENT_PASSES
  const uint32_t* tk_bits;     // first word, in pass_bits, of the value ids the requirement admits
  const uint64_t* pass_bits;
  const kp_resource_list* tmpl;   // [n_tmpl] requests
  // pools
  const uint32_t* pool_off;    // [n_pools + 1] CSR of the nodes whose karpenter.sh/nodepool label names the pool
  const uint32_t* pool_nodes;
  const uint64_t* pool_compat; // [n_pools][words] templates compatible with the pool's NodeClaimTemplate (host)
  const kp_resource_list* limits;  // [n_pools] spec.limits
  // outputs
  uint64_t* compat;            // [n_nodes][words]
  SiNodeOut* node_out;         // [n_nodes]
  int64_t* part;               // [n_pools][SI_POOL_CHUNKS][KP_NUM_RESOURCES]
  SiPoolOut* pool_out;         // [n_pools]
};

// the four kernels on stream s; nothing is synchronised
hipError_t launch_scheduler_inputs(const SchedInArgs& a, hipStream_t s);
