// kp_cand.h — device data model of kp_cluster_candidates (kp_cand.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// kp_pool_disruption / kp_node_disruption / kp_pod_disruption / kp_candidate as the device reads and writes them
struct CandPool {
  int32_t policy, pad;
  int64_t consolidate_after;
};
struct CandNode {
  uint32_t flags, pad;
  int64_t created, expire_after, last_pod_event, drifted;
};
struct CandPod {
  int32_t priority, deletion_cost;
  uint32_t flags, pad;
};
struct CandOut {
  int32_t reason;
  uint32_t detail;
  int64_t cost_fx;
  double cost;
};

#define CAND_NONE 0xFFFFFFFFu
// node_static[n]: what the snapshot itself says of node n; the owning NodePool sits in the high half
#define CAND_ST_UNMANAGED 1u
#define CAND_ST_UNINITIALIZED 2u
#define CAND_ST_DELETING 4u
// A PDB selector compiled against the plan's label dictionary: a run of tokens, each a bit of the shapes' label bitsets
// (a label pair or a label key) and what the selector asks of it. The members of one In expression are consecutive ANY
// tokens, the last one marked CAND_TOK_END.
#define CAND_TOK_ID 0x0FFFFFFFu
#define CAND_TOK_MUST (0u << 28)     // matchLabels pair, Exists key
#define CAND_TOK_MUSTNOT (1u << 28)  // NotIn pair, DoesNotExist key
#define CAND_TOK_ANY (2u << 28)      // In pair
#define CAND_TOK_KIND (3u << 28)
#define CAND_TOK_END (1u << 30)

#define CAND_WAVES 4       // waves per block of the match and node kernels
#define CAND_TILE 2048     // keys one workgroup sorts in LDS (24 KiB)
#define CAND_SORT_THREADS (CAND_TILE / 2)

struct CandArgs {
  // resident per plan
  const uint32_t* node_off;     // [n_nodes + 1] CSR of the nodes' reschedulable pods
  const uint32_t* node_pods;    // cluster pod indices, each node's in its `pods` order
  const uint32_t* pod_shape;    // [n_pods]
  const uint32_t* node_static;  // [n_nodes] CAND_ST_* | pool << 16
  const uint32_t* node_rank;    // [n_nodes] rank of the node's name (bytes, then index): distinct
  const uint32_t* rank_node;    // its inverse
  const uint64_t* shape_bits;   // [n_shapes][words] label pairs and label keys of the shape
  const uint32_t* shape_ns;     // [n_shapes] namespace id
  int n_shapes, words;
  // per call
  const CandPool* pools;
  const CandNode* nodes;
  const CandPod* pods;
  const uint32_t* pdb_ns;       // [n_pdbs] namespace id (CAND_NONE: a namespace without pods)
  const uint8_t* pdb_blocks;    // [n_pdbs] 1: disruptions_allowed == 0 and the selector can match
  const uint32_t* pdb_tok_off;  // [n_pdbs + 1]
  const uint32_t* pdb_tok;
  int n_pdbs;
  uint32_t* verdict;            // [n_shapes] lowest blocking PDB or CAND_NONE
  CandOut* out;                 // [n_nodes]
  uint64_t* keys;               // [n_pad] sort key; ~0 for a node that is no candidate and for the padding
  uint32_t* ranks;              // [n_pad] name rank below the key; CAND_NONE likewise
  uint32_t* order;              // [n_nodes]
  uint32_t* n_cand;
  int n_nodes;
  uint32_t n_pad;               // power of two >= max(n_nodes, CAND_TILE)
  int64_t now;
  int method;
};

// match, per-node ladder, sort and order on stream s; nothing is synchronised
hipError_t launch_candidates(const CandArgs& a, hipStream_t s);
