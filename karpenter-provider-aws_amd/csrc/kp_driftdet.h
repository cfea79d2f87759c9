// kp_driftdet.h — device data model of kp_cluster_detect_drift (kp_driftdet.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DR_NONE 0xFFFFFFFFu

// Strings never reach the device: every hash, image, subnet, security-group and reservation id of a call is interned to
// an integer (DR_NONE: absent), equal integers meaning equal strings.
struct DrPool {
  int32_t nodeclass;  // -1: none
  uint32_t hash, version, pad;
};
struct DrNode {
  uint32_t flags;  // KP_DRIFT_HAS_INSTANCE
  uint32_t np_hash, np_version, nc_hash, nc_version;
  uint32_t image, subnet, reservation;
};
// one EC2NodeClass: its AMIs are amis [ami_off, ami_off + n_amis) of the call's flat AMI arrays, its id lists rows of
// class_ids, each sorted and distinct
struct DrClass {
  uint32_t hash, version;
  uint32_t ami_off, n_amis;
  uint32_t sg_off, n_sg;
  uint32_t subnet_off, n_subnets;
  uint32_t res_off, n_res;
};
struct DrOut {
  int32_t reason, status;
  uint32_t detail, reserved;
};

// An AMI's requirements compiled against the types' requirement dictionary (keys, and per key the values some type
// carries): a run of groups, one per key of the AMI, each a header word, a count n and n value ids of that key.
//   DR_TOK_ANY  the ids are the values the merged requirement admits (In): it meets a type holding any of them
//   DR_TOK_NOT  the ids are the values it refuses (NotIn, and the values outside Gt / Lt): it meets a type holding a
//               value that is none of them
// DR_TOK_NEGOP: the merged requirement's operator is NotIn or DoesNotExist, which alone passes a type that does not
// define the key, or defines it as DoesNotExist. A lone DR_TOK_NEVER: the AMI can match no type (a key no type defines
// under an operator that is not negative).
#define DR_TOK_KEY 0x00FFFFFFu
#define DR_TOK_ANY (0u << 28)
#define DR_TOK_NOT (1u << 28)
#define DR_TOK_KIND (1u << 28)
#define DR_TOK_NEGOP (1u << 30)
#define DR_TOK_NEVER 0xFFFFFFFFu

#define DR_ABSENT_PASSES 0x80000000u  // pk_first: a node without the key passes the pool's requirement on it

#define DR_WAVES 4            // waves per block of the AMI and node kernels
#define DR_COUNT_THREADS 256
#define DR_COUNT_MAX_BLOCKS 64
#define DR_REASONS 8

struct DriftDetArgs {
  // resident per plan
  const uint32_t* node_pool;     // [n_nodes] owning NodePool, DR_NONE: not managed
  const uint32_t* node_type;     // [n_nodes] used-type index of the node's type inside its pool's catalogue, DR_NONE: not there
  const uint32_t* node_val;      // [n_keys][n_nodes] key-major: the node's value id in the key's dictionary, DR_NONE: no label
  const uint32_t* pool_key_off;  // [n_pools + 1] the distinct keys of each pool's requirements, by first appearance
  const uint32_t* pk_key;        // key index (row of node_val)
  const uint32_t* pk_first;      // index of the key's first requirement in the pool's list | DR_ABSENT_PASSES
  const uint32_t* pk_bits;       // first word, in pass_bits, of the value ids the pool's merged requirement admits
  const uint64_t* pass_bits;
  const uint32_t* type_cnt;      // [n_types][n_tkeys] how many values the type holds under the key, DR_NONE: key undefined
  const uint64_t* type_bits;     // [n_types][type_words] those values, key k's words from tkey_off[k]
  const uint32_t* tkey_off;      // [n_tkeys]
  int n_types, n_tkeys, type_words;
  // per call
  const DrPool* pools;
  const DrNode* nodes;
  const DrClass* classes;
  const uint32_t* node_sg_off;   // [n_nodes + 1] CSR of the instances' security groups, each row sorted and distinct
  const uint32_t* node_sg;
  const uint32_t* class_ids;
  const uint32_t* ami_id;        // [total AMIs] interned image id
  const uint32_t* ami_tok_off;   // [total AMIs + 1]
  const uint32_t* ami_tok;
  const uint32_t* pairs;         // [n_pairs] nodeclass * n_types + type: the (nodeclass, type) pairs some node needs
  int n_pairs;
  uint32_t* ami_of;              // [n_nodeclasses][n_types] index, in the nodeclass's list, of the type's AMI; DR_NONE
  DrOut* out;                    // [n_nodes]
  uint64_t* part;                // [DR_COUNT_MAX_BLOCKS][DR_REASONS]
  uint64_t* counts;              // [DR_REASONS]
  int n_nodes;
};

inline int drift_count_blocks(int n) {
  const int b = (n + DR_COUNT_THREADS - 1) / DR_COUNT_THREADS;
  return b < 1 ? 1 : (b > DR_COUNT_MAX_BLOCKS ? DR_COUNT_MAX_BLOCKS : b);
}

// the AMI map, the per-node ladder and the histogram on stream s; nothing is synchronised
hipError_t launch_detect_drift(const DriftDetArgs& a, hipStream_t s);
