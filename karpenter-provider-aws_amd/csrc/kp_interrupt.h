// kp_interrupt.h — device data model of kp_cluster_interruptions (kp_interrupt.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define IR_NONE 0xFFFFFFFFu   // an empty table slot; a node without both labels; a pair no node carries yet
#define IR_KEY_BYTES 32       // an instance id in a zero-padded slot: at most 31 bytes and the terminator
#define IR_THREADS 256        // every kernel's block: 4 waves
#define IR_NODE_HAS_ID 1u     // node_state bits
#define IR_NODE_DELETING 2u
#define IR_SUMS 8             // per block: deletes, marks, deletes of kinds 2..5, two spare words

struct IrKey {                // compared as two 16-byte loads
  uint4 lo, hi;
};
struct IrNodeOut {            // kp_interrupt_node
  int32_t first_message;
  uint32_t kinds, n_messages, flags;
};
struct IrDelete {             // kp_interrupt_delete
  uint32_t node, message;
  int32_t kind;
  uint32_t reserved;
};
struct IrMark {               // kp_interrupt_mark
  uint32_t node, n_nodes;
};

struct InterruptArgs {
  // resident per plan
  const uint32_t* node_pair;   // [n_nodes] id of the node's (instance-type label, zone label) pair, IR_NONE: lacks one
  const uint8_t* node_deleting;  // [n_nodes]
  int n_pairs;
  // per call, uploaded
  const IrKey* node_key;       // [n_nodes]
  const uint8_t* node_has_id;  // [n_nodes]
  const IrKey* entry_key;      // [n_entries] one per (message, id)
  const uint32_t* entry_msg;   // [n_entries] the entry's message
  const uint8_t* msg_kind;     // [n_messages]
  int n_nodes, n_entries;
  uint32_t table_mask;         // table size - 1, the size a power of two above the number of nodes with an id
  // per call, device only. `ones` (table, node_first, pair_first) starts as all-ones words, `zeros` (node_kinds,
  // node_count, pair_count) as zero words: one fill each
  uint32_t* table;             // [table_mask + 1] node index, IR_NONE: empty
  uint32_t* node_first;        // [n_nodes] min over acting matches of the message index; IR_NONE reads as -1
  uint32_t* pair_first;        // [n_pairs] min over ICE nodes of the node index
  uint32_t* node_kinds;        // [n_nodes]
  uint32_t* node_count;        // [n_nodes]
  uint32_t* pair_count;        // [n_pairs] ICE nodes of the pair
  uint32_t* block_sums;        // [n_blocks][IR_SUMS], then exclusive bases in place; n_blocks = interrupt_blocks(n_nodes)
  // outputs
  IrNodeOut* out_nodes;        // [n_nodes]
  uint32_t* out_matches;       // [n_entries]
  IrDelete* deletes;           // [n_nodes]
  IrMark* marks;               // [n_nodes]
  uint32_t* totals;            // [IR_SUMS] n_deletes, n_marks, deletes of kinds 2..5
};

inline int interrupt_blocks(int n) { return (n + IR_THREADS - 1) / IR_THREADS; }

// build, probe, resolve and the three compaction passes on stream s, after the caller's two fills; nothing is synchronised
hipError_t launch_interruptions(const InterruptArgs& a, hipStream_t s);
