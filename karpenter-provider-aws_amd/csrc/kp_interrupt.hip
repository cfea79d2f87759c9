// kp_interrupt.hip — kp_cluster_interruptions on the device (gfx950; DESIGN §20, the rule: include/kp/kp_abi.h).
//
// The join of message instance ids against the snapshot's nodes is a hash join. The caller's two fills leave the table
// empty and the accumulators at their identities; then, each phase a kernel of its own on the plan's stream:
//   ir_build_kernel    a lane per node with an id: hashes its 32-byte slot and claims the first empty slot of its probe
//                      run with a 32-bit compare-and-swap. Nodes with equal ids take separate slots of one run.
//   ir_probe_kernel    a lane per (message, id) entry: walks the run from the id's home slot to the first empty slot,
//                      compares all 32 bytes of every node on the way, stores its match count and folds the message
//                      into each matching node with integer min / or / add. Which slot a node landed in depends on the
//                      order the build's lanes arrived in; what a walk finds does not: with linear probing and no
//                      removals every node of an id lies between the id's home slot and the next empty one.
//   ir_resolve_kernel  a lane per node: the flags and the 16-byte record, and for a node that carries an ICE mark the
//                      min and add into its (type, zone) pair, reduced over the block first (a table in LDS keyed by
//                      pair; each of its used slots then issues the two global atomics for all the block's nodes)
//   ir_count_kernel    per block of 256 nodes: its deletes, its marks (a node that is the lowest of its pair) and its
//                      deletes per kind, by ballot and popcount
//   ir_scan_kernel     one block, a wave per column: the blocks' exclusive bases in block order, and the totals
//   ir_scatter_kernel  per block again: ballot, prefix inside the wave, the waves' bases through LDS, then the delete
//                      and mark records at base + rank: both lists come out in node order
// Every atomic is an integer min, or, add or compare-and-swap whose result does not depend on arrival order, no
// workgroup waits on another inside a kernel, and every probe loop ends after at most table-size steps.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kp/kp_abi.h"
#include "kp_interrupt.h"

static_assert(sizeof(IrKey) == IR_KEY_BYTES, "a key is two 16-byte loads");
static_assert(IR_THREADS == 256, "four waves per block");

// FNV-1a over the eight words of a slot, then a finalizer so that ids differing in one late byte spread over the low bits
static __device__ inline uint32_t ir_hash(const IrKey& k) {
  const uint32_t w[8] = {k.lo.x, k.lo.y, k.lo.z, k.lo.w, k.hi.x, k.hi.y, k.hi.z, k.hi.w};
  uint32_t h = 0x811C9DC5u;
#pragma unroll
  for (int i = 0; i < 8; i++) h = (h ^ w[i]) * 0x01000193u;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  return h;
}
static __device__ inline bool ir_same(const IrKey& a, const IrKey& b) {
  return a.lo.x == b.lo.x && a.lo.y == b.lo.y && a.lo.z == b.lo.z && a.lo.w == b.lo.w && a.hi.x == b.hi.x &&
         a.hi.y == b.hi.y && a.hi.z == b.hi.z && a.hi.w == b.hi.w;
}

__global__ __launch_bounds__(IR_THREADS) void ir_build_kernel(InterruptArgs a) {
  const int n = blockIdx.x * IR_THREADS + threadIdx.x;
  if (n >= a.n_nodes || !a.node_has_id[n]) return;
  const uint32_t h = ir_hash(a.node_key[n]);
  for (uint32_t i = 0; i <= a.table_mask; i++) {  // (the table has more slots than nodes with an id: one is free)
    const uint32_t slot = (h + i) & a.table_mask;
    if (atomicCAS(&a.table[slot], IR_NONE, (uint32_t)n) == IR_NONE) break;
  }
}

__global__ __launch_bounds__(IR_THREADS) void ir_probe_kernel(InterruptArgs a) {
  const int e = blockIdx.x * IR_THREADS + threadIdx.x;
  if (e >= a.n_entries) return;
  const uint32_t msg = a.entry_msg[e];
  const uint32_t kind = a.msg_kind[msg];
  uint32_t found = 0;
  if (kind != KP_MSG_NO_OP) {
    const IrKey key = a.entry_key[e];
    const uint32_t h = ir_hash(key);
    for (uint32_t i = 0; i <= a.table_mask; i++) {
      const uint32_t node = a.table[(h + i) & a.table_mask];
      if (node == IR_NONE) break;
      if (node >= (uint32_t)a.n_nodes || !ir_same(a.node_key[node], key)) continue;  // (no slot can name a node past the end)
      found++;
      atomicOr(&a.node_kinds[node], 1u << kind);
      atomicAdd(&a.node_count[node], 1u);
      if (kind >= KP_MSG_SCHEDULED_CHANGE) atomicMin(&a.node_first[node], msg);
    }
  }
  a.out_matches[e] = found;
}

static __device__ inline uint32_t ir_flags(uint32_t first, uint32_t kinds, uint32_t pair, bool deleting) {
  uint32_t f = 0;
  if (first != IR_NONE) f |= deleting ? KP_INTERRUPT_ALREADY_DELETING : KP_INTERRUPT_DELETE;
  if ((kinds & (1u << KP_MSG_SPOT_INTERRUPTED)) && pair != IR_NONE) f |= KP_INTERRUPT_ICE;
  return f;
}

__global__ __launch_bounds__(IR_THREADS) void ir_resolve_kernel(InterruptArgs a) {
  // the block's marks by pair: an open-addressing table in LDS with a slot per thread, so it cannot fill up
  __shared__ uint32_t s_pair[IR_THREADS], s_first[IR_THREADS], s_count[IR_THREADS];
  const int tid = threadIdx.x, n = blockIdx.x * IR_THREADS + tid;
  s_pair[tid] = IR_NONE, s_first[tid] = IR_NONE, s_count[tid] = 0;
  __syncthreads();
  if (n < a.n_nodes) {
    const uint32_t first = a.node_first[n], kinds = a.node_kinds[n], pair = a.node_pair[n];
    const uint32_t flags = ir_flags(first, kinds, pair, a.node_deleting[n] != 0);
    // the 16-byte record in one vector store; an untouched first reads as -1
    reinterpret_cast<uint4*>(a.out_nodes)[n] = make_uint4(first, kinds, a.node_count[n], flags);
    if ((flags & KP_INTERRUPT_ICE) && pair < (uint32_t)a.n_pairs) {
      for (uint32_t i = 0; i < IR_THREADS; i++) {
        const uint32_t slot = (pair + i) & (IR_THREADS - 1);
        const uint32_t held = atomicCAS(&s_pair[slot], IR_NONE, pair);
        if (held != IR_NONE && held != pair) continue;
        atomicMin(&s_first[slot], (uint32_t)n);
        atomicAdd(&s_count[slot], 1u);
        break;
      }
    }
  }
  __syncthreads();
  // one pair of global atomics per distinct pair of the block
  if (s_pair[tid] != IR_NONE) {
    atomicMin(&a.pair_first[s_pair[tid]], s_first[tid]);
    atomicAdd(&a.pair_count[s_pair[tid]], s_count[tid]);
  }
}

// what node n adds to the two lists: bit 0 a delete, bit 1 a mark; *kind the kind of its first acting message
static __device__ inline uint32_t ir_emits(const InterruptArgs& a, int n, uint32_t* first, uint32_t* kind) {
  if (n >= a.n_nodes) return 0;
  const IrNodeOut r = a.out_nodes[n];
  uint32_t out = 0;
  if (r.flags & KP_INTERRUPT_DELETE) {
    *first = (uint32_t)r.first_message;
    *kind = a.msg_kind[*first];
    out |= 1;
  }
  if (r.flags & KP_INTERRUPT_ICE) {
    const uint32_t p = a.node_pair[n];
    if (p < (uint32_t)a.n_pairs && a.pair_first[p] == (uint32_t)n) out |= 2;
  }
  return out;
}

__global__ __launch_bounds__(IR_THREADS) void ir_count_kernel(InterruptArgs a) {
  __shared__ uint32_t s[IR_THREADS / 64][6];
  const int n = blockIdx.x * IR_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t first = 0, kind = 0;
  const uint32_t em = ir_emits(a, n, &first, &kind);
  const unsigned long long del = __ballot(em & 1), mark = __ballot(em & 2);
  if (lane == 0) s[wave][0] = (uint32_t)__popcll(del), s[wave][1] = (uint32_t)__popcll(mark);
#pragma unroll
  for (uint32_t k = KP_MSG_SCHEDULED_CHANGE; k <= KP_MSG_INSTANCE_TERMINATED; k++) {
    const unsigned long long m = __ballot((em & 1) && kind == k);
    if (lane == 0) s[wave][k] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (threadIdx.x < IR_SUMS) {
    uint32_t t = 0;
    if (threadIdx.x < 6)
      for (int w = 0; w < IR_THREADS / 64; w++) t += s[w][threadIdx.x];
    a.block_sums[(size_t)blockIdx.x * IR_SUMS + threadIdx.x] = t;
  }
}

// one block, a wave per column of the blocks' sums: 64 blocks at a time, an inclusive scan across the lanes and the
// carry of the passes before, leaving each block's exclusive base in place and the column's total
__global__ __launch_bounds__(IR_SUMS * 64) void ir_scan_kernel(InterruptArgs a, int n_blocks) {
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t run = 0;
  for (int base = 0; base < n_blocks; base += 64) {  // (wave-uniform bounds: every lane reaches the shuffles)
    const int b = base + lane;
    const uint32_t v = b < n_blocks ? a.block_sums[(size_t)b * IR_SUMS + k] : 0u;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t below = __shfl_up(inc, o, 64);
      if (lane >= o) inc += below;
    }
    if (b < n_blocks) a.block_sums[(size_t)b * IR_SUMS + k] = run + inc - v;
    run += __shfl(inc, 63, 64);
  }
  if (lane == 0) a.totals[k] = run;
}

__global__ __launch_bounds__(IR_THREADS) void ir_scatter_kernel(InterruptArgs a) {
  __shared__ uint32_t s[IR_THREADS / 64][2];
  const int n = blockIdx.x * IR_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t first = 0, kind = 0;
  const uint32_t em = ir_emits(a, n, &first, &kind);
  const unsigned long long del = __ballot(em & 1), mark = __ballot(em & 2);
  const unsigned long long below = (1ull << lane) - 1;
  if (lane == 0) s[wave][0] = (uint32_t)__popcll(del), s[wave][1] = (uint32_t)__popcll(mark);
  __syncthreads();
  uint32_t dbase = a.block_sums[(size_t)blockIdx.x * IR_SUMS + 0], mbase = a.block_sums[(size_t)blockIdx.x * IR_SUMS + 1];
  for (int w = 0; w < wave; w++) dbase += s[w][0], mbase += s[w][1];
  if (em & 1) {
    const uint32_t at = dbase + (uint32_t)__popcll(del & below);
    if (at < (uint32_t)a.n_nodes)  // (a list holds at most one record per node)
      reinterpret_cast<uint4*>(a.deletes)[at] = make_uint4((uint32_t)n, first, kind, 0u);
  }
  if (em & 2) {
    const uint32_t at = mbase + (uint32_t)__popcll(mark & below);
    if (at < (uint32_t)a.n_nodes)
      reinterpret_cast<uint2*>(a.marks)[at] = make_uint2((uint32_t)n, a.pair_count[a.node_pair[n]]);
  }
}

hipError_t launch_interruptions(const InterruptArgs& a, hipStream_t s) {
  const int nb = interrupt_blocks(a.n_nodes);
  if (a.n_nodes > 0) {
    hipLaunchKernelGGL(ir_build_kernel, dim3(nb), dim3(IR_THREADS), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  if (a.n_entries > 0) {
    hipLaunchKernelGGL(ir_probe_kernel, dim3(interrupt_blocks(a.n_entries)), dim3(IR_THREADS), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  if (a.n_nodes > 0) {
    hipLaunchKernelGGL(ir_resolve_kernel, dim3(nb), dim3(IR_THREADS), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(ir_count_kernel, dim3(nb), dim3(IR_THREADS), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(ir_scan_kernel, dim3(1), dim3(IR_SUMS * 64), 0, s, a, nb);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (a.n_nodes > 0) {
    hipLaunchKernelGGL(ir_scatter_kernel, dim3(nb), dim3(IR_THREADS), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}
