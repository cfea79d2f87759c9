// kp_cand.hip — kp_cluster_candidates on the device (gfx950; DESIGN §14, the rule: include/kp/kp_abi.h).
//
//   cand_match_kernel      shapes x PDBs: a wave per shape, lanes over the PDBs; per shape the lowest blocking PDB
//   cand_node_kernel       a wave per node, lanes over its pods 64 at a time through the CSR: the int64 cost sum, the
//                          first do-not-disrupt pod and the first PDB-blocked pod by wave reductions, then the reason
//                          ladder, the record and the node's sort key
//   cand_sort_tile_kernel  bitonic network on (key, name rank) inside one CAND_TILE of LDS
//   cand_sort_step_kernel  one compare-exchange distance at or above the tile, in global memory
//   cand_order_kernel      the sorted ranks back to node indices, and the candidate count from the one place where a
//                          candidate is followed by a non-candidate
// Nodes that are no candidates, and the padding up to a power of two, carry the all-ones key and rank: the sort itself
// compacts the candidates to the front. (key, rank) pairs of candidates are distinct, so the network's result is one
// fixed permutation: nothing depends on the order in which blocks or atomics arrive (there are no atomics).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kp/kp_abi.h"
#include "kp_cand.h"

static __device__ inline uint32_t wave_min_u32(uint32_t v) {
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t o = __shfl_xor(v, d, 64);
    v = o < v ? o : v;
  }
  return v;
}
static __device__ inline uint64_t wave_min_u64(uint64_t v) {
  for (int d = 32; d > 0; d >>= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
    v = o < v ? o : v;
  }
  return v;
}
static __device__ inline int64_t wave_sum_i64(int64_t v) {
  for (int d = 32; d > 0; d >>= 1) v += (int64_t)__shfl_xor((long long)v, d, 64);
  return v;
}

__global__ __launch_bounds__(CAND_WAVES * 64) void cand_match_kernel(CandArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * CAND_WAVES + (threadIdx.x >> 6);
  const int n_waves = gridDim.x * CAND_WAVES;
  for (int s = wave; s < a.n_shapes; s += n_waves) {
    const uint64_t* __restrict__ bits = a.shape_bits + (size_t)s * a.words;
    const uint32_t ns = a.shape_ns[s];
    uint32_t best = CAND_NONE;
    for (int p = lane; p < a.n_pdbs && best == CAND_NONE; p += 64) {  // a lane's PDBs ascend: its first match is its lowest
      if (!a.pdb_blocks[p] || a.pdb_ns[p] != ns) continue;
      bool ok = true, any = false;
      const uint32_t end = a.pdb_tok_off[p + 1];
      for (uint32_t t = a.pdb_tok_off[p]; t < end && ok; t++) {
        const uint32_t tok = a.pdb_tok[t];
        const uint32_t id = tok & CAND_TOK_ID;
        const bool set = (bits[id >> 6] >> (id & 63)) & 1;
        const uint32_t kind = tok & CAND_TOK_KIND;
        if (kind == CAND_TOK_MUST) ok = set;
        else if (kind == CAND_TOK_MUSTNOT) ok = !set;
        else {
          any |= set;
          if (tok & CAND_TOK_END) ok = any, any = false;
        }
      }
      if (ok) best = (uint32_t)p;
    }
    best = wave_min_u32(best);
    if (lane == 0) a.verdict[s] = best;
  }
}

// the Go float64 order as an unsigned one: -0.0 is +0.0, negative values reversed below the positive ones
static __device__ inline uint64_t cost_key(double c) {
  uint64_t b = (uint64_t)__double_as_longlong(c);
  if (b == 0x8000000000000000ull) b = 0;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ __launch_bounds__(CAND_WAVES * 64) void cand_node_kernel(CandArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * CAND_WAVES + (threadIdx.x >> 6);
  const int n_waves = gridDim.x * CAND_WAVES;
  // the padding of the sort arrays
  for (uint32_t i = (uint32_t)a.n_nodes + blockIdx.x * blockDim.x + threadIdx.x; i < a.n_pad; i += gridDim.x * blockDim.x) {
    a.keys[i] = ~0ull;
    a.ranks[i] = CAND_NONE;
  }
  const int64_t kOne = (int64_t)1 << 27;
  for (int n = wave; n < a.n_nodes; n += n_waves) {
    const uint32_t lo = a.node_off[n], hi = a.node_off[n + 1];
    int64_t sum = 0;
    uint64_t dnd = ~0ull, blk = ~0ull;  // (position in the node's pods) << 32 | argument, the least one wins
    for (uint32_t i = lo + lane; i < hi; i += 64) {
      const uint32_t p = a.node_pods[i];
      const CandPod r = a.pods[p];
      const uint32_t v = a.verdict[a.pod_shape[p]];
      int64_t fx = kOne + (int64_t)r.deletion_cost + 4 * (int64_t)r.priority;
      fx = fx < -10 * kOne ? -10 * kOne : fx > 10 * kOne ? 10 * kOne : fx;
      sum += fx;
      const uint64_t pos = (uint64_t)(i - lo) << 32;
      if ((r.flags & KP_POD_DO_NOT_DISRUPT) && (pos | p) < dnd) dnd = pos | p;
      if (v != CAND_NONE && (pos | v) < blk) blk = pos | v;
    }
    sum = wave_sum_i64(sum);
    dnd = wave_min_u64(dnd);
    blk = wave_min_u64(blk);
    if (lane != 0) continue;
    const uint32_t st = a.node_static[n];
    const CandNode nd = a.nodes[n];
    const int m = a.method;
    const bool consolidation = m != KP_METHOD_DRIFT;
    const bool pods_pass = m == KP_METHOD_DRIFT && (nd.flags & KP_NODE_TERMINATION_GRACE_PERIOD);
    int32_t reason = KP_CANDIDATE;
    uint32_t detail = 0;
    if (st & CAND_ST_UNMANAGED) reason = KP_NOT_MANAGED;
    else if (nd.flags & KP_NODE_DO_NOT_DISRUPT) reason = KP_NODE_DO_NOT_DISRUPT_REASON;
    else if (st & CAND_ST_UNINITIALIZED) reason = KP_NOT_INITIALIZED;
    else if (st & CAND_ST_DELETING) reason = KP_DELETING;
    else if (nd.flags & KP_NODE_NOMINATED) reason = KP_NOMINATED;
    else if (!pods_pass && dnd != ~0ull) reason = KP_POD_DO_NOT_DISRUPT_REASON, detail = (uint32_t)dnd;
    else if (!pods_pass && blk != ~0ull) reason = KP_PDB_BLOCKED, detail = (uint32_t)blk;
    else {
      const CandPool pl = a.pools[st >> 16];
      const bool single_multi = m == KP_METHOD_SINGLE_NODE || m == KP_METHOD_MULTI_NODE;
      if (consolidation && pl.consolidate_after < 0) reason = KP_CONSOLIDATION_DISABLED;
      else if (single_multi && pl.policy == KP_WHEN_EMPTY) reason = KP_POLICY_WHEN_EMPTY;
      else if (consolidation && a.now - nd.last_pod_event < pl.consolidate_after) reason = KP_NOT_CONSOLIDATABLE;
      else if (m == KP_METHOD_EMPTINESS && hi > lo) reason = KP_NOT_EMPTY;
      else if (m == KP_METHOD_DRIFT && !(nd.flags & KP_NODE_DRIFTED)) reason = KP_NOT_DRIFTED;
    }
    double life = 1.0;
    if (nd.expire_after == 0) life = 0.0;
    else if (nd.expire_after > 0) {
      life = (double)(nd.expire_after - (a.now - nd.created)) / (double)nd.expire_after;
      life = life < 0.0 ? 0.0 : life > 1.0 ? 1.0 : life;
    }
    const double cost = ((double)sum * 0x1p-27) * life;
    CandOut o;
    o.reason = reason, o.detail = detail, o.cost_fx = sum, o.cost = cost;
    a.out[n] = o;
    const uint64_t key = m == KP_METHOD_DRIFT ? ((uint64_t)nd.drifted ^ 0x8000000000000000ull) : cost_key(cost);
    a.keys[n] = reason == KP_CANDIDATE ? key : ~0ull;
    a.ranks[n] = reason == KP_CANDIDATE ? a.node_rank[n] : CAND_NONE;
  }
}

static __device__ inline bool cand_after(uint64_t ka, uint32_t ra, uint64_t kb, uint32_t rb) {
  return ka > kb || (ka == kb && ra > rb);
}

// One tile per block. k_outer == 0: the whole network up to sequences of CAND_TILE (the first pass). Otherwise the
// tail of merge stage k_outer (> CAND_TILE): its distances below the tile.
__global__ __launch_bounds__(CAND_SORT_THREADS) void cand_sort_tile_kernel(uint64_t* __restrict__ keys,
                                                                          uint32_t* __restrict__ ranks, uint32_t k_outer) {
  __shared__ uint64_t sk[CAND_TILE];
  __shared__ uint32_t sr[CAND_TILE];
  const uint32_t base = blockIdx.x * CAND_TILE;
  const uint32_t t = threadIdx.x;
  sk[t] = keys[base + t], sr[t] = ranks[base + t];
  sk[t + CAND_SORT_THREADS] = keys[base + t + CAND_SORT_THREADS], sr[t + CAND_SORT_THREADS] = ranks[base + t + CAND_SORT_THREADS];
  __syncthreads();
  for (uint32_t k = k_outer ? k_outer : 2; k <= (k_outer ? k_outer : CAND_TILE); k <<= 1) {
    for (uint32_t j = (k > CAND_TILE ? CAND_TILE : k) >> 1; j > 0; j >>= 1) {
      const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
      const bool asc = ((base + i) & k) == 0;
      const uint64_t ki = sk[i], kl = sk[l];
      const uint32_t ri = sr[i], rl = sr[l];
      if (cand_after(ki, ri, kl, rl) == asc) sk[i] = kl, sr[i] = rl, sk[l] = ki, sr[l] = ri;
      __syncthreads();
    }
    if (k_outer) break;
  }
  keys[base + t] = sk[t], ranks[base + t] = sr[t];
  keys[base + t + CAND_SORT_THREADS] = sk[t + CAND_SORT_THREADS], ranks[base + t + CAND_SORT_THREADS] = sr[t + CAND_SORT_THREADS];
}

// distance j >= CAND_TILE of merge stage k: one pair per thread, n_pad / 2 pairs
__global__ __launch_bounds__(256) void cand_sort_step_kernel(uint64_t* __restrict__ keys, uint32_t* __restrict__ ranks,
                                                             uint32_t n_pairs, uint32_t k, uint32_t j) {
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_pairs; t += gridDim.x * blockDim.x) {
    const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
    const bool asc = (i & k) == 0;
    const uint64_t ki = keys[i], kl = keys[l];
    const uint32_t ri = ranks[i], rl = ranks[l];
    if (cand_after(ki, ri, kl, rl) == asc) keys[i] = kl, ranks[i] = rl, keys[l] = ki, ranks[l] = ri;
  }
}

__global__ __launch_bounds__(256) void cand_order_kernel(CandArgs a) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n_pad; i += gridDim.x * blockDim.x) {
    const uint32_t r = a.ranks[i];
    if (r == CAND_NONE) {
      if (i == 0) *a.n_cand = 0;
      continue;
    }
    if (i < (uint32_t)a.n_nodes) a.order[i] = a.rank_node[r];  // (a candidate's rank: i < n_candidates <= n_nodes)
    if (i + 1 == a.n_pad || a.ranks[i + 1] == CAND_NONE) *a.n_cand = i + 1;
  }
}

hipError_t launch_candidates(const CandArgs& a, hipStream_t s) {
  if (a.n_shapes > 0) {
    const int blocks = (a.n_shapes + CAND_WAVES - 1) / CAND_WAVES;
    hipLaunchKernelGGL(cand_match_kernel, dim3(blocks < 2048 ? blocks : 2048), dim3(CAND_WAVES * 64), 0, s, a);
  }
  {
    const int blocks = (a.n_nodes + CAND_WAVES - 1) / CAND_WAVES;
    hipLaunchKernelGGL(cand_node_kernel, dim3(blocks < 1 ? 1 : blocks < 2048 ? blocks : 2048), dim3(CAND_WAVES * 64), 0, s, a);
  }
  const uint32_t tiles = a.n_pad / CAND_TILE, n_pairs = a.n_pad / 2;
  const uint32_t step_blocks = (n_pairs + 255) / 256 < 2048 ? (n_pairs + 255) / 256 : 2048;
  hipLaunchKernelGGL(cand_sort_tile_kernel, dim3(tiles), dim3(CAND_SORT_THREADS), 0, s, a.keys, a.ranks, 0u);
  for (uint64_t k = 2ull * CAND_TILE; k <= a.n_pad; k <<= 1) {
    for (uint32_t j = (uint32_t)(k >> 1); j >= CAND_TILE; j >>= 1)
      hipLaunchKernelGGL(cand_sort_step_kernel, dim3(step_blocks), dim3(256), 0, s, a.keys, a.ranks, n_pairs, (uint32_t)k, j);
    hipLaunchKernelGGL(cand_sort_tile_kernel, dim3(tiles), dim3(CAND_SORT_THREADS), 0, s, a.keys, a.ranks, (uint32_t)k);
  }
  hipLaunchKernelGGL(cand_order_kernel, dim3(step_blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}
