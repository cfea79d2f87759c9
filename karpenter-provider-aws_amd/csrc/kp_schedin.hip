// kp_schedin.hip — kp_scheduler_inputs on the device (gfx950, wave64; DESIGN §17, the rule: include/kp/kp_abi.h).
//
//   schedin_compat_kernel      a wave per node, lanes over the daemonset templates 64 at a time: each lane reads its
//                              template's bit of the node's taint set, then tests every key of the template's strict
//                              requirements against the node's value id (one bitset word per test); a ballot gives
//                              one compatibility word per pass. The words are an output and the next kernel's input
//   schedin_node_kernel        16 lanes per node, four nodes per wave: lanes add the request rows of the templates the
//                              words select, and the request rows of the node's bound pods (all of them, and the
//                              daemonset-owned ones), 12 int64 each; a shuffle butterfly over the 16 lanes leaves the
//                              totals in each of them; lanes 0..11 then subtract, clamp, mask and store one resource
//                              each. (A wave per node spent its time in 36 six-step 64-bit butterflies that 30 pods
//                              and 50 templates do not need: 62 us at 10,000 nodes.)
//   schedin_pool_kernel        block (slice, pool): the capacity of a fixed slice of the pool's node list, one partial
//   schedin_pool_final_kernel  a wave per pool: adds the pool's partials in slice order and subtracts them from its
//                              limits; lanes over the templates the host found compatible with the pool's
//                              NodeClaimTemplate add their request rows
// Every word of the output has one writer and there are no atomics: the result does not depend on the order blocks
// run in. All arithmetic is int64 milli-units.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kp/kp_abi.h"
#include "kp_schedin.h"

#define SI_R KP_NUM_RESOURCES
static_assert(SI_GROUP > SI_R && 64 % SI_GROUP == 0, "a group holds a lane per resource and one for the masks");

static __device__ inline int64_t wave_sum(int64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
static __device__ inline uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}
// acc += the present resources of l
static __device__ inline void add_row(int64_t (&acc)[SI_R], const kp_resource_list& l) {
  const uint32_t m = l.present;
#pragma unroll
  for (int r = 0; r < SI_R; r++) acc[r] += (m >> r) & 1 ? l.milli[r] : 0;
}

__global__ __launch_bounds__(SI_WAVES * 64) void schedin_compat_kernel(SchedInArgs a) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * SI_WAVES + (threadIdx.x >> 6);  // wave-uniform
  if (n >= a.n_nodes) return;
  const uint64_t* __restrict__ tol = a.tol_bits + (size_t)a.node_tset[n] * a.words;
  for (int w = 0; w < a.words; w++) {  // (wave-uniform bounds: every lane reaches the ballot)
    const int d = w * 64 + lane;
    bool ok = d < a.n_tmpl && ((tol[w] >> lane) & 1) != 0;
    if (ok) {
      const uint32_t end = a.tk_off[d + 1];
      for (uint32_t e = a.tk_off[d]; e < end && ok; e++) {
        const uint32_t key = a.tk_key[e];
        const uint32_t v = a.node_val[(size_t)(key & ~SI_ABSENT_PASSES) * a.n_nodes + n];
        ok = v == SI_NONE ? (key & SI_ABSENT_PASSES) != 0 : ((a.pass_bits[a.tk_bits[e] + (v >> 6)] >> (v & 63)) & 1) != 0;
      }
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) a.compat[(size_t)n * a.words + w] = m;
  }
}

// the sum over the 16 lanes of a group, left in each of them
static __device__ inline int64_t group_sum(int64_t v) {
#pragma unroll
  for (int o = SI_GROUP / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
static __device__ inline uint32_t group_or(uint32_t v) {
#pragma unroll
  for (int o = SI_GROUP / 2; o >= 1; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(SI_WAVES * 64) void schedin_node_kernel(SchedInArgs a) {
  const int lane = threadIdx.x & (SI_GROUP - 1);  // within the node's group of 16 lanes
  const int n = (blockIdx.x * SI_WAVES * 64 + threadIdx.x) / SI_GROUP;
  const bool live = n < a.n_nodes;  // (a dead group runs the shuffles on zeros and stores nothing)
  int64_t expect[SI_R], bound[SI_R], daemon[SI_R];
#pragma unroll
  for (int r = 0; r < SI_R; r++) expect[r] = bound[r] = daemon[r] = 0;
  uint32_t mask = 0, count = 0;
  if (live) {
    for (int d = lane; d < a.n_tmpl; d += SI_GROUP) {
      if ((a.compat[(size_t)n * a.words + (d >> 6)] >> (d & 63)) & 1) {
        const kp_resource_list& t = a.tmpl[d];
        add_row(expect, t);
        mask |= t.present;
        count++;
      }
    }
    const uint32_t end = a.pod_off[n + 1];
    for (uint32_t i = a.pod_off[n] + lane; i < end; i += SI_GROUP) {
      const uint32_t p = a.pod[i];
      const kp_resource_list& q = a.rows[p & ~SI_POD_DAEMON];
      add_row(bound, q);
      if (p & SI_POD_DAEMON) add_row(daemon, q);
    }
  }
  mask = group_or(mask);
  count = (uint32_t)group_sum((int64_t)count);
  // the butterfly leaves every total in every lane of the group; lane r keeps resource r
  int64_t e = 0, b = 0, dm = 0;
#pragma unroll
  for (int r = 0; r < SI_R; r++) {
    const int64_t se = group_sum(expect[r]), sb = group_sum(bound[r]), sd = group_sum(daemon[r]);
    if (lane == r) e = se, b = sb, dm = sd;
  }
  if (!live) return;
  SiNodeOut* out = a.node_out + n;
  if (lane < SI_R) {
    const kp_resource_list& al = a.alloc[n];
    const int64_t rest = e - dm;
    out->available.milli[lane] = (al.present >> lane) & 1 ? al.milli[lane] - b : 0;
    out->requests.milli[lane] = (mask >> lane) & 1 ? (rest > 0 ? rest : 0) : 0;
  } else if (lane == SI_R) {
    out->available.present = a.alloc[n].present & ((1u << SI_R) - 1);
    out->available.reserved_ = 0;
    out->requests.present = mask & ((1u << SI_R) - 1);
    out->requests.reserved_ = 0;
    out->n_compatible = count;
    out->reserved = 0;
  }
}

__global__ __launch_bounds__(SI_POOL_THREADS) void schedin_pool_kernel(SchedInArgs a) {
  __shared__ int64_t s_sum[SI_POOL_THREADS / 64][SI_R];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int p = blockIdx.y, c = blockIdx.x;
  const uint32_t lo0 = a.pool_off[p], len = a.pool_off[p + 1] - lo0;
  // the slices: at most SI_POOL_CHUNKS of them, each a whole number of block strides
  uint32_t per = (len + SI_POOL_CHUNKS - 1) / SI_POOL_CHUNKS;
  per = (per + SI_POOL_THREADS - 1) / SI_POOL_THREADS * SI_POOL_THREADS;
  const uint64_t lo = (uint64_t)c * per;
  const uint64_t hi = lo + per < len ? lo + per : len;
  int64_t acc[SI_R];
#pragma unroll
  for (int r = 0; r < SI_R; r++) acc[r] = 0;
  for (uint64_t i = lo + tid; i < hi; i += SI_POOL_THREADS) add_row(acc, a.cap[a.pool_nodes[lo0 + i]]);
#pragma unroll
  for (int r = 0; r < SI_R; r++) {
    const int64_t v = wave_sum(acc[r]);
    if (lane == 0) s_sum[wave][r] = v;
  }
  __syncthreads();
  if (tid < SI_R) {
    int64_t t = 0;
    for (int w = 0; w < SI_POOL_THREADS / 64; w++) t += s_sum[w][tid];
    a.part[((size_t)p * SI_POOL_CHUNKS + c) * SI_R + tid] = t;
  }
}

__global__ __launch_bounds__(64) void schedin_pool_final_kernel(SchedInArgs a) {
  const int lane = threadIdx.x, p = blockIdx.x;
  int64_t expect[SI_R];
#pragma unroll
  for (int r = 0; r < SI_R; r++) expect[r] = 0;
  uint32_t mask = 0, count = 0;
  for (int w = 0; w < a.words; w++) {
    const int d = w * 64 + lane;
    if (d < a.n_tmpl && ((a.pool_compat[(size_t)p * a.words + w] >> lane) & 1)) {
      const kp_resource_list& t = a.tmpl[d];
      add_row(expect, t);
      mask |= t.present;
      count++;
    }
  }
  mask = wave_or(mask);
  count = (uint32_t)wave_sum((int64_t)count);
  int64_t e = 0;
#pragma unroll
  for (int r = 0; r < SI_R; r++) {
    const int64_t se = wave_sum(expect[r]);
    if (lane == r) e = se;
  }
  SiPoolOut* out = a.pool_out + p;
  if (lane < SI_R) {
    int64_t used = 0;
    for (int c = 0; c < SI_POOL_CHUNKS; c++) used += a.part[((size_t)p * SI_POOL_CHUNKS + c) * SI_R + lane];
    const kp_resource_list& lim = a.limits[p];
    out->daemon_requests.milli[lane] = (mask >> lane) & 1 ? e : 0;
    out->remaining.milli[lane] = (lim.present >> lane) & 1 ? lim.milli[lane] - used : 0;
  } else if (lane == SI_R) {
    out->daemon_requests.present = mask & ((1u << SI_R) - 1);
    out->daemon_requests.reserved_ = 0;
    out->remaining.present = a.limits[p].present & ((1u << SI_R) - 1);
    out->remaining.reserved_ = 0;
    out->n_compatible = count;
    out->reserved = 0;
  }
}

hipError_t launch_scheduler_inputs(const SchedInArgs& a, hipStream_t s) {
  if (a.n_nodes > 0) {
    const int blocks = (a.n_nodes + SI_WAVES - 1) / SI_WAVES;
    hipLaunchKernelGGL(schedin_compat_kernel, dim3(blocks), dim3(SI_WAVES * 64), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const int per_block = SI_WAVES * 64 / SI_GROUP;
    hipLaunchKernelGGL(schedin_node_kernel, dim3((a.n_nodes + per_block - 1) / per_block), dim3(SI_WAVES * 64), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  if (a.n_pools > 0) {
    hipLaunchKernelGGL(schedin_pool_kernel, dim3(SI_POOL_CHUNKS, a.n_pools), dim3(SI_POOL_THREADS), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(schedin_pool_final_kernel, dim3(a.n_pools), dim3(64), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}
