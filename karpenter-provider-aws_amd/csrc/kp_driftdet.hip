// kp_driftdet.hip — kp_cluster_detect_drift on the device (gfx950; DESIGN §16, the rule: include/kp/kp_abi.h).
//
//   drift_ami_kernel    a wave per (nodeclass, type some node of it runs), lanes over the nodeclass's AMIs 64 at a time:
//                       each lane judges type.Requirements.Compatible(its AMI's requirements) from the type's row and
//                       the AMI's tokens, a ballot gives the lowest compatible AMI of the pass, the first pass that has
//                       one ends the walk. Writes ami_of[nodeclass][type], MapToInstanceTypes for one type
//   drift_node_kernel   a thread per node: the ladder of kp_abi.h on interned integers. A node's ladder is a dozen
//                       dependent loads with no loop long enough to feed 64 lanes (a pool names a few keys, an
//                       instance a few security groups), so a wave per node would idle 63 of them; with a thread per
//                       node a wave reads 64 consecutive nodes of the key-major value table and of the per-node
//                       arrays in one coalesced load each
//   drift_count_kernel  (+ final) the histogram of the reasons, built as why_count_kernel is: integer partials per
//                       block, one block adds them in block order
// Every word of the output has one writer and there are no atomics: nothing depends on the order blocks run in.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kp/kp_abi.h"
#include "kp_driftdet.h"

static_assert(DR_REASONS == KP_DRIFT_REASON_COUNT, "the histogram has one bin per reason");

__global__ __launch_bounds__(DR_WAVES * 64) void drift_ami_kernel(DriftDetArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * DR_WAVES + (threadIdx.x >> 6);
  const int n_waves = gridDim.x * DR_WAVES;
  for (int p = wave; p < a.n_pairs; p += n_waves) {
    const uint32_t pair = a.pairs[p];
    const uint32_t nc = pair / (uint32_t)a.n_types, u = pair % (uint32_t)a.n_types;
    const DrClass c = a.classes[nc];
    const uint32_t* __restrict__ cnt = a.type_cnt + (size_t)u * a.n_tkeys;
    const uint64_t* __restrict__ row = a.type_bits + (size_t)u * a.type_words;
    uint32_t found = DR_NONE;
    for (uint32_t base = 0; base < c.n_amis; base += 64) {  // (wave-uniform bounds: every lane reaches the ballot)
      const uint32_t i = base + lane;
      bool ok = i < c.n_amis;
      if (ok) {
        uint32_t t = a.ami_tok_off[c.ami_off + i];
        const uint32_t end = a.ami_tok_off[c.ami_off + i + 1];
        while (t < end && ok) {
          const uint32_t hdr = a.ami_tok[t];
          if (hdr == DR_TOK_NEVER) {
            ok = false;
            break;
          }
          const uint32_t n = a.ami_tok[t + 1], key = hdr & DR_TOK_KEY;
          t += 2;
          const uint32_t held = cnt[key];
          if (held == DR_NONE) {  // the type does not define the key
            ok = (hdr & DR_TOK_NEGOP) != 0;
          } else {
            const uint64_t* __restrict__ bits = row + a.tkey_off[key];
            uint32_t hits = 0;
            for (uint32_t j = 0; j < n; j++) {
              const uint32_t id = a.ami_tok[t + j];
              hits += (uint32_t)((bits[id >> 6] >> (id & 63)) & 1);
            }
            const bool meets = (hdr & DR_TOK_KIND) == DR_TOK_ANY ? hits > 0 : held > hits;
            ok = meets || (held == 0 && (hdr & DR_TOK_NEGOP));
          }
          t += n;
        }
      }
      const unsigned long long m = __ballot(ok);
      if (m) {
        found = base + (uint32_t)(__ffsll(m) - 1);
        break;
      }
    }
    if (lane == 0) a.ami_of[pair] = found;
  }
}

// both lists sorted and distinct: sets are equal iff the lists are
static __device__ inline bool same_ids(const uint32_t* x, uint32_t nx, const uint32_t* y, uint32_t ny) {
  if (nx != ny) return false;
  for (uint32_t i = 0; i < nx; i++)
    if (x[i] != y[i]) return false;
  return true;
}
static __device__ inline bool has_id(const uint32_t* x, uint32_t n, uint32_t id) {
  uint32_t lo = 0, hi = n;  // first position whose id is >= id
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (x[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && x[lo] == id;
}
static __device__ inline bool static_drift(uint32_t h0, uint32_t v0, uint32_t h1, uint32_t v1) {
  return h0 != DR_NONE && v0 != DR_NONE && h1 != DR_NONE && v1 != DR_NONE && v0 == v1 && h0 != h1;
}

__global__ __launch_bounds__(DR_WAVES * 64) void drift_node_kernel(DriftDetArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.n_nodes) return;
  int32_t reason = KP_DRIFT_NONE, status = KP_DRIFT_OK;
  uint32_t detail = 0;
  const uint32_t pool = a.node_pool[n];
  if (pool == DR_NONE) {
    status = KP_DRIFT_SKIP_NOT_MANAGED;
  } else {
    const DrPool pd = a.pools[pool];
    const DrNode nd = a.nodes[n];
    if (pd.nodeclass < 0) {
      status = KP_DRIFT_SKIP_NO_NODECLASS;
    } else if (static_drift(pd.hash, pd.version, nd.np_hash, nd.np_version)) {
      reason = KP_DRIFT_NODEPOOL;
    } else {
      const uint32_t k_end = a.pool_key_off[pool + 1];
      for (uint32_t e = a.pool_key_off[pool]; e < k_end; e++) {
        const uint32_t first = a.pk_first[e];
        const uint32_t v = a.node_val[(size_t)a.pk_key[e] * a.n_nodes + n];
        const bool pass = v == DR_NONE ? (first & DR_ABSENT_PASSES) != 0
                                       : ((a.pass_bits[a.pk_bits[e] + (v >> 6)] >> (v & 63)) & 1) != 0;
        if (!pass) {
          reason = KP_DRIFT_REQUIREMENTS;
          detail = first & ~DR_ABSENT_PASSES;
          break;
        }
      }
      if (reason == KP_DRIFT_NONE) {
        const DrClass c = a.classes[pd.nodeclass];
        const uint32_t ut = a.node_type[n];
        if (static_drift(c.hash, c.version, nd.nc_hash, nd.nc_version)) {
          reason = KP_DRIFT_NODECLASS;
        } else if (!(nd.flags & KP_DRIFT_HAS_INSTANCE)) {
          status = KP_DRIFT_ERR_INSTANCE;
        } else if (ut == DR_NONE) {
          status = KP_DRIFT_ERR_INSTANCE_TYPE;
        } else if (c.n_amis == 0) {
          status = KP_DRIFT_ERR_NO_AMIS;
        } else if (c.n_sg == 0) {
          status = KP_DRIFT_ERR_NO_SECURITY_GROUPS;
        } else if (c.n_subnets == 0) {
          status = KP_DRIFT_ERR_NO_SUBNETS;
        } else {
          const uint32_t ami = a.ami_of[(size_t)pd.nodeclass * a.n_types + ut];
          const uint32_t sg_lo = a.node_sg_off[n], sg_hi = a.node_sg_off[n + 1];
          if (ami == DR_NONE || a.ami_id[c.ami_off + ami] != nd.image) {
            reason = KP_DRIFT_AMI;
            detail = ami;
          } else if (!same_ids(a.class_ids + c.sg_off, c.n_sg, a.node_sg + sg_lo, sg_hi - sg_lo)) {
            reason = KP_DRIFT_SECURITY_GROUP;
          } else if (!has_id(a.class_ids + c.subnet_off, c.n_subnets, nd.subnet)) {
            reason = KP_DRIFT_SUBNET;
          } else if (nd.reservation != DR_NONE && !has_id(a.class_ids + c.res_off, c.n_res, nd.reservation)) {
            reason = KP_DRIFT_CAPACITY_RESERVATION;
          }
        }
      }
    }
  }
  // the 16-byte record in one vector store
  reinterpret_cast<uint4*>(a.out)[n] = make_uint4((uint32_t)reason, (uint32_t)status, detail, 0u);
}

__global__ __launch_bounds__(DR_COUNT_THREADS) void drift_count_kernel(const DrOut* out, int n, uint64_t* part) {
  __shared__ uint32_t s_cnt[DR_COUNT_THREADS / 64][DR_REASONS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int per = (n + gridDim.x - 1) / gridDim.x;
  const int lo = blockIdx.x * per, hi = min(n, lo + per);
  uint32_t c[DR_REASONS];
#pragma unroll
  for (int k = 0; k < DR_REASONS; k++) c[k] = 0;
  for (int i = lo + tid; i < hi; i += DR_COUNT_THREADS) {
    const uint32_t reason = (uint32_t)out[i].reason;
#pragma unroll
    for (int k = 0; k < DR_REASONS; k++) c[k] += reason == (uint32_t)k ? 1u : 0u;
  }
#pragma unroll
  for (int k = 0; k < DR_REASONS; k++) {
    uint32_t v = c[k];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) s_cnt[wave][k] = v;
  }
  __syncthreads();
  if (tid < DR_REASONS) {
    uint64_t t = 0;
    for (int w = 0; w < DR_COUNT_THREADS / 64; w++) t += s_cnt[w][tid];
    part[(size_t)blockIdx.x * DR_REASONS + tid] = t;
  }
}
// one block: thread k adds the partials of reason k, in block order
__global__ __launch_bounds__(64) void drift_count_final_kernel(const uint64_t* part, int np, uint64_t* counts) {
  const int k = threadIdx.x;
  if (k >= DR_REASONS) return;
  uint64_t t = 0;
  for (int b = 0; b < np; b++) t += part[(size_t)b * DR_REASONS + k];
  counts[k] = t;
}

hipError_t launch_detect_drift(const DriftDetArgs& a, hipStream_t s) {
  if (a.n_pairs > 0) {
    const int blocks = (a.n_pairs + DR_WAVES - 1) / DR_WAVES;
    hipLaunchKernelGGL(drift_ami_kernel, dim3(blocks < 1024 ? blocks : 1024), dim3(DR_WAVES * 64), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  const int nb = drift_count_blocks(a.n_nodes);
  if (a.n_nodes > 0) {
    hipLaunchKernelGGL(drift_node_kernel, dim3((a.n_nodes + DR_WAVES * 64 - 1) / (DR_WAVES * 64)), dim3(DR_WAVES * 64), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(drift_count_kernel, dim3(nb), dim3(DR_COUNT_THREADS), 0, s, a.out, a.n_nodes, a.part);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(drift_count_final_kernel, dim3(1), dim3(64), 0, s, a.part, a.n_nodes > 0 ? nb : 0, a.counts);
  return hipGetLastError();
}
