// kp_catcomp.hip — the kernels of kp_catalog_compile: NewInstanceType's capacity and overhead lists and
// createOfferings' prices and availability for every (NodeClass, instance type) pair. Lanes run over the instance
// types (the type facts are a structure of arrays, so a wave's loads coalesce), a grid row is a NodeClass (its record
// is wave-uniform). No atomics, no LDS, no cross-lane traffic: every lane owns its outputs.
//
// The float64 steps (memory()'s VM overhead, the eviction percentages, the kube-reserved CPU ranges, the reserved
// price) are each one multiply or divide chain ending in ceil or a truncation, never followed by an add: this file is
// compiled with -ffp-contract=off and without fast-math so that the device's bits are the host's
// (kp_instance_type_resolve / kp_instance_type_overhead in kp_host.cpp, which the tests compare against).
#include "kp_catcomp.h"

namespace {

constexpr int CC_R = KP_NUM_RESOURCES;
constexpr int64_t kMiB = 1048576ll;

__device__ __forceinline__ void set_res(kp_resource_list& l, int r, int64_t v) {
  l.milli[r] = v;
  l.present |= 1u << r;
}
__device__ __forceinline__ void clear_list(kp_resource_list& l) {
#pragma unroll
  for (int r = 0; r < CC_R; r++) l.milli[r] = 0;
  l.present = 0;
  l.reserved_ = 0;
}
// ENILimitedPods (R:types.go:461-475)
__device__ __forceinline__ int64_t eni_limited_pods(int max_enis, int ipv4_per_eni, int reserved) {
  const int64_t d = (int64_t)max_enis - reserved, usable = d > 0 ? d : 0;
  return usable == 0 ? 0 : usable * ((int64_t)ipv4_per_eni - 1) + 2;
}
// computeEvictionSignal (R:types.go:571-598) in milli-units
__device__ __forceinline__ int64_t eviction_signal(int64_t capacity_units, const kp_eviction_value& v) {
  if (!v.is_percent) return v.milli;
  const double p = v.percent == 100.0 ? 0.0 : v.percent;
  return (int64_t)ceil((double)capacity_units / 100 * p) * 1000;
}
// MaxResources over the signal maps, one map at a time
__device__ __forceinline__ void fold_signal(kp_resource_list& ov, int r, int64_t capacity_units, const kp_eviction_value& v) {
  if (!v.set) return;
  const int64_t m = eviction_signal(capacity_units, v);
  if (!(ov.present & (1u << r)) || m > ov.milli[r]) set_res(ov, r, m);
}

}  // namespace

__global__ __launch_bounds__(CC_THREADS) void catcomp_resolve_kernel(CatCompArgs a) {
  const int t = blockIdx.x * CC_THREADS + threadIdx.x, n = blockIdx.y;
  if (t >= a.n_types) return;
  const CcNodeClass& nc = a.nodeclasses[n];
  const uint32_t nf = nc.flags, tf = a.type_flags[t];
  const int vcpu = a.vcpu[t], max_enis = a.max_enis[t], ipv4 = a.ipv4_per_eni[t];
  const size_t i = (size_t)n * a.n_types + t;

  // memory() (R:types.go:337-347)
  int64_t mib = a.memory_mib[t];
  if (tf & CC_T_ARM64) mib -= 64;  // Graviton CMA
  const int64_t ov_mib = (int64_t)ceil((double)(mib * kMiB) * a.vm_memory_overhead_percent / 1024 / 1024);
  const int64_t mem_bytes = (mib - ov_mib) * kMiB;
  // pods() (R:types.go:553-569)
  int64_t pods = nc.max_pods >= 0 ? nc.max_pods : (nf & CC_N_ENI_DENSITY) ? eni_limited_pods(max_enis, ipv4, a.reserved_enis) : 110;
  if (nc.pods_per_core > 0 && (nf & CC_N_PODS_PER_CORE)) {
    const int64_t by_core = (int64_t)nc.pods_per_core * vcpu;
    if (by_core < pods) pods = by_core;
  }
  // ephemeralStorage (R:types.go:349-385): RAID0 takes the instance store when the type has one
  const int64_t gb = a.storage_gb[t];
  const int64_t storage = ((nf & CC_N_RAID0) && gb > 0) ? gb * 1000000000ll : nc.storage_bytes;

  kp_resource_list cap;
  clear_list(cap);
  const uint32_t gm = (tf >> CC_T_GPU_SHIFT) & 3u;
  const int64_t gpus = (int64_t)a.gpu_count[t] * 1000;
  const int neuron = a.neuron_devices[t];
  set_res(cap, KP_RES_CPU, (int64_t)vcpu * 1000);
  set_res(cap, KP_RES_MEMORY, mem_bytes * 1000);
  set_res(cap, KP_RES_EPHEMERAL_STORAGE, storage * 1000);
  set_res(cap, KP_RES_PODS, pods * 1000);
  set_res(cap, KP_RES_POD_ENI, ((tf & CC_T_IN_LIMITS) && (tf & CC_T_TRUNKING)) ? (int64_t)a.branch_enis[t] * 1000 : 0);
  set_res(cap, KP_RES_EFA, (int64_t)a.efa[t] * 1000);
  set_res(cap, KP_RES_NVIDIA_GPU, gm == CC_GPU_NVIDIA ? gpus : 0);
  set_res(cap, KP_RES_AMD_GPU, gm == CC_GPU_AMD ? gpus : 0);
  set_res(cap, KP_RES_NEURON, (int64_t)neuron * 1000);
  set_res(cap, KP_RES_NEURONCORE, (int64_t)neuron * a.neuron_cores[t] * 1000);
  set_res(cap, KP_RES_GAUDI, gm == CC_GPU_HABANA ? gpus : 0);
  if ((nf & CC_N_WINDOWS) && (tf & CC_T_AMD64))
    set_res(cap, KP_RES_PRIVATE_IPV4, (tf & CC_T_IN_LIMITS) ? ((int64_t)ipv4 - 1) * 1000 : 0);
  // UpdateInstanceTypeCapacityFromNode (R:instancetype.go:213-215): the capacity alone, the overhead keeps memory()
  if (a.discovered) {
    const int64_t d = a.discovered[i];
    if (d >= 0) cap.milli[KP_RES_MEMORY] = d * 1000;
  }

  // kubeReservedResources (R:types.go:500-533)
  kp_resource_list kube;
  clear_list(kube);
  const int64_t mem_pods = (nf & CC_N_ENI_MEMORY) ? eni_limited_pods(max_enis, ipv4, 0) : pods;
  set_res(kube, KP_RES_MEMORY, (11 * mem_pods + 255) * kMiB * 1000ll);
  set_res(kube, KP_RES_EPHEMERAL_STORAGE, (1ll << 30) * 1000);
  {
    const int64_t cpu_m = (int64_t)vcpu * 1000;
    const int64_t rs[4] = {0, 1000, 2000, 4000}, re[4] = {1000, 2000, 4000, 1ll << 31};
    const double rp[4] = {0.06, 0.01, 0.005, 0.0025};
    int64_t cpu_overhead = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (cpu_m >= rs[k]) cpu_overhead += (int64_t)((double)(cpu_m < re[k] ? cpu_m - rs[k] : re[k] - rs[k]) * rp[k]);
    set_res(kube, KP_RES_CPU, cpu_overhead);
  }
  kp_resource_list sys;
  clear_list(sys);
#pragma unroll
  for (int r = 0; r < CC_R; r++) {
    if (nc.kube_reserved.present & (1u << r)) set_res(kube, r, nc.kube_reserved.milli[r]);
    if (nc.system_reserved.present & (1u << r)) set_res(sys, r, nc.system_reserved.milli[r]);
  }
  // evictionThreshold (R:types.go:535-564)
  kp_resource_list ev;
  clear_list(ev);
  set_res(ev, KP_RES_MEMORY, 100ll * kMiB * 1000ll);
  set_res(ev, KP_RES_EPHEMERAL_STORAGE, (int64_t)ceil((double)storage / 100 * 10) * 1000);
  if (nf & CC_N_KUBELET) {
    kp_resource_list ov;
    clear_list(ov);
    if (nf & CC_N_EVICTION_HARD) {
      fold_signal(ov, KP_RES_MEMORY, mem_bytes, nc.hard_memory);
      fold_signal(ov, KP_RES_EPHEMERAL_STORAGE, storage, nc.hard_nodefs);
    }
    if (nf & CC_N_EVICTION_SOFT) {
      fold_signal(ov, KP_RES_MEMORY, mem_bytes, nc.soft_memory);
      fold_signal(ov, KP_RES_EPHEMERAL_STORAGE, storage, nc.soft_nodefs);
    }
    if (ov.present & (1u << KP_RES_MEMORY)) set_res(ev, KP_RES_MEMORY, ov.milli[KP_RES_MEMORY]);
    if (ov.present & (1u << KP_RES_EPHEMERAL_STORAGE)) set_res(ev, KP_RES_EPHEMERAL_STORAGE, ov.milli[KP_RES_EPHEMERAL_STORAGE]);
  }
  // InstanceTypeOverhead.Total(): resources.Merge of the three lists
  kp_resource_list total;
  clear_list(total);
#pragma unroll
  for (int r = 0; r < CC_R; r++) {
    if (kube.present & (1u << r)) set_res(total, r, total.milli[r] + kube.milli[r]);
    if (sys.present & (1u << r)) set_res(total, r, total.milli[r] + sys.milli[r]);
    if (ev.present & (1u << r)) set_res(total, r, total.milli[r] + ev.milli[r]);
  }
  a.capacity[i] = cap;
  a.overhead[i] = total;
  a.kube_reserved[i] = kube;
  a.system_reserved[i] = sys;
  a.eviction_threshold[i] = ev;
}

// createOfferings' Available per (NodeClass, type, capacity type): bit z = !IsUnavailable && hasPrice && z in itZones
__global__ __launch_bounds__(CC_THREADS) void catcomp_offer_kernel(CatCompArgs a) {
  const int t = blockIdx.x * CC_THREADS + threadIdx.x, n = blockIdx.y;
  if (t >= a.n_types) return;
  const uint64_t itz = a.type_zones[t] & a.nodeclasses[n].zone_mask;
  const bool od_priced = !isnan(a.od_price[t]);
  const uint64_t bit = 1ull << (t & 63);
  const int w = t >> 6;
  uint64_t av[2] = {0, 0};
  for (int z = 0; z < a.n_zones; z++) {
    if (!((itz >> z) & 1) || ((a.ice_zones >> z) & 1)) continue;
    const bool priced[2] = {od_priced, !isnan(a.spot_price[(size_t)t * a.n_zones + z])};
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const bool ice = ((a.ice_capacity_types >> c) & 1) || (a.ice_rows[((size_t)c * a.n_zones + z) * a.words + w] & bit);
      if (!ice && priced[c]) av[c] |= 1ull << z;
    }
  }
  const size_t i = (size_t)n * a.n_types + t;
  a.it_zones[i] = itz;
  a.available[i * 2 + 0] = av[0];
  a.available[i * 2 + 1] = av[1];
}

// the NodeClass-independent price table, a lane per (type, zone), and the reserved offerings, a lane per reservation
__global__ __launch_bounds__(CC_THREADS) void catcomp_price_kernel(CatCompArgs a) {
  const int i = blockIdx.x * CC_THREADS + threadIdx.x;
  if (i < a.n_types * a.n_zones) {
    const double od = a.od_price[i / a.n_zones], spot = a.spot_price[i];
    a.price[(size_t)i * 2 + KP_CT_ON_DEMAND] = isnan(od) ? 0.0 : od + 0.0;  // (-0.0 -> +0.0, as kp_catalog_upload)
    a.price[(size_t)i * 2 + KP_CT_SPOT] = isnan(spot) ? 0.0 : spot + 0.0;
  }
  if (i < a.n_reservations) {
    const CcReservation r = a.reservations[i];
    const uint64_t itz = a.type_zones[r.type] & a.nodeclasses[r.nodeclass].zone_mask;
    const double od = a.od_price[r.type];
    kp_reserved_offering o;
    o.price = isnan(od) ? 0.0 : od / 10000000.0;
    o.available = (r.count != 0 && ((itz >> r.zone) & 1)) ? 1 : 0;
    o.capacity = r.count;
    a.reserved[i] = o;
  }
}

hipError_t launch_catalog_compile(const CatCompArgs& a, hipStream_t s) {
  if (a.n_types > 0 && a.n_nodeclasses > 0) {
    const dim3 grid((a.n_types + CC_THREADS - 1) / CC_THREADS, a.n_nodeclasses);
    hipLaunchKernelGGL(catcomp_resolve_kernel, grid, dim3(CC_THREADS), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(catcomp_offer_kernel, grid, dim3(CC_THREADS), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  const int lanes = a.n_types * a.n_zones > a.n_reservations ? a.n_types * a.n_zones : a.n_reservations;
  if (lanes > 0) {
    hipLaunchKernelGGL(catcomp_price_kernel, dim3((lanes + CC_THREADS - 1) / CC_THREADS), dim3(CC_THREADS), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}
