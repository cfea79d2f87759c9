// kp_catcomp.h — device data model of kp_catalog_compile (kp_catcomp.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kp/kp_abi.h"

// Strings never reach the device. A type's architecture and limits-table facts are bits of type_flags, its GPU
// manufacturer two more; a zone is its index in all_zones; a NodeClass is one fixed-width record. The unavailable
// offerings are one bit row over the types per (capacity type, zone), plus the capacity types and the zones that
// are unavailable as a whole.
#define CC_T_ARM64 0x1u
#define CC_T_AMD64 0x2u
#define CC_T_IN_LIMITS 0x4u
#define CC_T_TRUNKING 0x8u
#define CC_T_GPU_SHIFT 4  // two bits: CC_GPU_*
#define CC_GPU_NONE 0u
#define CC_GPU_NVIDIA 1u
#define CC_GPU_AMD 2u
#define CC_GPU_HABANA 3u

// the AMI family's FeatureFlags, the instance-store policy and which eviction maps count
#define CC_N_ENI_MEMORY 0x1u     // UsesENILimitedMemoryOverhead
#define CC_N_PODS_PER_CORE 0x2u  // PodsPerCoreEnabled
#define CC_N_ENI_DENSITY 0x4u    // SupportsENILimitedPodDensity
#define CC_N_WINDOWS 0x8u
#define CC_N_RAID0 0x10u
#define CC_N_KUBELET 0x20u       // the NodeClass has a kubelet block
#define CC_N_EVICTION_HARD 0x40u // evictionHard is not nil
#define CC_N_EVICTION_SOFT 0x80u // evictionSoft is not nil and the family honours it (EvictionSoftEnabled)

#define CC_THREADS 256

struct CcNodeClass {
  kp_resource_list kube_reserved, system_reserved;  // the user's keys (present = 0 without a kubelet block)
  kp_eviction_value hard_memory, hard_nodefs, soft_memory, soft_nodefs;
  int64_t storage_bytes;  // ephemeralStorage without RAID0: the block-device mappings resolved on the host
  uint64_t zone_mask;     // the subnet zones, as bits over all_zones
  int32_t max_pods;       // < 0: nil
  int32_t pods_per_core;  // <= 0: nil
  uint32_t flags;         // CC_N_*
  uint32_t reserved;
};

struct CcReservation {
  uint32_t nodeclass, type, zone;
  int32_t count;
};

struct CatCompArgs {
  int n_types, n_nodeclasses, n_zones, n_reservations;
  int words;  // ceil(n_types / 64): the length of an unavailable-offerings bit row
  double vm_memory_overhead_percent;
  int reserved_enis;
  // types, structure of arrays, [n_types] each
  const int32_t* vcpu;
  const int64_t* memory_mib;
  const uint32_t* type_flags;
  const int32_t* gpu_count;
  const int32_t* neuron_devices;
  const int32_t* neuron_cores;
  const int32_t* efa;
  const int32_t* max_enis;
  const int32_t* ipv4_per_eni;
  const int32_t* branch_enis;
  const int64_t* storage_gb;  // InstanceStorageInfo.TotalSizeInGB, else the local NVMe size; 0: no instance store
  const uint64_t* type_zones;
  const double* od_price;
  const double* spot_price;   // [n_types][n_zones]
  const CcNodeClass* nodeclasses;
  const int64_t* discovered;  // [n_nodeclasses][n_types], or null
  // unavailable offerings
  const uint64_t* ice_rows;   // [2][n_zones][words]
  uint64_t ice_zones;         // zones unavailable as a whole
  uint32_t ice_capacity_types;  // bit c: capacity type c unavailable as a whole
  const CcReservation* reservations;
  // outputs
  kp_resource_list *capacity, *overhead, *kube_reserved, *system_reserved, *eviction_threshold;  // [n_nodeclasses][n_types]
  uint64_t* it_zones;         // [n_nodeclasses][n_types]
  uint64_t* available;        // [n_nodeclasses][n_types][2]
  double* price;              // [n_types][n_zones][2]
  kp_reserved_offering* reserved;  // [n_reservations]
};

// the three kernels on stream s; nothing is synchronised
hipError_t launch_catalog_compile(const CatCompArgs& a, hipStream_t s);
