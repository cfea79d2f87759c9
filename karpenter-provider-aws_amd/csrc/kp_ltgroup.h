// kp_ltgroup.h — device data model of kp_launch_templates (kp_ltgroup.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kp_device.h"
#include "kp_driftdet.h"  // the AMI token format (DR_TOK_*), DR_NONE

#define LT_WAVES 2         // waves per block of the grouping kernel: a request's working set is LtWaveLds, 24 KB of LDS
#define LT_AMI_THREADS 256
#define LT_MAX_AMIS 65535  // the group key holds the AMI index in 16 bits

struct LtOut {     // kp_lt_result as the device writes it
  int32_t status;
  uint32_t n_configs, n_unmapped, n_dropped;
};
struct LtConfig {  // kp_lt_config as the device writes it
  int32_t ami, max_pods, efa_count, reservation_offering, reservation_type;
  uint32_t first_override, n_overrides, n_types;
};

struct LtArgs {
  LaunchArgs la;  // the launch plan's arguments: its requests, catalogue, offering tables and the selection
                  // launch_kernel left in la.out / la.out_types
  // resident per plan: the requirement rows of the catalogue's types, key-major and word-major (lane = type: a wave
  // reads 64 consecutive types of a row in one coalesced load)
  const uint32_t* type_cnt;   // [n_tkeys][T] how many values the type holds under the key, DR_NONE: key undefined
  const uint64_t* type_bits;  // [type_words][T] those values, key k's words from tkey_off[k]
  const uint32_t* tkey_off;   // [n_tkeys]
  const uint32_t* used;       // [n_used] the catalogue types some request lists, ascending
  const uint8_t* req_efa;     // [n] 1: the request's resource list carries vpc.amazonaws.com/efa
  int32_t T, n_tkeys, type_words, n_used;
  // per call
  const uint32_t* ami_tok_off;  // [n_amis + 1]
  const uint32_t* ami_tok;      // kp_driftdet.h's tokens over this table's dictionary
  int32_t n_amis, pad_;
  uint32_t* ami_of;             // [T] index of the type's AMI, DR_NONE: no AMI takes it (written for used types)
  // outputs (la.ovr_stride = max_types * max(1, subnet zones) entries per request)
  LtOut* lt_out;                // [n]
  int32_t* type_config;         // [n][max_types]
  LtConfig* configs;            // [n][ovr_stride]
  uint32_t* overrides;          // [n][ovr_stride]
};

// lt_ami_kernel, then lt_group_kernel, on stream s after launch_kernel; nothing is synchronised
hipError_t launch_lt(const LtArgs& a, hipStream_t s);
