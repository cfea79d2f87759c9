// kp_ltgroup.hip — kp_launch_templates on the device (gfx950; DESIGN §19, the rule: include/kp/kp_abi.h).
//
//   lt_ami_kernel    MapToInstanceTypes for every catalogue type some request lists, once per call (the map does not
//                    depend on the request). The shape is the opposite of drift_ami_kernel's, thousands of types and a
//                    handful of AMIs, so lanes go over types and the walk over the AMIs' tokens is wave-uniform (scalar
//                    loads); the first AMI that takes a lane's type wins, and a wave stops once every lane has one
//   lt_group_kernel  a wave per request, lanes over the types launch_kernel selected (read where it left them, in the
//                    plan's blob). Each lane packs (AMI, EFA count, max-pods) into 64 bits; groups form by leader
//                    election, one round per group: the lowest unassigned lane broadcasts its key, a ballot finds the
//                    equal keys, they take the next group number. Past 64 types the walk goes in passes of 64 against
//                    the group keys in LDS. Then, per type, the overrides are counted from the offering arrays with the
//                    class sets launch_kernel used, summed per group, the empty groups dropped, the rest numbered by a
//                    wave prefix sum in group order (a group's number is its first member's launch position, so that is
//                    the canonical config order), and the overrides stored. A reserved launch has one config per
//                    (type, reservation of its slice): the slice is recomputed as launch_kernel's rof_pick
// Every word of the output has one writer and there are no atomics.
//
// The requirement algebra (allowed_word, allowed_classes, ...) is kp_kernels.hip's, compiled into this translation unit
// without that file's kernels (KP_TU 0).
#define KP_TU 0
#include "kp_kernels.hip"
#include "kp_ltgroup.h"

static_assert(sizeof(LtOut) == sizeof(kp_lt_result) && sizeof(LtConfig) == sizeof(kp_lt_config), "device mirrors");
static_assert(sizeof(LtOut) == 16 && sizeof(LtConfig) == 32, "records are whole vector stores");

__global__ __launch_bounds__(LT_AMI_THREADS) void lt_ami_kernel(LtArgs a) {
  const int u = blockIdx.x * LT_AMI_THREADS + threadIdx.x;
  const bool live = u < a.n_used;
  const uint32_t t = live ? a.used[u] : 0;
  uint32_t found = DR_NONE;
  for (int i = 0; i < a.n_amis; i++) {
    const bool open = live && found == DR_NONE;
    if (!__ballot(open)) break;
    uint32_t p = a.ami_tok_off[i];
    const uint32_t end = a.ami_tok_off[i + 1];
    bool ok = open;
    while (p < end) {  // (p, hdr and n are wave-uniform)
      const uint32_t hdr = a.ami_tok[p];
      if (hdr == DR_TOK_NEVER) {
        ok = false;
        break;
      }
      const uint32_t n = a.ami_tok[p + 1], key = hdr & DR_TOK_KEY;
      p += 2;
      if (ok) {
        const uint32_t held = a.type_cnt[(size_t)key * a.T + t];
        if (held == DR_NONE) {  // the type does not define the key
          ok = (hdr & DR_TOK_NEGOP) != 0;
        } else {
          const uint64_t* __restrict__ bits = a.type_bits + (size_t)a.tkey_off[key] * a.T + t;
          uint32_t hits = 0;
          for (uint32_t j = 0; j < n; j++) {
            const uint32_t id = a.ami_tok[p + j];
            hits += (uint32_t)((bits[(size_t)(id >> 6) * a.T] >> (id & 63)) & 1);
          }
          const bool meets = (hdr & DR_TOK_KIND) == DR_TOK_ANY ? hits > 0 : held > hits;
          ok = meets || (held == 0 && (hdr & DR_TOK_NEGOP));
        }
      }
      p += n;
    }
    if (ok) found = (uint32_t)i;
  }
  if (live) a.ami_of[t] = found;
}

struct LtWaveLds {
  uint64_t gkey[LAUNCH_CAP];    // per group: its key
  uint32_t g_first[LAUNCH_CAP]; // per group: its overrides, then (kept groups) its first override
  uint32_t pos_off[LAUNCH_CAP]; // per position: overrides of the earlier members of its group
  uint16_t g_nt[LAUNCH_CAP];    // per group: members
  int16_t g_cfg[LAUNCH_CAP];    // per group: config number, -1 dropped
  int16_t pos_grp[LAUNCH_CAP];  // per position: group, -1 no AMI takes the type
  uint16_t pos_cnt[LAUNCH_CAP]; // per position: overrides of the type
};

// Quantity.Value() of a non-negative milli-quantity: rounded up
static __device__ __forceinline__ int64_t lt_value(int64_t milli) { return (milli + 999) / 1000; }

__global__ __launch_bounds__(LT_WAVES * 64) void lt_group_kernel(LtArgs a) {
  __shared__ DevDict D;
  __shared__ LtWaveLds Wl[LT_WAVES];
  const LaunchArgs& la = a.la;
  block_copy(D, la.dict);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = LANE;
  const DevCatalog& Cg = *la.cat;
  LtWaveLds& L = Wl[wave];
  const double INF = __builtin_huge_val();
  const uint64_t below = (1ull << lane) - 1;
  for (long q = (long)blockIdx.x * LT_WAVES + wave; q < la.n; q += (long)gridDim.x * LT_WAVES) {
    const LaunchOut res = la.out[q];
    const uint32_t* __restrict__ sel = la.out_types + (size_t)q * la.max_types;
    int32_t* tc = a.type_config + (size_t)q * la.max_types;
    LtConfig* cf = a.configs + (size_t)q * la.ovr_stride;
    uint32_t* ov = a.overrides + (size_t)q * la.ovr_stride;
    const int cut = res.status == KP_LAUNCH_OK ? (int)res.n_types : 0;
    for (int i = cut + lane; i < la.max_types; i += 64) tc[i] = -1;
    if (res.status != KP_LAUNCH_OK) {
      if (lane == 0) reinterpret_cast<uint4*>(a.lt_out)[q] = make_uint4(KP_LT_SKIPPED, 0u, 0u, 0u);
      continue;
    }
    // the request's compatible offering classes, as launch_kernel forms them
    const KReqs* Q = reinterpret_cast<const KReqs*>(la.q_reqs + (size_t)q * sizeof(KReqs));
    const uint64_t v = lane < D.W ? Q->vals[lane] : 0;
    ReqView rv;
    rv.present = Q->present;
    rv.compl_ = Q->compl_ & Q->present;
    rv.hgt = Q->hgt;
    rv.hlt = Q->hlt;
    rv.hmin = Q->hmin;
    rv.nz = nz_keys(D, v);
    rv.dne = 0;
    rv.gt = Q->gt;
    rv.lt = Q->lt;
    rv.minv = Q->minv;
    const uint64_t negQ = negop_mask(rv.present, rv.compl_, rv.nz);
    const uint64_t allowed = allowed_word(D, rv, v, vint_global(la.vint));
    const uint64_t cls = allowed_classes<true>(D, Cg.cls, rv, allowed, negQ);
    const bool ctw = la.ct_key >= 0 && lane < D.W && D.wkey[lane] == la.ct_key;
    const uint64_t cls_noct = allowed_classes<true>(D, Cg.cls, rv, ctw ? D.validbits[lane] : allowed, negQ);
    const bool reserved = res.capacity_type == 2;
    // The offering slices. Not reserved: the launch filters replaced nothing, or (a capacity block that is not
    // available) left reserved offerings only, and then launch_kernel wrote no override at all. Reserved: the
    // ReservedOfferingFilter ran (a reserved launch needs an available compatible reserved offering, which that filter
    // keeps), over the classes M the two filters before it left: the partition reservation_type names, narrowed to one
    // class when that is capacity-block (CapacityBlockFilter then kept one type, the only one selected).
    const uint64_t res_cand = cls & la.cls_res;
    uint64_t M = ~0ull;
    if (reserved && res.reservation_type == 0) M = la.cls_res & la.cls_rt0;
    if (reserved && res.reservation_type == 1) {
      M = la.cls_res & la.cls_rt1;
      const int t0 = (int)sel[0];
      double p = INF;
      int sc = -1;
      for (int j = 0; j < la.MO; j++) {
        const int c = la.ofs_cls[(size_t)t0 * la.MO + j];
        if (c == 0xFF) break;
        if (!((M >> c) & 1)) continue;
        const double pc = la.price_all[(size_t)t0 * D.C + c];
        if (sc < 0 || pc < p) {
          p = pc;
          sc = c;
        }
      }
      if (sc >= 0) M = 1ull << sc;
    }
    auto rof_pick = [&](int t) -> uint64_t {
      const uint64_t cand = res_cand & M;
      uint64_t pick = 0;
      for (int j = 0; j < la.MO && cand; j++) {
        const int c = la.ofs_cls[(size_t)t * la.MO + j];
        if (c == 0xFF) break;
        if (!((cand >> c) & 1) || !(Cg.price[(size_t)t * D.C + c] < INF)) continue;
        const int z = Cg.cls[c].zone_bit;
        int cur = -1;
        for (uint64_t pp = pick; pp; pp &= pp - 1)
          if (Cg.cls[__builtin_ctzll(pp)].zone_bit == z) {
            cur = __builtin_ctzll(pp);
            break;
          }
        if (cur < 0) pick |= 1ull << c;
        else if (la.rcap[(size_t)t * D.C + c] > la.rcap[(size_t)t * D.C + cur]) pick = (pick & ~(1ull << cur)) | (1ull << c);
      }
      return pick;
    };
    const bool efa_asked = a.req_efa[q] != 0;
    int unmapped = 0, n_cfg = 0, dropped = 0;
    if (reserved) {
      // ---- one config per (type, reservation of its slice), one override each ----------------------------------
      for (int base = 0; base < cut; base += 64) {
        const int i = base + lane;
        int t = 0, kept = 0, lost = 0;
        uint32_t ami = DR_NONE;
        uint64_t pick = 0;
        if (i < cut) {
          t = (int)sel[i];
          ami = a.ami_of[t];
          if (ami != DR_NONE) {
            pick = rof_pick(t);
            for (uint64_t pp = pick; pp; pp &= pp - 1)
              if (la.cls_zone[__builtin_ctzll(pp)] >= 0) kept++;
              else lost++;
          }
        }
        unmapped += __builtin_popcountll(__ballot(i < cut && ami == DR_NONE));
        int incl = kept;  // inclusive wave scan
        for (int o = 1; o < 64; o <<= 1) {
          const int y = __shfl_up(incl, o, 64);
          if (lane >= o) incl += y;
        }
        int pos = n_cfg + incl - kept;
        if (i < cut) {
          tc[i] = kept ? pos : -1;
          const int32_t pods = (int32_t)lt_value(Cg.cap[(size_t)KP_RES_PODS * D.T + t]);
          const int32_t efa = efa_asked ? (int32_t)lt_value(Cg.cap[(size_t)KP_RES_EFA * D.T + t]) : 0;
          for (int j = 0; j < la.MO && kept; j++) {  // offering order
            const int c = la.ofs_cls[(size_t)t * la.MO + j];
            if (c == 0xFF) break;
            if (!((pick >> c) & 1) || la.cls_zone[c] < 0 || pos >= (int)la.ovr_stride) continue;
            const int32_t rt = ((la.cls_rt0 >> c) & 1) ? 0 : ((la.cls_rt1 >> c) & 1) ? 1 : -1;
            uint4* rec = reinterpret_cast<uint4*>(cf + pos);
            rec[0] = make_uint4(ami, (uint32_t)pods, (uint32_t)efa, (uint32_t)j);
            rec[1] = make_uint4((uint32_t)rt, (uint32_t)pos, 1u, 1u);
            ov[pos] = ((uint32_t)t << 8) | (uint32_t)la.cls_zone[c];
            pos++;
          }
        }
        n_cfg += __shfl(incl, 63, 64);
        for (int o = 32; o >= 1; o >>= 1) lost += __shfl_xor(lost, o, 64);
        dropped += lost;
      }
    } else {
      // ---- groups by leader election; per position its group and its override count ------------------------------
      const uint64_t c3 = res.n_overrides ? cls_noct & (res.capacity_type == 1 ? la.cls_spot : la.cls_od) : 0;
      int ng = 0;
      for (int base = 0; base < cut; base += 64) {
        const int i = base + lane;
        uint64_t key = 0;
        bool mapped = false;
        int cnt = 0;
        if (i < cut) {
          const int t = (int)sel[i];
          const uint32_t ami = a.ami_of[t];
          mapped = ami != DR_NONE;
          const uint64_t pods = (uint64_t)lt_value(Cg.cap[(size_t)KP_RES_PODS * D.T + t]);
          const uint64_t efa = efa_asked ? (uint64_t)lt_value(Cg.cap[(size_t)KP_RES_EFA * D.T + t]) : 0;
          key = ((uint64_t)ami << 48) | (efa << 32) | pods;
          for (int j = 0; j < la.MO && mapped; j++) {
            const int c = la.ofs_cls[(size_t)t * la.MO + j];
            if (c == 0xFF) break;
            if (((c3 >> c) & 1) && Cg.price[(size_t)t * D.C + c] < INF && la.cls_zone[c] >= 0) cnt++;
          }
        }
        unmapped += __builtin_popcountll(__ballot(i < cut && !mapped));
        int grp = -1;
        for (int g = 0; g < ng; g++)  // the groups of earlier passes
          if (mapped && grp < 0 && L.gkey[g] == key) grp = g;
        uint64_t pending = __ballot(mapped && grp < 0);
        while (pending) {  // one round per new group
          const int leader = __builtin_ctzll(pending);
          const uint64_t k = lane_bcast(key, leader);
          const uint64_t eq = __ballot(mapped && grp < 0 && key == k);
          if ((eq >> lane) & 1) grp = ng;
          if (lane == leader) L.gkey[ng] = k;
          ng++;
          pending &= ~eq;
        }
        if (i < cut) {
          L.pos_grp[i] = (int16_t)grp;
          L.pos_cnt[i] = (uint16_t)cnt;
        }
        wave_sync();
      }
      // ---- per position the overrides of the earlier members of its group; the last member writes the group's totals
      for (int base = 0; base < cut; base += 64) {
        const int i = base + lane;
        const int grp = i < cut ? L.pos_grp[i] : -1;
        uint32_t off = 0, before = 0;
        bool later = false;
        for (int j = 0; j < cut; j++) {
          const bool same = grp >= 0 && L.pos_grp[j] == grp;
          if (same && j < i) off += L.pos_cnt[j], before++;
          if (same && j > i) later = true;
        }
        if (i < cut) L.pos_off[i] = off;
        if (grp >= 0 && !later) {
          L.g_first[grp] = off + L.pos_cnt[i];
          L.g_nt[grp] = (uint16_t)(before + 1);
        }
      }
      wave_sync();
      // ---- drop the groups without overrides, number the rest in group order, write their records ----------------
      int novr = 0;
      for (int base = 0; base < ng; base += 64) {
        const int g = base + lane;
        const uint32_t tot = g < ng ? L.g_first[g] : 0;
        const bool keep = tot > 0;
        const uint64_t bal = __ballot(keep);
        int incl = (int)tot;
        for (int o = 1; o < 64; o <<= 1) {
          const int y = __shfl_up(incl, o, 64);
          if (lane >= o) incl += y;
        }
        const int cfg = n_cfg + __builtin_popcountll(bal & below);
        const uint32_t first = (uint32_t)(novr + incl) - tot;
        if (g < ng) {
          L.g_cfg[g] = keep ? (int16_t)cfg : (int16_t)-1;
          L.g_first[g] = first;
        }
        if (keep) {
          const uint64_t k = L.gkey[g];
          uint4* rec = reinterpret_cast<uint4*>(cf + cfg);
          rec[0] = make_uint4((uint32_t)(k >> 48), (uint32_t)k, (uint32_t)(k >> 32) & 0xFFFFu, 0xFFFFFFFFu);
          rec[1] = make_uint4(0xFFFFFFFFu, first, tot, (uint32_t)L.g_nt[g]);
        }
        n_cfg += __builtin_popcountll(bal);
        novr += __shfl(incl, 63, 64);
        dropped += __builtin_popcountll(__ballot(g < ng && !keep));
      }
      wave_sync();
      // ---- each type's config and its overrides, in the type's offering order --------------------------------------
      for (int i = lane; i < cut; i += 64) {
        const int grp = L.pos_grp[i];
        const int cfg = grp >= 0 ? L.g_cfg[grp] : -1;
        tc[i] = cfg;
        if (cfg < 0) continue;
        const int t = (int)sel[i];
        uint32_t pos = L.g_first[grp] + L.pos_off[i];
        for (int j = 0; j < la.MO; j++) {
          const int c = la.ofs_cls[(size_t)t * la.MO + j];
          if (c == 0xFF) break;
          if (((c3 >> c) & 1) && Cg.price[(size_t)t * D.C + c] < INF && la.cls_zone[c] >= 0 && pos < la.ovr_stride)
            ov[pos++] = ((uint32_t)t << 8) | (uint32_t)la.cls_zone[c];
        }
      }
    }
    if (lane == 0) {
      const int32_t status = a.n_amis == 0        ? KP_LT_NO_AMIS
                             : unmapped == cut    ? KP_LT_NO_COMPATIBLE_AMI
                             : n_cfg == 0         ? KP_LT_NO_OFFERINGS
                                                  : KP_LT_OK;
      reinterpret_cast<uint4*>(a.lt_out)[q] = make_uint4((uint32_t)status, (uint32_t)n_cfg, (uint32_t)unmapped, (uint32_t)dropped);
    }
    wave_sync();  // (the next request rewrites this wave's LDS rows)
  }
}

hipError_t launch_lt(const LtArgs& a, hipStream_t s) {
  if (a.n_used > 0 && a.n_amis > 0) {
    hipLaunchKernelGGL(lt_ami_kernel, dim3((a.n_used + LT_AMI_THREADS - 1) / LT_AMI_THREADS), dim3(LT_AMI_THREADS), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  long blocks = ((long)a.la.n + LT_WAVES - 1) / LT_WAVES;
  if (blocks > 65536) blocks = 65536;
  if (blocks < 1) return hipSuccess;
  hipLaunchKernelGGL(lt_group_kernel, dim3((unsigned)blocks), dim3(LT_WAVES * 64), 0, s, a);
  return hipGetLastError();
}
