// kp_sim.hip — batched consolidation simulations (included by kp_kernels.hip; shares its wave helpers).
//
// Upstream disruption computeConsolidation(S) runs SimulateScheduling = Solve(pods of S, existing nodes =
// every node not in S) and turns the Results into delete / replace / no-op (SURVEY §3 CS3, §8a a19;
// R:website/content/en/preview/concepts/disruption.md:89-128). Thousands of subsets S probe the SAME
// cluster snapshot, so the snapshot is resident and each simulation is an overlay on it:
//
//  sim_usable_kernel  per shape-level sl: the existing nodes whose ExistingNode.CanAdd succeeds on the
//                     snapshot (taints, Requirements.Compatible without the well-known allowance, Fits).
//                     Node labels are single-valued In requirements, so Compatible is one dictionary-bit
//                     test per pod key (lane = node, ballot -> 64-node word).
//  sim_prep_kernel    per shape-level: the addToNewNodeClaim outcome (first NodeClaimTemplate whose Add
//                     succeeds, and the NodeClaim it creates), before the NodePool limits; sim_kernel applies
//                     filterByRemainingResources on the replacement against the pools' remaining budget.
//  sim_kernel         one WAVE per simulation, persistent over the batch. Per simulation: exclusion bitmap
//                     of S and a "touched" bitmap in LDS, the pods of S sorted into Queue order (bitonic
//                     sort of their global queue ranks in LDS), then the Solve loop:
//                       existing nodes  first set bit of usable[sl] & ~excluded at or after start[sl];
//                                       touched nodes re-check Fits against their overlay requests.
//                                       Nodes only lose capacity, so every position before the last
//                                       winner stays a failure for sl: start[sl] is monotone.
//                       in-flight       the single NodeClaim: merge_compatible + filter_types (exact, as
//                                       in solve_kernel), failure memo per (sl, NodeClaim version)
//                       new NodeClaim   the precomputed template outcome; a second NodeClaim makes the
//                                       result a no-op, so the simulation stops there.
//                     then the decision: TruncateInstanceTypes (cheapest compatible offering, name; LDS
//                     bitonic sort) + minValues, filterByPrice on WorstLaunchPrice, filterOutSameType.
//  budget_gate_kernel NodePool disruption budgets (kp_*_budgeted), before sim_kernel: per subset the members per owning
//                     NodePool against allowed[]; the admissible subsets' ascending index list (gate_scan_kernel,
//                     gate_scatter_kernel) is what the gated sim_kernel instantiation walks (end of this file).
//
// The host routes the clusters these kernels do not model to the general path (each subset a whole device Solve,
// batched one workgroup per subset on the cluster's superset Solve: kp_host.cpp GeneralBatch): topology spread and pod (anti-)affinity, a pod NotIn/DoesNotExist requirement on a
// key some node lacks (ExistingNode requirements could then grow a key, and CanAdd would no longer be a function of
// the snapshot), and catalogues holding capacity reservations (strict reservation accounting).

__device__ __forceinline__ void sim_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}
__device__ __forceinline__ double lane_bcast_f64(double v, int src) {
  return __longlong_as_double((long long)lane_bcast((uint64_t)__double_as_longlong(v), src));
}

// ReqView of a stored requirement set (final NodeClaim requirements, pod requirements)
__device__ __forceinline__ ReqView stored_view(const DevDict& D, const KReqs* R, uint64_t v) {
  ReqView rv;
  rv.present = R->present;
  rv.compl_ = R->compl_ & R->present;
  rv.hgt = R->hgt;
  rv.hlt = R->hlt;
  rv.hmin = R->hmin;
  rv.nz = nz_keys(D, v);
  rv.dne = 0;
  rv.gt = R->gt;
  rv.lt = R->lt;
  rv.minv = R->minv;
  return rv;
}

// stage one shape-level (requirements, requests, PVP slots) into this wave's LDS
__device__ __forceinline__ void stage_shape(const SimArgs& a, int sl, int shape, KReqs* sB, int64_t* spreq,
                                            int32_t* spslot) {
  const int lane = LANE;
  const uint64_t* src = reinterpret_cast<const uint64_t*>(a.shape_reqs + (size_t)sl * sizeof(KReqs));
  uint64_t* dst = reinterpret_cast<uint64_t*>(sB);
  constexpr int NQ = (int)(sizeof(KReqs) / 8);
  for (int i = lane; i < NQ; i += 64) dst[i] = src[i];
  if (lane < KP_NRES) spreq[lane] = a.shape_requests[(size_t)shape * KP_NRES + lane];
  spslot[lane] = a.pvp_slot[(size_t)sl * KP_MAX_KEYS + lane];
}

// wave-wide bitonic sort of n2 (power of two) u32 keys in LDS, ascending
__device__ void wave_bitonic_u32(uint32_t* k, int n2) {
  const int lane = LANE;
  for (int sz = 2; sz <= n2; sz <<= 1)
    for (int j = sz >> 1; j > 0; j >>= 1) {
      for (int i = lane; i < n2; i += 64) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint32_t x = k[i], y = k[ixj];
          if ((x > y) == ((i & sz) == 0)) {
            k[i] = y;
            k[ixj] = x;
          }
        }
      }
      wave_sync();
    }
}
// same for (u64 key, u32 tie) pairs
__device__ void wave_bitonic_kv(uint64_t* k, uint32_t* v, int n2) {
  const int lane = LANE;
  for (int sz = 2; sz <= n2; sz <<= 1)
    for (int j = sz >> 1; j > 0; j >>= 1) {
      for (int i = lane; i < n2; i += 64) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint64_t ki = k[i], kj = k[ixj];
          const uint32_t vi = v[i], vj = v[ixj];
          const bool gt = ki > kj || (ki == kj && vi > vj);
          if (gt == ((i & sz) == 0)) {
            k[i] = kj;
            k[ixj] = ki;
            v[i] = vj;
            v[ixj] = vi;
          }
        }
      }
      wave_sync();
    }
}

// ------------------------------------------------------------------------------------------------
// usable[sl][w]: ExistingNode.CanAdd on the snapshot for the 64 nodes of word w
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SIM_WAVES * 64) void sim_usable_kernel(SimArgs a) {
  __shared__ DevDict D;
  __shared__ uint64_t s_allow[SIM_WAVES][KP_MAX_WORDS];
  block_copy(D, a.dict);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = LANE;
  const long items = (long)a.SL * a.EW;
  for (long it = (long)blockIdx.x * SIM_WAVES + wave; it < items; it += (long)gridDim.x * SIM_WAVES) {
    const int sl = (int)(it / a.EW), w = (int)(it % a.EW);
    const int shape = a.sl_shape[sl];
    const KReqs* B = reinterpret_cast<const KReqs*>(a.shape_reqs + (size_t)sl * sizeof(KReqs));
    const uint64_t v = lane < D.W ? B->vals[lane] : 0;
    const ReqView rv = stored_view(D, B, v);
    s_allow[wave][lane] = allowed_word(D, rv, v, vint_global(a.vint));
    wave_sync();
    const uint64_t negB = a.shape_negop[sl];
    const uint64_t tol = a.shape_tolerates[sl];
    const int e = w * 64 + lane;
    bool ok = e < a.E;
    if (ok) ok = (tol >> a.ex_taintset[e]) & 1;
    if (ok && a.hp_any) ok = !(a.ex_hp[e] & a.shape_hp_conf[shape]);  // HostPortUsage.Conflicts
    for (int r = 0; r < KP_NRES && ok; r++) {  // Fits(Merge(requests, pod), available)
      const int64_t av = a.ex_available[(size_t)e * KP_NRES + r];
      ok = av >= 0 && a.ex_requests[(size_t)e * KP_NRES + r] + a.shape_requests[(size_t)shape * KP_NRES + r] <= av;
    }
    uint64_t keys = B->present;
    while (ok && keys) {  // Requirements.Compatible(node labels, pod) without the well-known allowance
      const int k = __builtin_ctzll(keys);
      keys &= keys - 1;
      const uint16_t code = a.ex_code[(size_t)k * a.E + e];
      if (code == 0xFFFF) ok = (negB >> k) & 1;  // undefined on the node: only NotIn / DoesNotExist
      else ok = (s_allow[wave][code >> 6] >> (code & 63)) & 1;  // In{label} ∩ pod requirement non-empty
    }
    const uint64_t bal = __ballot(ok);
    if (lane == 0) a.usable[(size_t)sl * a.EW + w] = bal;
    wave_sync();
  }
}

// ------------------------------------------------------------------------------------------------
// tres[sl]: addToNewNodeClaim for a pod of shape-level sl (templates in weight order, first success)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void copy_u64(uint64_t* dst, const uint64_t* src, int n) {
  for (int i = LANE; i < n; i += 64) dst[i] = src[i];
}

__global__ __launch_bounds__(SIM_WAVES * 64) void sim_prep_kernel(SimArgs a) {
  __shared__ DevDict D;
  __shared__ WaveSlots slots[SIM_WAVES];
  __shared__ KReqs s_B[SIM_WAVES];
  __shared__ int64_t s_preq[SIM_WAVES][KP_NRES];
  __shared__ int32_t s_pslot[SIM_WAVES][KP_MAX_KEYS];
  __shared__ uint32_t s_scratch[SIM_WAVES][2 * KP_MAX_WORDS];
  __shared__ int32_t s_fitj[SIM_WAVES][KP_NRES];
  __shared__ RowPtr s_rl[SIM_WAVES][RL_CAP];
  __shared__ CatHdr s_hdr[8];
  __shared__ CatHdr s_hdrw[SIM_WAVES];
  block_copy(D, a.dict);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = LANE;
  for (int c = wave; c < min(a.n_catalogs, 8); c += SIM_WAVES) hdr_fill_wave((CatHdr LDS*)&s_hdr[c], &a.cats[c], D.C);
  __syncthreads();
  auto hdr = [&](int c) -> const CatHdr LDS* {
    if (c < 8) return (const CatHdr LDS*)&s_hdr[c];
    hdr_fill_wave((CatHdr LDS*)&s_hdrw[wave], &a.cats[c], D.C);
    wave_sync();
    return (const CatHdr LDS*)&s_hdrw[wave];
  };
  uint64_t bytes = 0;
  for (int sl = blockIdx.x * SIM_WAVES + wave; sl < a.SL; sl += gridDim.x * SIM_WAVES) {
    const int shape = a.sl_shape[sl];
    stage_shape(a, sl, shape, &s_B[wave], s_preq[wave], s_pslot[wave]);
    wave_sync();
    SimNC* out = &a.tres[sl];
    const uint64_t negB = a.shape_negop[sl];
    const uint64_t tol = a.shape_tolerates[sl];
    int won = -1;
    for (int t = 0; t < a.n_tmpl && won < 0; t++) {
      if (!((tol >> a.tmpl_taintset[t]) & 1)) continue;
      const int cat = a.tmpl_catalog[t];
      uint64_t X = lane < D.TW ? a.tmpl_X[(size_t)t * D.TW + lane] : 0;
      const uint32_t lim = a.tmpl_limit_present[t];
      if (lim) {  // filterByRemainingResources: every limited resource's capacity within the NodePool's remaining
        const int64_t* rem = a.tmpl_remaining + (size_t)t * KP_NRES;
        const int64_t* capv = a.cats[cat].cap;
        uint64_t m = X, keep = 0;
        while (m) {
          const int b = __builtin_ctzll(m);
          m &= m - 1;
          const int ty = lane * 64 + b;
          bool viable = true;
          for (int r = 0; r < KP_NRES; r++)
            if (((lim >> r) & 1) && capv[(size_t)r * D.T + ty] > rem[r]) viable = false;
          if (viable) keep |= 1ull << b;
        }
        X = keep;
      }
      if (!__ballot(X != 0)) continue;
      uint64_t m_v = 0;
      ReqView rv;
      bool ok = merge_compatible(D, reinterpret_cast<const KReqs*>(a.tmpl_reqs + (size_t)t * sizeof(KReqs)), &s_B[wave],
                                 negB, true, m_v, rv, &slots[wave], vint_global(a.vint));
      if (ok) {
        const uint64_t* pvp = a.shape_pvp + (size_t)a.pvp_base[sl * a.n_catalogs + cat] * D.TW;
        const int64_t q_lane = lane < KP_NRES ? a.tmpl_daemon[(size_t)t * KP_NRES + lane] + s_preq[wave][lane] : 0;
        X = filter_types(D, hdr(cat), rv, m_v, X, s_B[wave].present, pvp, s_pslot[wave], q_lane, 0, nullptr,
                         a.req_res_mask, vint_global(a.vint), s_scratch[wave], (RowPtr LDS*)s_rl[wave], &bytes, s_fitj[wave]);
        ok = __ballot(X != 0) != 0;
      }
      if (ok) {
        store_merged(&out->reqs, rv, m_v, D.W, D.KB);
        if (lane < KP_MAX_TYPE_WORDS) out->X[lane] = lane < D.TW ? X : 0;
        if (lane < KP_NRES) {
          out->requests[lane] = a.tmpl_daemon[(size_t)t * KP_NRES + lane] + s_preq[wave][lane];
          out->fitj[lane] = s_fitj[wave][lane];
          out->maxalloc[lane] = INT64_MAX;
        }
        wave_sync();
        store_maxalloc(a.cats[cat].alloc, lane < D.TW ? X : 0, D.T, a.req_res_mask, out->maxalloc);
        if (lane == 0) {
          out->tmpl = t;
          out->taintset = a.tmpl_taintset[t];
          out->ver = 0;
          out->hp = a.hp_any ? a.shape_hp_add[shape] : 0;
        }
        won = t;
      }
      wave_sync();
    }
    if (won < 0 && lane == 0) out->tmpl = -1;
    wave_sync();
  }
}

// ------------------------------------------------------------------------------------------------
// sim_kernel: one wave per simulation
// ------------------------------------------------------------------------------------------------
#ifndef SIM_WPE
#define SIM_WPE 0  // waves per SIMD the register allocation targets (0: the compiler's choice; tools/kp_diag.h)
#endif
#if SIM_WPE
#define SIM_OCCUPANCY __attribute__((amdgpu_waves_per_eu(SIM_WPE, SIM_WPE)))
#else
#define SIM_OCCUPANCY
#endif
// GL = SimLive is the gated instantiation (kp_*_budgeted): a.n_subsets counts the admissible subsets and the k-th
// simulation is subset gl.live[k] (ascending: budget_gate_kernel). GL = SimAll walks every subset; its conditionals on
// GL::gated fold away before code generation, so that instantiation compiles as it did without the gate.
// GL = SimCheck (kp_cluster_validate) is gated too and takes no decision: every statement of its own sits under
// GL::check, which is false in the three other policies, so those are generated from the code they had.
// GL = SimWhy (kp_cluster_simulate_explained) is gated, decides as SimLive decides and also says which exit a no-op
// took (kp_abi.h's order): every statement of its own sits under GL::why, false in the four other policies. It runs a
// simulation to its end as SimCheck does, truncates before it looks at the prices and the spot-to-spot gate (the other
// deciding policies test the gate first: both are no-ops there), and the price stages then run only for a simulation
// SimLive would have taken that far.
template <int NW, class GL>
__global__ __launch_bounds__(NW * 64) SIM_OCCUPANCY void sim_kernel(SimArgs a, GL gl) {
  __shared__ DevDict D;
  __shared__ WaveSlots slots[NW];
  __shared__ KReqs s_B[NW];
  __shared__ int64_t s_preq[NW][KP_NRES];
  __shared__ int32_t s_pslot[NW][KP_MAX_KEYS];
  __shared__ uint32_t s_scratch[NW][2 * KP_MAX_WORDS];
  __shared__ uint64_t s_mask[NW][KP_MAX_TYPE_WORDS];
  __shared__ int32_t s_fitj[NW][KP_NRES];
  __shared__ RowPtr s_rl[NW][RL_CAP];
  __shared__ CatHdr s_hdr[8];
  __shared__ CatHdr s_hdrw[NW];
  extern __shared__ uint64_t s_dyn64[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = LANE;
  block_copy(D, a.dict);
  __syncthreads();
  for (int c = wave; c < min(a.n_catalogs, 8); c += NW) hdr_fill_wave((CatHdr LDS*)&s_hdr[c], &a.cats[c], D.C);
  __syncthreads();
  auto hdr = [&](int c) -> const CatHdr LDS* {
    if (c < 8) return (const CatHdr LDS*)&s_hdr[c];
    hdr_fill_wave((CatHdr LDS*)&s_hdrw[wave], &a.cats[c], D.C);
    wave_sync();
    return (const CatHdr LDS*)&s_hdrw[wave];
  };
  const int EW = a.EW, SL = a.SL, cap = a.cap;
  uint8_t* wbase = reinterpret_cast<uint8_t*>(s_dyn64) + (size_t)wave * a.wave_lds;
  uint64_t* excl = reinterpret_cast<uint64_t*>(wbase);
  uint64_t* dirty = excl + EW;
  uint32_t* keys = reinterpret_cast<uint32_t*>(dirty + EW);
  uint16_t* ring = reinterpret_cast<uint16_t*>(keys + a.cap2);
  uint64_t* fkey = dirty + EW;                                   // option sort (after the pod loop)
  uint32_t* fidx = reinterpret_cast<uint32_t*>(fkey + a.cap2 / 2);
  const int slot = blockIdx.x * NW + wave;
  uint64_t* spod = a.s_pod + (size_t)slot * cap;
  int32_t* sstart = a.s_start + (size_t)slot * SL;
  int64_t* ovl = a.s_ovl + (size_t)slot * a.E * a.RU;
  uint64_t* ovlhp = a.hp_any ? a.s_ovlhp + (size_t)slot * a.E : nullptr;
  SimNC* nc = a.s_nc + slot;
  int32_t* ncfail = a.s_ncfail + (size_t)slot * SL;
  KReqs* sB = &s_B[wave];
  int64_t* spreq = s_preq[wave];
  uint64_t attempts = 0, bytes = 0, pops = 0, words = 0;
  int32_t vcount = 0;
  const uint32_t rmask = a.req_res_mask;

  bool cancelled = false;
  for (int sim = slot, it = 0; sim < a.n_subsets; sim += a.n_slots, it++) {
    // kp_cancel (consolidation timeouts): the flag every 8 subsets of this wave; a set flag ends the wave's share
    if ((it & 7) == 0 && cancel_set(a.cancel)) {
      cancelled = true;
      break;
    }
    const uint32_t s0 = a.sub_off[GL::gated ? (int)gl.live[sim] : sim];
    const int ns = (int)(a.sub_off[(GL::gated ? (int)gl.live[sim] : sim) + 1] - s0);
    for (int w = lane; w < EW; w += 64) {
      excl[w] = a.base_excl[w];  // deleting nodes are never destinations
      dirty[w] = 0;
    }
    for (int i = lane; i < a.n_base; i += 64) keys[i] = a.base_keys[i];  // pending + deleting-node pods
    wave_sync();
    // ---- exclusions, candidate prices, pods of S ------------------------------------------------
    for (int i = lane; i < ns; i += 64) {
      const int pos = a.node_pos[a.sub_nodes[s0 + i]];
      atomicOr((unsigned long long*)&excl[pos >> 6], 1ull << (pos & 63));
    }
    int n = a.n_base;
    bool overflow = false;
    for (int i0 = 0; i0 < ns; i0 += 64) {
      const int i = i0 + lane;
      uint32_t off = 0;
      int cnt = 0;
      if (i < ns) {
        const uint32_t c = a.sub_nodes[s0 + i];
        off = a.node_pod_off[c];
        cnt = (int)(a.node_pod_off[c + 1] - off);
      }
      int incl = cnt;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
      }
      const int total = __shfl(incl, 63, 64);
      if (n + total > cap) {
        overflow = true;
        break;
      }
      const int at = n + incl - cnt;
      for (int j = 0; j < cnt; j++) keys[at + j] = a.pod_rank[a.node_pods[off + j]];
      n += total;
    }
    double candPrice = 0;
    int flags_and = 3;
    int w_unpriced = -1;  // GL::why: the first candidate without a label-compatible offering (position in S)
    if (lane == 0) {  // getCandidatePrices: summed in candidate order (float addition order matters)
      for (int i = 0; i < ns; i++) {
        const uint32_t c = a.sub_nodes[s0 + i];
        candPrice += a.node_price[c];
        flags_and &= a.node_flags[c];
        if constexpr (GL::why) {
          if (w_unpriced < 0 && !(a.node_flags[c] & 1)) w_unpriced = i;
        }
      }
    }
    candPrice = lane_bcast_f64(candPrice, 0);
    flags_and = __builtin_amdgcn_readlane(flags_and, 0);
    if constexpr (GL::why) w_unpriced = __builtin_amdgcn_readlane(w_unpriced, 0);
    const bool priced = flags_and & 1, allSpot = (flags_and >> 1) & 1;
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = n + lane; i < n2; i += 64) keys[i] = 0xFFFFFFFFu;
    wave_sync();
    wave_bitonic_u32(keys, n2);  // Queue order byCPUAndMemoryDescending over the pods of S
    for (int i = lane; i < n; i += 64) {
      ring[i] = (uint16_t)i;
      spod[i] = 0;
    }
    for (int q = lane; q < SL; q += 64) sstart[q] = 0;
    // the command record (GL::emit): the queue's ranks now (the option sort reuses keys[]), no pod placed yet
    SimCmdHdr* rh = nullptr;
    uint32_t* rq = nullptr;
    int32_t* rp = nullptr;
    uint32_t* ro = nullptr;
    int n_add = 0;
    if constexpr (GL::emit) {
      rh = reinterpret_cast<SimCmdHdr*>(gl.rec + gl.stride * (size_t)gl.live[sim]);
      rq = reinterpret_cast<uint32_t*>(rh + 1);
      rp = reinterpret_cast<int32_t*>(rq + cap);
      ro = reinterpret_cast<uint32_t*>(rp + cap);
      for (int i = lane; i < n; i += 64) {
        rq[i] = keys[i];
        rp[i] = -1;
      }
    }
    sim_sync();

    // ---- the Solve loop -------------------------------------------------------------------------
    // need: pods that must schedule (all but the pending ones: AllNonPendingPodsScheduled)
    int need = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int i = i0 + lane;
      const bool req = i < n && a.pod_kind[a.rank_pod[keys[i]]] != 2;
      need += __builtin_popcountll(__ballot(req));
    }
    int head = 0, len = overflow ? 0 : n, n_nc = 0, placed_cnt = 0;
    uint32_t epoch = 1;
    bool abort = overflow;
    // GL::check (kp_cluster_validate): candidate pods on uninitialized nodes, non-pending pods on the NodeClaim, and
    // whether the simulation stopped at a second NodeClaim
    int n_uninit = 0, nc_np = 0;
    bool multi = false;
    // GL::why counts those too, and keeps the lowest queue position of a candidate pod on an uninitialized node and of
    // a non-pending pod on the NodeClaim (the first unscheduled pod, should its truncated options break minValues)
    int w_uninit_first = 0x7FFFFFFF, w_nc_first = 0x7FFFFFFF;
    while (len > 0) {
      const int i = ring[head];
      const uint64_t ent = spod[i];
      if ((uint32_t)(ent >> 40) == epoch && (int)(uint32_t)ent == len) break;  // Pop: no progress
      head = head + 1 == n ? 0 : head + 1;
      len--;
      pops++;
      const int lvl = (int)((ent >> 32) & 0xFF);
      const int gid = (int)a.rank_pod[keys[i]];
      const int kind = a.pod_kind[gid];
      const int shape = a.pod_shape[gid];
      const int sl = a.shape_level_base[shape] + lvl;
      stage_shape(a, sl, shape, sB, spreq, s_pslot[wave]);
      sim_sync();
      const uint64_t hpc = a.hp_any ? a.shape_hp_conf[shape] : 0, hpa = a.hp_any ? a.shape_hp_add[shape] : 0;
      int placed = -1;  // 0: the NodeClaim; <= -2: existing position -2-placed
      // addToExistingNode
      int st = sstart[sl];
      for (int w0 = st >> 6; w0 < EW; w0 += 64) {
        const int w = w0 + lane;
        uint64_t c = 0, d = 0;
        if (w < EW) {
          c = a.usable[(size_t)sl * EW + w] & ~excl[w];
          if (w == (st >> 6)) c &= ~0ull << (st & 63);
          d = c & dirty[w];
        }
        words++;
        const uint64_t cl = c & ~d;
        int found = -1;
        uint64_t dd = d & (cl ? (cl & (0 - cl)) - 1 : ~0ull);  // touched nodes before the first untouched one
        while (dd) {
          const int b = __builtin_ctzll(dd);
          dd &= dd - 1;
          const int e = w * 64 + b;
          bool fits = true;
          for (int u = 0; u < a.RU; u++) {
            const int r = a.ru_res[u];
            fits = fits && ovl[(size_t)e * a.RU + u] + spreq[r] <= a.ex_available[(size_t)e * KP_NRES + r];
          }
          if (hpc) fits = fits && !(ovlhp[e] & hpc);  // ports the simulation's pods took on the node
          if (fits) {
            found = b;
            break;
          }
        }
        if (found < 0 && cl) found = __builtin_ctzll(cl);
        const uint64_t bal = __ballot(found >= 0);
        if (bal) {
          const int L = __builtin_ctzll(bal);
          const int fb = __builtin_amdgcn_readlane(found, L);
          const int e = (w0 + L) * 64 + fb;
          placed = -2 - e;
          st = e;
          break;
        }
        st = (w0 + 64) * 64;
      }
      bytes += 8ull * 64;
      if (lane == 0) sstart[sl] = st;
      if (placed <= -2) {
        const int e = -2 - placed;
        if constexpr (GL::check) {  // the verdict counts it with the unscheduled pods; the Solve goes on
          if (!a.ex_init[e] && kind == 0) n_uninit++;
        }
        if constexpr (GL::why) {
          if (!a.ex_init[e] && kind == 0) {
            n_uninit++;
            w_uninit_first = min(w_uninit_first, i);
          }
        }
        if (!GL::check && !GL::why && !a.ex_init[e] && kind == 0) {
          abort = true;  // SimulateScheduling: a candidate pod relied on an uninitialized node
        } else {
          const bool first = !((dirty[e >> 6] >> (e & 63)) & 1);
          if (lane < a.RU) {
            const int r = a.ru_res[lane];
            const int64_t prev = first ? a.ex_requests[(size_t)e * KP_NRES + r] : ovl[(size_t)e * a.RU + lane];
            ovl[(size_t)e * a.RU + lane] = prev + spreq[r];
          }
          if (ovlhp && lane == 0) ovlhp[e] = (first ? a.ex_hp[e] : ovlhp[e]) | hpa;
          wave_sync();
          if (lane == 0) dirty[e >> 6] |= 1ull << (e & 63);
        }
        sim_sync();
      }
      // addToInflightNode (at most one NodeClaim exists)
      if (placed == -1 && n_nc == 1) {
        const uint64_t tol = a.shape_tolerates[sl];
        bool cand = ((tol >> nc->taintset) & 1) && ncfail[sl] != nc->ver && !(nc->hp & hpc);
        if (cand)
          for (int r = 0; r < KP_NRES; r++)
            if (((rmask >> r) & 1) && nc->requests[r] + spreq[r] > nc->maxalloc[r]) cand = false;
        if (cand) {
          attempts++;
          const int cat = a.tmpl_catalog[nc->tmpl];
          uint64_t m_v = 0, X = 0;
          ReqView rv;
          bool ok = merge_compatible(D, &nc->reqs, sB, a.shape_negop[sl], true, m_v, rv, &slots[wave],
                                     vint_global(a.vint));
          bytes += sizeof(KReqs);
          if (ok) {
            X = lane < D.TW ? nc->X[lane] : 0;
            const uint64_t* pvp = a.shape_pvp + (size_t)a.pvp_base[sl * a.n_catalogs + cat] * D.TW;
            const int64_t q_lane = lane < KP_NRES ? nc->requests[lane] + spreq[lane] : 0;
            const int32_t j0_lane = lane < KP_NRES ? nc->fitj[lane] : 0;
            X = filter_types(D, hdr(cat), rv, m_v, X, sB->present, pvp, s_pslot[wave], q_lane, j0_lane, nullptr,
                             rmask, vint_global(a.vint), s_scratch[wave], (RowPtr LDS*)s_rl[wave],
                             &bytes, s_fitj[wave]);
            ok = __ballot(X != 0) != 0;
          }
          if (ok) {
            store_merged(&nc->reqs, rv, m_v, D.W, D.KB);
            if (lane < D.TW) nc->X[lane] = X;
            if (lane < KP_NRES) {
              nc->requests[lane] += spreq[lane];
              nc->fitj[lane] = s_fitj[wave][lane];
            }
            if (lane == 0) nc->ver = ++vcount;
            if (lane == 0) nc->hp |= hpa;
            placed = 0;
          } else if (lane == 0) {
            ncfail[sl] = nc->ver;
          }
          sim_sync();
        }
      }
      // addToNewNodeClaim: precomputed outcome; a second NodeClaim makes the result a no-op
      if (placed == -1 && a.tres[sl].tmpl >= 0) {
        if (n_nc == 1) {
          abort = true;
          if constexpr (GL::check || GL::why) multi = true;
        } else {
          copy_u64(reinterpret_cast<uint64_t*>(nc), reinterpret_cast<const uint64_t*>(&a.tres[sl]),
                   (int)(sizeof(SimNC) / 8));
          sim_sync();
          if (lane == 0) nc->ver = ++vcount;
          sim_sync();
          n_nc = 1;
          placed = 0;
        }
      }
      if (abort) break;
      if (placed != -1) {
        if (kind != 2) placed_cnt++;
        if constexpr (GL::check) {
          if (placed == 0 && kind != 2) nc_np++;
        }
        if constexpr (GL::why) {
          if (placed == 0 && kind != 2) {
            nc_np++;
            w_nc_first = min(w_nc_first, i);
          }
        }
        if constexpr (GL::emit) {  // where the pod went, and the NodeClaim's add order
          if (lane == 0) {
            rp[i] = placed;
            if (placed == 0) ro[n_add] = (uint32_t)i;
          }
          if (placed == 0) n_add++;
        }
      } else {  // Preferences.Relax + Queue.Push
        const bool relaxed = lvl + 1 < a.shape_nlevels[shape];
        int tail = head + len;
        if (tail >= n) tail -= n;
        len++;
        uint64_t ne;
        if (relaxed) {
          epoch++;  // lastLen = map{}
          ne = (uint64_t)(lvl + 1) << 32;
        } else {
          ne = ((uint64_t)epoch << 40) | ((uint64_t)lvl << 32) | (uint32_t)len;
        }
        if (lane == 0) {
          ring[tail] = (uint16_t)i;
          spod[i] = ne;
        }
        sim_sync();
      }
    }

    // GL::why: the first unscheduled pod in queue order, as cluster pod indices, before the option sort reuses keys[].
    // The pods never placed are what the ring still holds (len entries from head); w_pod_bad is the first of those and
    // of the candidate pods on uninitialized nodes, w_pod_nc the first non-pending pod on the NodeClaim.
    int w_pos_bad = 0x7FFFFFFF, w_pod_bad = -1, w_pod_nc = -1;
    if constexpr (GL::why) {
      if (!abort) {
        int mine = w_uninit_first;
        for (int k = lane; k < len; k += 64) {
          int at = head + k;
          if (at >= n) at -= n;
          const int i = ring[at];
          if (a.pod_kind[a.rank_pod[keys[i]]] != 2) mine = min(mine, i);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mine = min(mine, __shfl_xor(mine, o, 64));
        w_pos_bad = mine;
        if (w_pos_bad != 0x7FFFFFFF) w_pod_bad = (int)a.rank_pod[keys[w_pos_bad]];
        if (w_nc_first != 0x7FFFFFFF) w_pod_nc = (int)a.rank_pod[keys[w_nc_first]];
      }
      sim_sync();
    }

    // ---- decision (computeConsolidation) ---------------------------------------------------------
    int decision = KP_DECISION_NOOP, nodepool = 0, n_options = 0;
    double repl = 0, savings = 0;
    const double candReported = priced ? candPrice : 0.0;
    // GL::check: whether the truncated options kept minValues, and the command's options absent from them. The
    // truncation runs for every finished simulation with a NodeClaim, whatever the candidates' prices and the
    // spot-to-spot gate say, and no price stage runs.
    bool v_minok = true;
    int v_missing = 0;
    // GL::why: the exit (enum kp_unconsolidatable) and the stage counts; w_sched: every non-pending pod scheduled, none
    // on an uninitialized node - what takes the other deciding policies past this point
    const bool w_sched = placed_cnt == need && n_uninit == 0;
    int w_reason = KP_UNCONS_NONE, w_stage = 0, w_trunc = 0, w_cheaper = 0, w_same = 0;
    double w_cheapest = 0;
    if (!abort && (GL::check || GL::why || placed_cnt == need)) {
      if (n_nc == 0) {
        if (!GL::why || w_sched) {
          decision = KP_DECISION_DELETE;
          savings = candReported;
        }
      } else if (GL::check || GL::why || priced) {
        const int cat = a.tmpl_catalog[nc->tmpl];
        const DevCatalog& Cg = a.cats[cat];
        const uint64_t v = lane < D.W ? nc->reqs.vals[lane] : 0;
        const ReqView rv = stored_view(D, &nc->reqs, v);
        const uint64_t negR = negop_mask(rv.present, rv.compl_, rv.nz);
        const uint64_t allowed = allowed_word(D, rv, v, vint_global(a.vint));
        const uint64_t cls = allowed_classes(D, Cg.cls, rv, allowed, negR);
        const bool ctp = (rv.present >> a.ct_key) & 1;
        bool ncSpot;
        if (a.spot_bit >= 0) ncSpot = !ctp || bit_of(allowed, a.spot_bit);
        else ncSpot = !ctp || ((rv.compl_ >> a.ct_key) & 1);
        // spot-to-spot (every candidate spot, the replacement may launch spot): only with the feature gate, on
        // the replacement narrowed to spot offerings, and a single candidate needs 15 cheaper options
        const bool s2s = allSpot && ncSpot;
        if (GL::check || GL::why || !s2s || a.spot_to_spot) {
          // TruncateInstanceTypes: OrderByPrice (cheapest compatible offering, then name) + cut
          const uint64_t Xl = lane < D.TW ? nc->X[lane] : 0;
          int cnt = 0;
          for (int ch = 0; ch < D.TW; ch++) {
            const uint64_t wd = lane_bcast(Xl, ch);
            const int t = ch * 64 + lane;
            const bool has = (wd >> lane) & 1;
            double p = __builtin_huge_val();
            if (has && Cg.price_sub) {  // min over the compatible class set in one gather
              p = Cg.price_sub[(size_t)cls * D.T + t];
            } else if (has) {
              uint64_t m = cls;
              while (m) {
                const int c = __builtin_ctzll(m);
                m &= m - 1;
                const double q = Cg.price[(size_t)t * D.C + c];
                p = q < p ? q : p;
              }
            }
            const uint64_t bal = __ballot(has);
            if (has) {
              const int pos = cnt + __builtin_popcountll(bal & ((1ull << lane) - 1));
              fkey[pos] = (uint64_t)__double_as_longlong(p);
              fidx[pos] = (Cg.name_rank[t] << 12) | (uint32_t)t;
            }
            cnt += __builtin_popcountll(bal);
          }
          int m2 = 1;
          while (m2 < cnt) m2 <<= 1;
          for (int q = cnt + lane; q < m2; q += 64) {
            fkey[q] = ~0ull;
            fidx[q] = ~0u;
          }
          wave_sync();
          wave_bitonic_kv(fkey, fidx, m2);
          const int lim = a.max_types ? min(cnt, a.max_types) : cnt;
          uint64_t* msk = s_mask[wave];
          const uint64_t hmin = rv.hmin & rv.present;
          bool ok = true;
          if (GL::check || hmin) {  // the truncated list as a type mask (GL::check: the subset test reads it too)
            msk[lane] = 0;
            wave_sync();
            for (int q = lane; q < lim; q += 64) {
              const uint32_t t = fidx[q] & 4095u;
              atomicOr((unsigned long long*)&msk[t >> 6], 1ull << (t & 63));
            }
            wave_sync();
          }
          if (hmin) {  // minValues must survive the truncation, else the pods fail (no-op)
            ok = minvalues_ok(D, Cg.code, Cg.TM, hmin, rv.minv, lane < D.TW ? msk[lane] : 0, s_scratch[wave]);
          }
          if constexpr (GL::check) {
            // the subset test, lane = mask word: the command's types the truncated list lacks (a list that broke
            // minValues is no list), plus its names this catalogue does not hold
            const size_t row = (size_t)gl.live[sim] * a.n_catalogs + cat;
            const uint64_t want = lane < D.TW ? gl.want[row * D.TW + lane] : 0;
            const uint64_t have = ok && lane < D.TW ? msk[lane] : 0;
            v_minok = ok;
            v_missing = wave_sum(__popcll(want & ~have)) + (int)gl.unknown[row];
          } else {
            // filterByPrice: Offerings.Available().WorstLaunchPrice(reqs) < candidate price
            double wlp[2] = {__DBL_MAX__, __DBL_MAX__};
            int tt[2] = {-1, -1};
            for (int h = 0; h < 2; h++) {
              const int q = h * 64 + lane;
              if (q >= lim) continue;
              const int t = (int)(fidx[q] & 4095u);
              tt[h] = t;
              for (int pass = 0; pass < (s2s ? 1 : 2); pass++) {  // capacity-type precedence: spot, on-demand
                const int ctb = pass == 0 ? a.spot_bit : a.od_bit;
                if (ctb < 0) continue;
                bool any = false;
                double mx = 0;
                uint64_t m = cls;
                while (m) {
                  const int c = __builtin_ctzll(m);
                  m &= m - 1;
                  if (Cg.cls[c].ct_bit != ctb || !((Cg.offer_avail[(size_t)c * D.TW + (t >> 6)] >> (t & 63)) & 1)) continue;
                  const double pr = Cg.price[(size_t)t * D.C + c];
                  if (!any || pr > mx) mx = pr;
                  any = true;
                }
                if (any) {
                  wlp[h] = mx;
                  break;
                }
              }
            }
            if constexpr (GL::why) {
              // Truncate's verdict is the Solve's (v_minok: a broken list fails the NodeClaim's pods). A scheduled
              // simulation whose list held reports it and its cheapest worst launch price over both lane halves; the
              // price stages run only past the candidates' prices and the spot-to-spot gate, in that order.
              v_minok = ok;
              if (ok && w_sched) {
                w_trunc = lim;
                w_cheapest = wave_min_f64(wlp[0] < wlp[1] ? wlp[0] : wlp[1]);
                if (!priced) w_reason = KP_UNCONS_UNPRICED;
                else if (s2s && !a.spot_to_spot) w_reason = KP_UNCONS_SPOT_TO_SPOT_DISABLED;
              }
              ok = ok && w_sched && w_reason == KP_UNCONS_NONE;
            }
            bool keep[2] = {tt[0] >= 0 && wlp[0] < candPrice, tt[1] >= 0 && wlp[1] < candPrice};
            for (int stage = 0; stage < 2 && ok; stage++) {
              if (stage == 1) {
                if (!a.multi_node) break;
                // filterOutSameType: the cheapest candidate of a kept option's type caps the price
                double mp = __DBL_MAX__;
                for (int h = 0; h < 2; h++) {
                  if (!keep[h]) continue;
                  const uint32_t nm = a.type_name[(size_t)cat * D.T + tt[h]];
                  for (int i = 0; i < ns; i++) {
                    const uint32_t c = a.sub_nodes[s0 + i];
                    if ((a.node_flags[c] & 1) && a.node_name[c] == nm && a.node_price[c] < mp) mp = a.node_price[c];
                  }
                }
                const double maxPrice = wave_min_f64(mp);
                keep[0] = keep[0] && wlp[0] < maxPrice;
                keep[1] = keep[1] && wlp[1] < maxPrice;
              }
              const int count = wave_sum((keep[0] ? 1 : 0) + (keep[1] ? 1 : 0));
              if (hmin) {
                msk[lane] = 0;
                wave_sync();
                for (int h = 0; h < 2; h++)
                  if (keep[h]) atomicOr((unsigned long long*)&msk[tt[h] >> 6], 1ull << (tt[h] & 63));
                wave_sync();
                if (!minvalues_ok(D, Cg.code, Cg.TM, hmin, rv.minv, lane < D.TW ? msk[lane] : 0, s_scratch[wave])) ok = false;
              }
              if (count == 0) ok = false;
              n_options = count;
              if constexpr (GL::why) {  // an empty set is the filter's exit; minValues only breaks a non-empty one
                if (stage == 0) w_cheaper = count;
                else w_same = count;
                if (count == 0) w_reason = stage == 0 ? KP_UNCONS_NOT_CHEAPER : KP_UNCONS_SAME_TYPE;
                else if (!ok) w_reason = KP_UNCONS_MIN_VALUES, w_stage = stage + 1;
              }
            }
            if constexpr (GL::why) {
              if (ok && !a.multi_node) w_same = w_cheaper;  // no same-type filter: the set passes on
            }
            if (ok && s2s && ns == 1) {  // MinInstanceTypesForSpotToSpotConsolidation, then the launch keeps 15
              if (n_options < 15) {
                ok = false;
                if constexpr (GL::why) w_reason = KP_UNCONS_SPOT_FLEXIBILITY;
              } else {  // the first 15 (100 with minValues) kept options in price order
                const int L = hmin ? 100 : 15;
                const uint64_t lt = (1ull << lane) - 1;
                const uint64_t b0 = __ballot(keep[0]), b1 = __ballot(keep[1]);
                keep[0] = keep[0] && __popcll(b0 & lt) < L;
                keep[1] = keep[1] && __popcll(b0) + __popcll(b1 & lt) < L;
                n_options = min(n_options, L);
              }
            }
            if (ok) {
              double b = __DBL_MAX__;
              for (int h = 0; h < 2; h++)
                if (keep[h] && wlp[h] < b) b = wlp[h];
              const double best = wave_min_f64(b);
              decision = KP_DECISION_REPLACE;
              nodepool = a.tmpl_nodepool[nc->tmpl];
              repl = best;
              savings = candPrice - best;
              if constexpr (GL::emit) {
                // the kept options in price order: keep[0..1] compacted over the sorted list, the second 64-lane half
                // behind the first one's count
                const uint64_t lt = (1ull << lane) - 1;
                const uint64_t b0 = __ballot(keep[0]), b1 = __ballot(keep[1]);
                if (keep[0]) rh->options[__popcll(b0 & lt)] = (uint32_t)tt[0];
                if (keep[1]) rh->options[__popcll(b0) + __popcll(b1 & lt)] = (uint32_t)tt[1];
                copy_u64(reinterpret_cast<uint64_t*>(&rh->reqs), reinterpret_cast<const uint64_t*>(&nc->reqs),
                         (int)(sizeof(KReqs) / 8));
                if (lane < KP_NRES) rh->requests[lane] = nc->requests[lane];
                if (lane == 0) {
                  rh->tmpl = nc->tmpl;
                  rh->n_remaining = (uint32_t)cnt;
                  rh->n_kept = (uint32_t)n_options;
                  rh->s2s = s2s ? 1u : 0u;
                }
              }
            } else {
              n_options = 0;
            }
          }
        }
      }
    }
    if constexpr (GL::check) {
      // the rule of kp_abi.h (kp_cluster_validate) on this simulation; every lane holds the same six words
      const uint32_t sub = gl.live[sim];
      const bool has_repl = gl.replace[sub] != 0;
      uint32_t verdict = KP_VALID, unsched = 0, missing = 0;
      if (multi) {
        verdict = KP_INVALID_MULTIPLE;
      } else if (!overflow) {
        unsched = (uint32_t)(need - placed_cnt + n_uninit + (v_minok ? 0 : nc_np));
        if (unsched) verdict = KP_INVALID_UNSCHEDULED;
        else if (n_nc == 0) verdict = has_repl ? KP_INVALID_NO_REPLACEMENT_NEEDED : KP_VALID;
        else if (!has_repl) verdict = KP_INVALID_NEEDS_REPLACEMENT;
        else if (v_missing) verdict = KP_INVALID_NOT_SUBSET, missing = (uint32_t)v_missing;
      }
      const uint32_t w[6] = {verdict, multi ? 2u : (uint32_t)n_nc, overflow ? 0xFFFFFFFFu : (uint32_t)n, unsched, missing, 0u};
      uint32_t mine = 0;
#pragma unroll
      for (int k = 0; k < 6; k++) mine = lane == k ? w[k] : mine;
      if (lane < 6) gl.val[(size_t)sub * 6 + lane] = mine;
    }
    if constexpr (GL::why) {
      // the record of kp_abi.h (kp_sim_why) from this simulation's own values; every lane holds the same twelve words
      // and every word is written whatever the exit, so nothing of the slot's previous subset survives
      uint32_t unsched = 0;
      int first = -1;
      if (multi) {
        w_reason = KP_UNCONS_MULTIPLE_NODECLAIMS;
      } else if (!overflow) {
        unsched = (uint32_t)(need - placed_cnt + n_uninit + (v_minok ? 0 : nc_np));
        first = w_pod_bad;
        if (!v_minok && w_nc_first < w_pos_bad) first = w_pod_nc;
        if (unsched || !v_minok) w_reason = KP_UNCONS_UNSCHEDULABLE;
      }
      const bool solved = w_reason != KP_UNCONS_MULTIPLE_NODECLAIMS && w_reason != KP_UNCONS_UNSCHEDULABLE;
      const uint64_t cl = (uint64_t)__double_as_longlong(solved ? w_cheapest : 0.0);
      const uint32_t w[WHY_WORDS] = {(uint32_t)w_reason,
                                     (uint32_t)w_stage,
                                     multi ? 2u : (uint32_t)n_nc,
                                     unsched,
                                     (uint32_t)first,
                                     (uint32_t)(w_reason == KP_UNCONS_UNPRICED ? w_unpriced : -1),
                                     solved ? (uint32_t)w_trunc : 0u,
                                     (uint32_t)w_cheaper,
                                     (uint32_t)w_same,
                                     0u,
                                     (uint32_t)cl,
                                     (uint32_t)(cl >> 32)};
      uint32_t mine = 0;
#pragma unroll
      for (int k = 0; k < WHY_WORDS; k++) mine = lane == k ? w[k] : mine;
      if (lane < WHY_WORDS) gl.rec[(size_t)gl.live[sim] * WHY_WORDS + lane] = mine;
    }
    if (!GL::check && lane == 0) {
      SimOut o;
      o.decision = decision;
      o.nodepool = (uint32_t)nodepool;
      o.candidate_price = candReported;
      o.replacement_price = repl;
      o.savings = savings;
      o.n_options = (uint32_t)(decision == KP_DECISION_REPLACE ? n_options : 0);
      o.n_pods = overflow ? 0xFFFFFFFFu : (uint32_t)n;
      a.out[GL::gated ? (int)gl.live[sim] : sim] = o;
      if constexpr (GL::emit) {
        rh->n_queue = (uint32_t)n;
        rh->n_added = (uint32_t)n_add;
      }
    }
    sim_sync();
  }
  if (lane == 0) {
    atomicAdd((unsigned long long*)&a.stats[0], (unsigned long long)attempts);
    atomicAdd((unsigned long long*)&a.stats[1], (unsigned long long)bytes);
    atomicAdd((unsigned long long*)&a.stats[2], (unsigned long long)pops);
    atomicAdd((unsigned long long*)&a.stats[3], (unsigned long long)words);
    if (cancelled) atomicAdd((unsigned long long*)&a.stats[5], 1ull);
  }
}

hipError_t launch_sim_prep(const SimArgs& a, hipStream_t s) {
  const long items = (long)a.SL * a.EW;
  long blocks = (items + SIM_WAVES - 1) / SIM_WAVES;
  blocks = blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks);
  if (a.EW > 0) hipLaunchKernelGGL(sim_usable_kernel, dim3((unsigned)blocks), dim3(SIM_WAVES * 64), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int pb = (a.SL + SIM_WAVES - 1) / SIM_WAVES;
  if (pb > 0) hipLaunchKernelGGL(sim_prep_kernel, dim3(pb), dim3(SIM_WAVES * 64), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_sim(const SimArgs& a, int blocks, size_t dyn_lds, hipStream_t s) {
  hipLaunchKernelGGL((sim_kernel<SIM_WAVES, SimAll>), dim3(blocks), dim3(SIM_WAVES * 64), dyn_lds, s, a, SimAll{});
  return hipGetLastError();
}
hipError_t launch_sim_gated(const SimArgs& a, const uint32_t* live, int n_live, int blocks, size_t dyn_lds, hipStream_t s) {
  SimArgs al = a;
  al.n_subsets = n_live;
  hipLaunchKernelGGL((sim_kernel<SIM_WAVES, SimLive>), dim3(blocks), dim3(SIM_WAVES * 64), dyn_lds, s, al, SimLive{live});
  return hipGetLastError();
}
hipError_t launch_sim_emit(const SimArgs& a, const SimEmit& em, int n_live, int blocks, size_t dyn_lds, hipStream_t s) {
  SimArgs al = a;
  al.n_subsets = n_live;
  hipLaunchKernelGGL((sim_kernel<SIM_WAVES, SimEmit>), dim3(blocks), dim3(SIM_WAVES * 64), dyn_lds, s, al, em);
  return hipGetLastError();
}
const void* sim_emit_kernel_ptr() { return reinterpret_cast<const void*>(sim_kernel<SIM_WAVES, SimEmit>); }
hipError_t launch_sim_check(const SimArgs& a, const SimCheck& ck, int n_live, int blocks, size_t dyn_lds, hipStream_t s) {
  SimArgs al = a;
  al.n_subsets = n_live;
  hipLaunchKernelGGL((sim_kernel<SIM_WAVES, SimCheck>), dim3(blocks), dim3(SIM_WAVES * 64), dyn_lds, s, al, ck);
  return hipGetLastError();
}
const void* sim_check_kernel_ptr() { return reinterpret_cast<const void*>(sim_kernel<SIM_WAVES, SimCheck>); }
hipError_t launch_sim_why(const SimArgs& a, const SimWhy& wy, int n_live, int blocks, size_t dyn_lds, hipStream_t s) {
  SimArgs al = a;
  al.n_subsets = n_live;
  hipLaunchKernelGGL((sim_kernel<SIM_WAVES, SimWhy>), dim3(blocks), dim3(SIM_WAVES * 64), dyn_lds, s, al, wy);
  return hipGetLastError();
}
const void* sim_why_kernel_ptr() { return reinterpret_cast<const void*>(sim_kernel<SIM_WAVES, SimWhy>); }

// ------------------------------------------------------------------------------------------------
// The histogram of a batch's reasons (kp_cluster_simulate_explained), so that a sweep is explained without reading its
// 48-byte records back. Two stages as argmax_kernel's: blocks count contiguous ranges into part[block][reason], one
// block adds the partials. Integer counts in registers, a shuffle tree per wave and one LDS row per wave: no atomics,
// and the result does not depend on any order. A subset the budget gate blocked has no simulation: the first stage
// writes its KP_UNCONS_BUDGET record (one thread, twelve plain stores) and counts it there.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WHY_COUNT_THREADS) void why_count_kernel(uint32_t* rec, const uint8_t* gate, int n,
                                                                      uint64_t* part) {
  __shared__ uint32_t s_cnt[WHY_COUNT_THREADS / 64][WHY_REASONS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = LANE;
  const int per = (n + gridDim.x - 1) / gridDim.x;
  const int lo = blockIdx.x * per, hi = min(n, lo + per);
  uint32_t c[WHY_REASONS];
#pragma unroll
  for (int k = 0; k < WHY_REASONS; k++) c[k] = 0;
  for (int i = lo + tid; i < hi; i += WHY_COUNT_THREADS) {
    uint32_t* r = rec + (size_t)i * WHY_WORDS;
    uint32_t reason;
    if (gate && !gate[i]) {
      reason = KP_UNCONS_BUDGET;
#pragma unroll
      for (int k = 0; k < WHY_WORDS; k++) r[k] = k == 0 ? (uint32_t)KP_UNCONS_BUDGET : ((k == 4 || k == 5) ? 0xFFFFFFFFu : 0u);
    } else {
      reason = r[0];
    }
#pragma unroll
    for (int k = 0; k < WHY_REASONS; k++) c[k] += reason == (uint32_t)k ? 1u : 0u;
  }
#pragma unroll
  for (int k = 0; k < WHY_REASONS; k++) {
    uint32_t v = c[k];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) s_cnt[wave][k] = v;
  }
  __syncthreads();
  if (tid < WHY_REASONS) {
    uint64_t t = 0;
    for (int w = 0; w < WHY_COUNT_THREADS / 64; w++) t += s_cnt[w][tid];
    part[(size_t)blockIdx.x * WHY_REASONS + tid] = t;
  }
}
// one block: thread k adds the partials of reason k, in block order
__global__ __launch_bounds__(64) void why_count_final_kernel(const uint64_t* part, int np, uint64_t* counts) {
  const int k = threadIdx.x;
  if (k >= WHY_REASONS) return;
  uint64_t t = 0;
  for (int b = 0; b < np; b++) t += part[(size_t)b * WHY_REASONS + k];
  counts[k] = t;
}
hipError_t launch_why_count(uint32_t* rec, const uint8_t* gate, int n, uint64_t* part, uint64_t* counts, hipStream_t s) {
  const int nb = why_count_blocks(n);
  if (n > 0) {
    hipLaunchKernelGGL(why_count_kernel, dim3(nb), dim3(WHY_COUNT_THREADS), 0, s, rec, gate, n, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(why_count_final_kernel, dim3(1), dim3(64), 0, s, part, n > 0 ? nb : 0, counts);
  return hipGetLastError();
}
const void* sim_kernel_ptr(bool gated) {
  return gated ? reinterpret_cast<const void*>(sim_kernel<SIM_WAVES, SimLive>)
               : reinterpret_cast<const void*>(sim_kernel<SIM_WAVES, SimAll>);
}

// ------------------------------------------------------------------------------------------------
// Best decision of a simulated batch (kp_consolidate_argmin): max savings over non-no-op decisions, ties to the
// lowest subset index, plus the decision counts. Two stages: blocks reduce contiguous ranges, one block the partials.
// ------------------------------------------------------------------------------------------------
#define ARGMAX_THREADS 256
__device__ __forceinline__ bool better(double s, int64_t i, double bs, int64_t bi) {
  return i >= 0 && (bi < 0 || s > bs || (s == bs && i < bi));
}
__global__ __launch_bounds__(ARGMAX_THREADS) void argmax_kernel(const SimOut* out, int n, ArgmaxPart* part) {
  __shared__ double s_s[ARGMAX_THREADS];
  __shared__ int64_t s_i[ARGMAX_THREADS];
  __shared__ unsigned long long s_cnt[4];
  const int tid = threadIdx.x;
  if (tid < 4) s_cnt[tid] = 0;
  __syncthreads();
  const int per = (n + gridDim.x - 1) / gridDim.x;
  const int lo = blockIdx.x * per, hi = min(n, lo + per);
  double bs = 0;
  int64_t bi = -1;
  unsigned long long c[4] = {0, 0, 0, 0};
  for (int i = lo + tid; i < hi; i += ARGMAX_THREADS) {
    const SimOut o = out[i];
    const int d = o.decision;
    c[d == KP_DECISION_DELETE ? 1 : (d == KP_DECISION_REPLACE ? 2 : 0)]++;
    if (o.n_pods == 0xFFFFFFFFu) c[3]++;  // overflowed the pod queue (an error on the host)
    if (d != KP_DECISION_NOOP && better(o.savings, i, bs, bi)) bs = o.savings, bi = i;
  }
  s_s[tid] = bs;
  s_i[tid] = bi;
  for (int k = 0; k < 4; k++) atomicAdd(&s_cnt[k], c[k]);
  __syncthreads();
  for (int w = ARGMAX_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w && better(s_s[tid + w], s_i[tid + w], s_s[tid], s_i[tid])) {
      s_s[tid] = s_s[tid + w];
      s_i[tid] = s_i[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[blockIdx.x].savings = s_s[0];
    part[blockIdx.x].index = s_i[0];
    for (int k = 0; k < 4; k++) part[blockIdx.x].counts[k] = s_cnt[k];
  }
}
// one block: partials -> the record this rank contributes to the all-gather
__global__ __launch_bounds__(ARGMAX_THREADS) void argmax_final_kernel(const ArgmaxPart* part, int np, const SimOut* out,
                                                                     int64_t base, CommBest* dst) {
  __shared__ double s_s[ARGMAX_THREADS];
  __shared__ int64_t s_i[ARGMAX_THREADS];
  __shared__ unsigned long long s_cnt[4];
  const int tid = threadIdx.x;
  if (tid < 4) s_cnt[tid] = 0;
  __syncthreads();
  double bs = 0;
  int64_t bi = -1;
  unsigned long long c[4] = {0, 0, 0, 0};
  for (int i = tid; i < np; i += ARGMAX_THREADS) {
    if (better(part[i].savings, part[i].index, bs, bi)) bs = part[i].savings, bi = part[i].index;
    for (int k = 0; k < 4; k++) c[k] += part[i].counts[k];
  }
  s_s[tid] = bs;
  s_i[tid] = bi;
  for (int k = 0; k < 4; k++) atomicAdd(&s_cnt[k], c[k]);
  __syncthreads();
  for (int w = ARGMAX_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w && better(s_s[tid + w], s_i[tid + w], s_s[tid], s_i[tid])) {
      s_s[tid] = s_s[tid + w];
      s_i[tid] = s_i[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    dst->index = s_i[0] >= 0 ? base + s_i[0] : -1;
    if (s_i[0] >= 0) dst->rec = out[s_i[0]];
    else memset(&dst->rec, 0, sizeof(SimOut));
    for (int k = 0; k < 4; k++) dst->counts[k] = s_cnt[k];
  }
}
hipError_t launch_argmax(const SimOut* out, int n, ArgmaxPart* part, int n_parts, int64_t base, CommBest* dst,
                         hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(argmax_kernel, dim3(n_parts), dim3(ARGMAX_THREADS), 0, s, out, n, part);
  else (void)hipMemsetAsync(part, 0xFF, sizeof(ArgmaxPart) * n_parts, s);  // index -1 everywhere (counts fixed below)
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(argmax_final_kernel, dim3(1), dim3(ARGMAX_THREADS), 0, s, part, n > 0 ? n_parts : 0, out, base, dst);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// NodePool disruption budgets (kp_cluster_simulate_budgeted / kp_consolidate_argmin_budgeted): a subset is admissible
// iff no NodePool owns more of its members than allowed[pool] (R:website/content/en/preview/concepts/disruption.md:
// 274-333). The gate runs over the resident CSR batch before sim_kernel and leaves, besides the per-subset gate byte
// and the zero no-op of every blocked subset, the ascending list live[] of the admissible ones, which the gated
// sim_kernel walks. The list is built order-preserving (count per block, scan of the block counts in one block,
// scatter), so which wave simulates which subset is the same from run to run.
// ------------------------------------------------------------------------------------------------
static_assert(GATE_BLOCK == 64, "gate_scatter_kernel: one wave per block of the gate");
// One subset per wave at a time, GATE_PER_WAVE consecutive subsets per wave. Members are loaded 64 at a time
// (coalesced over sub_nodes), their pools gathered from the node table, and the per-pool counts of the chunk taken
// from the wave's own ballot: the first pending lane's pool, the lanes that share it, their popcount; per-wave LDS
// counters carry the counts across chunks.
__global__ __launch_bounds__(GATE_WAVES * 64) void budget_gate_kernel(GateArgs g) {
  __shared__ uint32_t s_cnt[GATE_WAVES][GATE_MAX_POOLS];
  __shared__ uint32_t s_adm[GATE_WAVES];
  const int wave = threadIdx.x >> 6, lane = LANE;
  uint32_t* cnt = s_cnt[wave];
  const int n_pools = min(g.n_pools, GATE_MAX_POOLS);
  const int first = blockIdx.x * GATE_BLOCK + wave * GATE_PER_WAVE;
  uint32_t adm = 0;
  for (int k = 0; k < GATE_PER_WAVE; k++) {
    const int sim = first + k;
    if (sim >= g.n_subsets) break;
    for (int q = lane; q < n_pools; q += 64) cnt[q] = 0;
    wave_sync();
    const uint32_t s0 = g.sub_off[sim], ns = g.sub_off[sim + 1] - s0;
    for (uint32_t i0 = 0; i0 < ns; i0 += 64) {
      const uint32_t i = i0 + lane;
      const bool valid = i < ns;
      uint32_t p = 0xFFFFu;
      if (valid) {
        const uint32_t c = g.sub_nodes[s0 + i];
        if (c < (uint32_t)g.n_nodes) p = g.node_pool[c];
      }
      uint64_t todo = __ballot(valid);
      while (todo) {
        const int L = __builtin_ctzll(todo);
        const uint32_t pl = (uint32_t)__builtin_amdgcn_readlane((int)p, L);
        const uint64_t same = __ballot(valid && p == pl);
        if (lane == 0 && pl < (uint32_t)n_pools) cnt[pl] += (uint32_t)__builtin_popcountll(same);
        todo &= ~same;
      }
    }
    wave_sync();
    bool over = false;
    for (int q = lane; q < n_pools; q += 64) over = over || cnt[q] > g.allowed[q];
    const bool ok = __ballot(over) == 0;
    if (lane == 0) {
      g.gate[sim] = ok ? 1 : 0;
      if (!ok) {  // a blocked subset is not simulated: the zero no-op
        SimOut o;
        o.decision = KP_DECISION_NOOP;
        o.nodepool = 0;
        o.candidate_price = 0;
        o.replacement_price = 0;
        o.savings = 0;
        o.n_options = 0;
        o.n_pods = 0;
        g.out[sim] = o;
      }
    }
    adm += ok ? 1u : 0u;
    wave_sync();
  }
  if (lane == 0) s_adm[wave] = adm;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < GATE_WAVES; w++) t += s_adm[w];
    g.blk_cnt[blockIdx.x] = t;
  }
}
// one block: exclusive scan of the gate blocks' counts, and the live count
#define GATE_SCAN_THREADS 256
__global__ __launch_bounds__(GATE_SCAN_THREADS) void gate_scan_kernel(GateArgs g, int nb) {
  __shared__ uint32_t s_sum[GATE_SCAN_THREADS];
  const int tid = threadIdx.x;
  const int per = (nb + GATE_SCAN_THREADS - 1) / GATE_SCAN_THREADS;
  const int lo = min(nb, tid * per), hi = min(nb, lo + per);
  uint32_t s = 0;
  for (int i = lo; i < hi; i++) s += g.blk_cnt[i];
  s_sum[tid] = s;
  __syncthreads();
  for (int d = 1; d < GATE_SCAN_THREADS; d <<= 1) {
    const uint32_t v = tid >= d ? s_sum[tid - d] : 0;
    __syncthreads();
    s_sum[tid] += v;
    __syncthreads();
  }
  uint32_t run = s_sum[tid] - s;
  for (int i = lo; i < hi; i++) {
    g.blk_off[i] = run;
    run += g.blk_cnt[i];
  }
  if (tid == GATE_SCAN_THREADS - 1) *g.n_live = s_sum[tid];
}
// one wave per gate block: its admissible subsets, in order, behind those of the blocks before it
__global__ __launch_bounds__(64) void gate_scatter_kernel(GateArgs g) {
  const int lane = LANE;
  const int sim = blockIdx.x * GATE_BLOCK + lane;
  const bool ok = sim < g.n_subsets && g.gate[sim] != 0;
  const uint64_t bal = __ballot(ok);
  if (ok) g.live[g.blk_off[blockIdx.x] + __builtin_popcountll(bal & ((1ull << lane) - 1))] = (uint32_t)sim;
}
hipError_t launch_budget_gate(const GateArgs& g, hipStream_t s) {
  const int nb = (g.n_subsets + GATE_BLOCK - 1) / GATE_BLOCK;
  if (nb < 1 || g.n_pools > GATE_MAX_POOLS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(budget_gate_kernel, dim3(nb), dim3(GATE_WAVES * 64), 0, s, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gate_scan_kernel, dim3(1), dim3(GATE_SCAN_THREADS), 0, s, g, nb);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gate_scatter_kernel, dim3(nb), dim3(64), 0, s, g);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Drift (kp_cluster_drift): every simulation of a general-path launch is a whole Solve (no early stop); what the host
// needs of it is AllNonPendingPodsScheduled, not its placements. drift_verdict_kernel reduces each simulation's
// placements to one 24-byte DriftOut, drift_first_kernel the launch's verdicts to one record (the lowest caller-order
// subset index among the feasible ones, the Solves' counters); the launch then downloads verdicts only. Both run
// behind solve_kernel in the launch's stream. Plain (vector) stores, no global atomics: each output has one writer.
// ------------------------------------------------------------------------------------------------
// One wave per simulation; the lanes stride over its queue positions: placement, the pod's kind (2 pending, 1 a
// deleting node's, 0 a candidate's) and, for a candidate pod on an existing node, that position's "not initialized"
// bit. The ballot of a 64-position chunk gives the count and - its lowest bit in the first chunk that has one - the
// first failing position.
// (The scan is a device function of its own: validate_verdict_kernel shares it. ON_NC also counts the non-pending pods
// on a new NodeClaim.)
struct Unscheduled {
  uint32_t n_bad;  // non-pending pods unscheduled or (candidate pods) on an uninitialized node
  int first;       // the first such queue position, -1
  uint32_t nc_np;  // ON_NC: non-pending pods on a new NodeClaim
};
template <bool ON_NC>
__device__ __forceinline__ Unscheduled scan_unscheduled(const DriftArgs& a, const int32_t* place, const int32_t* qp, int n,
                                                        int lane) {
  uint32_t n_bad = 0;
  [[maybe_unused]] uint32_t nc_np = 0;
  int first = -1;
  for (int p0 = 0; p0 < n; p0 += 64) {
    const int p = p0 + lane;
    bool bad = false;
    [[maybe_unused]] bool on_nc = false;
    if (p < n) {
      const int32_t pl = place[p];
      const uint32_t sp = (uint32_t)qp[p];
      const uint32_t kind = sp < (uint32_t)a.n_super ? a.pod_kind[sp] : 2u;
      if (kind != 2u) {
        if (pl == -1) {
          bad = true;
        } else if (kind == 0u && pl <= -2) {  // SimulateScheduling's UninitializedNodeError (deleting nodes' pods exempt)
          const uint32_t pos = (uint32_t)(-(pl + 2));
          bad = pos < (uint32_t)a.n_existing && a.pos_uninit[pos] != 0;
        }
        if constexpr (ON_NC) on_nc = pl >= 0;
      }
    }
    const uint64_t m = __ballot(bad);
    if (m) {
      n_bad += (uint32_t)__builtin_popcountll(m);
      if (first < 0) first = p0 + __builtin_ctzll(m);
    }
    if constexpr (ON_NC) nc_np += (uint32_t)__builtin_popcountll(__ballot(on_nc));
  }
  if constexpr (ON_NC) return Unscheduled{n_bad, first, nc_np};
  else return Unscheduled{n_bad, first, 0u};
}
__global__ __launch_bounds__(DRIFT_WAVES * 64) void drift_verdict_kernel(DriftArgs a) {
  const int lane = LANE;
  const int j = blockIdx.x * DRIFT_WAVES + (threadIdx.x >> 6);
  if (j >= a.n) return;  // (wave-uniform)
  const uint8_t* ar = a.arenas + a.stride * (size_t)j;
  const int32_t* place = reinterpret_cast<const int32_t*>(ar + a.off_place);
  const uint64_t* st = reinterpret_cast<const uint64_t*>(ar + a.off_stats);
  const int32_t* qp = a.qpod + (size_t)j * a.Pc;
  const int n = max(0, min(a.qlen[j], a.Pc));
  const Unscheduled u = scan_unscheduled<false>(a, place, qp, n, lane);
  const uint32_t n_bad = u.n_bad;
  const int first = u.first;
  if (lane == 0) {
    DriftOut o;
    o.feasible = n_bad == 0 ? 1 : 0;
    o.n_nodeclaims = (uint32_t)st[3];
    o.n_pods = (uint32_t)n;
    o.n_unscheduled = n_bad;
    o.first_unscheduled = -1;
    if (first >= 0) {
      const uint32_t sp = (uint32_t)qp[first];
      if (sp < (uint32_t)a.n_super) o.first_unscheduled = a.pod_cluster[sp];
    }
    o.blocked = 0;
    a.out[a.cidx[j]] = o;
  }
}
// One block per launch: the lowest caller-order index among the launch's feasible simulations (the launches are ordered
// longest-first, so this is not the launch-local index) with its launch-local index, and the sums of the Solves'
// counters. Every thread folds its simulations in index order and the tree is fixed, so the record does not depend on
// arrival order.
__global__ __launch_bounds__(DRIFT_FIRST_THREADS) void drift_first_kernel(DriftArgs a) {
  __shared__ int64_t s_first[DRIFT_FIRST_THREADS], s_run[DRIFT_FIRST_THREADS];
  __shared__ uint64_t s_sum[5][DRIFT_FIRST_THREADS];
  const int tid = threadIdx.x;
  int64_t first = INT64_MAX, run = INT64_MAX;  // first: caller index << 32 | launch-local index
  uint64_t sum[5] = {0, 0, 0, 0, 0};           // feasible, attempts, bytes, pops, cancelled
  for (int j = tid; j < a.n; j += DRIFT_FIRST_THREADS) {
    const uint64_t* st = reinterpret_cast<const uint64_t*>(a.arenas + a.stride * (size_t)j + a.off_stats);
    const int64_t c = a.cidx[j];
    const bool bad = st[7] != 0 || st[46] != 0;  // a Solve that did not finish has no verdict
    if (st[7] != 0 && c < run) run = c;
    sum[4] += st[46] != 0 ? 1 : 0;
    sum[1] += st[0];
    sum[2] += st[1];
    sum[3] += st[2];
    if (!bad && a.out[c].feasible) {
      sum[0]++;
      const int64_t key = (c << 32) | (int64_t)j;
      if (key < first) first = key;
    }
  }
  s_first[tid] = first;
  s_run[tid] = run;
  for (int k = 0; k < 5; k++) s_sum[k][tid] = sum[k];
  __syncthreads();
  for (int w = DRIFT_FIRST_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) {
      if (s_first[tid + w] < s_first[tid]) s_first[tid] = s_first[tid + w];
      if (s_run[tid + w] < s_run[tid]) s_run[tid] = s_run[tid + w];
      for (int k = 0; k < 5; k++) s_sum[k][tid] += s_sum[k][tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    DriftRec r;
    const bool any = s_first[0] != INT64_MAX;
    r.first = any ? (s_first[0] >> 32) : -1;
    r.local = any ? (s_first[0] & 0xFFFFFFFFll) : -1;
    r.feasible = s_sum[0][0];
    r.attempts = s_sum[1][0];
    r.bytes = s_sum[2][0];
    r.pops = s_sum[3][0];
    r.runaway = s_run[0] != INT64_MAX ? s_run[0] : -1;
    r.cancelled = s_sum[4][0];
    *a.rec = r;
  }
}
hipError_t launch_drift_verdict(const DriftArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(drift_verdict_kernel, dim3((a.n + DRIFT_WAVES - 1) / DRIFT_WAVES), dim3(DRIFT_WAVES * 64), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_drift_first(const DriftArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(drift_first_kernel, dim3(1), dim3(DRIFT_FIRST_THREADS), 0, s, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Command validation on general-path plans (kp_cluster_validate): behind solve_kernel (consolidation mode: the Solve
// ends at its second NodeClaim) and finalize_kernel in the launch's stream. validate_verdict_kernel, one wave per
// simulation, applies the rule of kp_abi.h to the arena: the AllNonPendingPodsScheduled scan drift_verdict_kernel runs
// (shared), the NodeClaim count from the stats word, and for a single NodeClaim its finalized option list as a type
// mask in LDS - Truncate's minValues check on it (minvalues_ok on the finalized requirements, as sim_kernel does), then
// the command's want row of that NodeClaim's catalogue against it. One 24-byte ValOut per simulation at the caller's
// index, lane w writes word w; validate_sum_kernel folds the launch's counters into one DriftRec (first, local and
// feasible unused). The launch downloads that record; the verdicts are read once at the end of the call.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DRIFT_WAVES * 64) void validate_verdict_kernel(ValidateArgs a) {
  __shared__ DevDict D;
  __shared__ uint64_t s_mask[DRIFT_WAVES][KP_MAX_TYPE_WORDS];
  __shared__ uint32_t s_scratch[DRIFT_WAVES][2 * KP_MAX_WORDS];
  block_copy(D, a.dict);
  __syncthreads();
  const int lane = LANE, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * DRIFT_WAVES + wave;
  if (j >= a.d.n) return;  // (wave-uniform; no block barrier below)
  const uint8_t* ar = a.d.arenas + a.d.stride * (size_t)j;
  const int32_t* place = reinterpret_cast<const int32_t*>(ar + a.d.off_place);
  const uint64_t* st = reinterpret_cast<const uint64_t*>(ar + a.d.off_stats);
  const int32_t* qp = a.d.qpod + (size_t)j * a.d.Pc;
  const int n = max(0, min(a.d.qlen[j], a.d.Pc));
  const uint32_t sub = (uint32_t)a.d.cidx[j];
  const Unscheduled u = scan_unscheduled<true>(a.d, place, qp, n, lane);
  uint32_t n_bad = u.n_bad;
  const uint32_t nc_np = u.nc_np;
  const uint32_t n_nc = (uint32_t)st[3];
  const bool repl = a.replace[sub] != 0;
  uint32_t verdict = KP_VALID, unsched = 0, missing = 0;
  if (n_nc > 1) {
    verdict = KP_INVALID_MULTIPLE;
  } else {
    int miss = 0;
    if (n_nc == 1) {
      const int32_t tmpl = *reinterpret_cast<const int32_t*>(ar + a.off_nct);
      const int cat = tmpl >= 0 && tmpl < a.n_tmpl ? a.tmpl_catalog[tmpl] : 0;
      const int nopt = (int)min(*reinterpret_cast<const uint32_t*>(ar + a.off_nopt), (uint32_t)a.opt_stride);
      const uint32_t* opts = reinterpret_cast<const uint32_t*>(ar + a.off_opts);
      uint64_t* msk = s_mask[wave];
      msk[lane] = 0;
      wave_sync();
      for (int q = lane; q < nopt; q += 64) {
        const uint32_t t = opts[q];
        if (t < (uint32_t)D.TW * 64u) atomicOr((unsigned long long*)&msk[t >> 6], 1ull << (t & 63));
      }
      wave_sync();
      const KReqs* R = reinterpret_cast<const KReqs*>(ar + a.off_ncr);
      const uint64_t v = lane < D.W ? R->vals[lane] : 0;
      const ReqView rv = stored_view(D, R, v);
      const uint64_t hmin = rv.hmin & rv.present;
      const DevCatalog& Cg = a.cats[cat];
      bool ok = true;  // Truncate(reqs, max): minValues must hold on the truncated options, else the NodeClaim's pods fail
      if (hmin) ok = minvalues_ok(D, Cg.code, Cg.TM, hmin, rv.minv, lane < D.TW ? msk[lane] : 0, s_scratch[wave]);
      if (!ok) n_bad += nc_np;
      const size_t row = (size_t)sub * a.n_catalogs + cat;
      const uint64_t want = lane < D.TW ? a.want[row * D.TW + lane] : 0;
      const uint64_t have = ok && lane < D.TW ? msk[lane] : 0;
      miss = wave_sum(__popcll(want & ~have)) + (int)a.unknown[row];
    }
    unsched = n_bad;
    if (unsched) verdict = KP_INVALID_UNSCHEDULED;
    else if (n_nc == 0) verdict = repl ? KP_INVALID_NO_REPLACEMENT_NEEDED : KP_VALID;
    else if (!repl) verdict = KP_INVALID_NEEDS_REPLACEMENT;
    else if (miss) verdict = KP_INVALID_NOT_SUBSET, missing = (uint32_t)miss;
  }
  const uint32_t w[6] = {verdict, n_nc > 1 ? 2u : n_nc, (uint32_t)n, unsched, missing, 0u};
  uint32_t mine = 0;
#pragma unroll
  for (int k = 0; k < 6; k++) mine = lane == k ? w[k] : mine;
  if (lane < 6) reinterpret_cast<uint32_t*>(a.out + sub)[lane] = mine;
}
// One block per launch: the Solves' counters, a Solve that exceeded its Queue.Pop bound, the ones that ended on the
// kp_cancel flag. Every thread folds its simulations in index order and the tree is fixed.
__global__ __launch_bounds__(DRIFT_FIRST_THREADS) void validate_sum_kernel(ValidateArgs a) {
  __shared__ int64_t s_run[DRIFT_FIRST_THREADS];
  __shared__ uint64_t s_sum[4][DRIFT_FIRST_THREADS];
  const int tid = threadIdx.x;
  int64_t run = INT64_MAX;
  uint64_t sum[4] = {0, 0, 0, 0};  // attempts, bytes, pops, cancelled
  for (int j = tid; j < a.d.n; j += DRIFT_FIRST_THREADS) {
    const uint64_t* st = reinterpret_cast<const uint64_t*>(a.d.arenas + a.d.stride * (size_t)j + a.d.off_stats);
    const int64_t c = a.d.cidx[j];
    if (st[7] != 0 && c < run) run = c;
    sum[0] += st[0];
    sum[1] += st[1];
    sum[2] += st[2];
    sum[3] += st[46] != 0 ? 1 : 0;
  }
  s_run[tid] = run;
  for (int k = 0; k < 4; k++) s_sum[k][tid] = sum[k];
  __syncthreads();
  for (int w = DRIFT_FIRST_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) {
      if (s_run[tid + w] < s_run[tid]) s_run[tid] = s_run[tid + w];
      for (int k = 0; k < 4; k++) s_sum[k][tid] += s_sum[k][tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    DriftRec r;
    r.first = -1;
    r.local = -1;
    r.feasible = 0;
    r.attempts = s_sum[0][0];
    r.bytes = s_sum[1][0];
    r.pops = s_sum[2][0];
    r.runaway = s_run[0] != INT64_MAX ? s_run[0] : -1;
    r.cancelled = s_sum[3][0];
    *a.d.rec = r;
  }
}
hipError_t launch_validate_verdict(const ValidateArgs& a, hipStream_t s) {
  if (a.d.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(validate_verdict_kernel, dim3((a.d.n + DRIFT_WAVES - 1) / DRIFT_WAVES), dim3(DRIFT_WAVES * 64), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(validate_sum_kernel, dim3(1), dim3(DRIFT_FIRST_THREADS), 0, s, a);
  return hipGetLastError();
}
