// kp_device.h — kernel argument blocks (host <-> device), plain pointers only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kp_model.h"

#define KP_SOLVE_STATS 48
// why the fast lane handed a popped pod to the full path (stats[32 + FB_*])
enum { FB_INELIGIBLE = 0, FB_SPILLED = 1, FB_SHIFT = 2, FB_SCAN = 3, FB_MERGE = 4, FB_MINVALUES = 5, FB_NONE = 6, FB_MEMO = 7 };

// The in-flight pre-check's view of one NodeClaim in one 64-byte line (one gather per candidate position instead of
// one per field): headroom = max allocatable over its types at creation minus its requests, for the first four
// requested resources (req_res_mask bit order; more are checked from nc_requests / nc_maxalloc), the exact failure
// memo's version, the taint set of its template.
struct NcHead {
  int64_t room[4];
  int32_t ver, taintset;
  int32_t pad_[6];
};

// One chunk of the spilled newNodeClaims order (solve_kernel's chunked mode): up to 64 NodeClaim ids in sorted order
// and their len(Pods).
struct ChkBlk {
  int32_t id[64];
  int32_t key[64];
};
#define CHK_MAXC 4096  // chunks (and blocks) of the chunked order; its directory lives in LDS
#define CHK_LDS_BYTES (CHK_MAXC * 14)  // the directory: start, info, block epochs (4 B each), free list (2 B)

struct SolveArgs {
  const DevDict* dict;
  const DevCatalog* cats;
  int32_t n_catalogs;
  const int64_t* vint;  // [W*64]
  // pods
  int32_t n_pods;
  const int32_t* pod_shape;      // [P]
  int32_t* pod_level;            // [P] relaxation level (mutable)
  int32_t* queue;                // [P] ring, pre-sorted byCPUAndMemoryDescending
  int32_t* lastlen;              // [P]
  int32_t* lastlen_epoch;        // [P]
  // shapes (x relaxation levels)
  const int32_t* shape_level_base;   // [S]
  const int32_t* shape_nlevels;      // [S]
  const uint8_t* shape_reqs;         // [SL] KReqs
  const uint64_t* shape_negop;       // [SL]
  const int64_t* shape_requests;     // [S][NRES]
  const uint64_t* shape_tolerates;   // [SL] bit ts: tolerates taint set ts (per level: toleratePreferNoScheduleTaints)
  const uint64_t* shape_pvp;         // rows of TW words
  const int32_t* pvp_base;           // [SL][n_catalogs] first row
  const int32_t* pvp_slot;           // [SL][64] row offset of key k (relative to base)
  const int32_t* sl_pvp_n;           // [SL] PVP rows of catalogue 0
  // templates
  int32_t n_tmpl;
  const uint8_t* tmpl_reqs;          // [NT] KReqs
  const int32_t* tmpl_taintset;      // [NT]
  const int32_t* tmpl_catalog;       // [NT]
  const uint64_t* tmpl_X;            // [NT][TW] InstanceTypeOptions after NewScheduler's pre-filter
  const int64_t* tmpl_daemon;        // [NT][NRES]
  const uint32_t* tmpl_limit_present;// [NT]
  int64_t* tmpl_remaining;           // [NT][NRES] (mutable)
  // existing nodes (upstream order)
  int32_t n_existing;
  uint8_t* ex_reqs;                  // [E] KReqs (mutable)
  // batched simulations: the existing nodes' requirements copy-on-write. ex_reqs_ro = the pristine [E] KReqs (shared by
  // every simulation), ex_own = [ceil(E/64)] bits, set once the simulation wrote its own copy into ex_reqs (store_merged
  // writes a complete set: no copy first). ex_reqs_ro null: ex_reqs is complete (single Solves restore it per run).
  const uint8_t* ex_reqs_ro;
  uint64_t* ex_own;
  // batched simulations: per shape-level the existing positions that can ever pass its count-independent checks
  // (headroom, taints, static check, host ports on the superset's pristine state; nodes only fill up and a simulation
  // only excludes nodes), ascending: ex_ulist[ex_ulist_off[sl] .. ex_ulist_off[sl + 1]), and ex_uidx[sl][e] = the first
  // list index whose position is >= e. The full path's addToExistingNode scans the list instead of every position.
  // Null: scan every position.
  const int32_t* ex_ulist;
  const int32_t* ex_ulist_off;
  const int32_t* ex_uidx;
  const int32_t* ex_taintset;        // [E]
  const int64_t* ex_available;       // [E][NRES]
  int64_t* ex_requests;              // [E][NRES] (mutable)
  int64_t* ex_room;                  // [4][E] available - requests of the first four requested resources (mutable;
                                     // INT64_MAX past the requested ones)
  // in-flight NodeClaims (capacity n_pods)
  uint8_t* nc_reqs;                  // [P] KReqs
  uint64_t* nc_X;                    // [P][TW]
  int64_t* nc_requests;              // [P][NRES]
  int32_t* nc_tmpl;                  // [P]
  int32_t* g_npods;                  // [P] len(Pods)
  int32_t* g_order;                  // [P] newNodeClaims order
  int32_t sort_in_lds;               // unused (LDS until SORT_CAP NodeClaims, then global)
  int32_t sort_cap;
  // past sort_cap NodeClaims the order is chunked (chk_blk, directory in LDS); when the directory is full (or
  // chk_maxc == 0) it falls back to the flat global arrays g_order / g_npods
  ChkBlk* chk_blk;                   // [CHK_MAXC]
  int32_t* chk_dead;                 // [chk_dead_rows][CHK_MAXC] per (shape-level, block): the block's insertion epoch
                                     // when every NodeClaim in it failed the shape-level permanently (-1 none)
  int32_t chk_dead_rows;             // shape-levels < this keep dead marks
  int32_t chk_maxc;                  // chunks the directory may use (<= CHK_MAXC; a test hook lowers it)
  // exact failure memo: outcome of Add/CanAdd depends only on (candidate state, pod shape-level), so a
  // recorded failure stays valid while the candidate's version is unchanged
  int32_t ncc;                       // NodeClaim ids < ncc are memoised
  NcHead* nc_head;                   // [P] pre-check record (version, taint set, headroom), written at creation
  int32_t* nc_fail;                  // [SL][ncc]
  int32_t* ex_ver;                   // [E]
  int32_t* ex_fail;                  // [SL][E]
  int32_t* tmpl_ver;                 // [NT] bumped when the template's remaining limits change (subtractMax)
  int32_t* tmpl_fail;                // [SL][NT] NC_NEVER: the template fails the shape-level for good
  uint64_t* tmpl_xlim;               // [NT][TW] the template's options after filterByRemainingResources ...
  int32_t* tmpl_xlim_ver;            // [NT] ... as of this tmpl_ver (-1: never computed)
  int64_t* nc_maxalloc;              // [P][NRES] max allocatable over the NodeClaim's types at creation
  int32_t* nc_fitj;                  // [P][NRES] threshold index of the last Fits per resource
  int32_t* nc_cat;                   // [P] catalogue of the NodeClaim's template
  uint32_t req_res_mask;             // resources some pod shape requests (> 0)
  int32_t timing;                    // 1: thread 0 accumulates per-phase s_memtime deltas into stats[8..15]
  int32_t stop_nc;                   // > 0 (consolidation simulations): end the Solve once this many NodeClaims exist
  const int32_t* cancel;             // kp_cancel flag (host-mapped, polled every ~1024 pops), NULL: none
  int32_t cont;                      // the fast lane variant: 1 with the continuation round and the run-length commit
                                     // (queue runs of one shape), 2 with the run-length commit alone (runs of shapes
                                     // with one request row), 3 as 2 with the open set's sequential loop in place of the
                                     // closed-form commit (runs across several NodeClaims being filled), 0 neither
  // topology spread (upstream Topology, TopologyTypeSpread groups). A group on a dictionary key keeps a
  // count per value ordinal and the mask of registered domains; a hostname group a saturating u8 count per
  // node (existing positions: hcnt_ex, NodeClaim ids: hcnt_nc).
  int32_t n_groups;
  const int32_t* tg_key;             // [G] dictionary key, -1: hostname
  const int32_t* tg_row;             // [G] row of a hostname group in hcnt_*, -1 otherwise
  const int32_t* tg_maxskew;         // [G]
  const int32_t* tg_mindom;          // [G] minDomains, 0: nil
  const int32_t* tg_aff;             // [G] node filter has an affinity term (NodeAffinityPolicy Honor)
  const int32_t* tg_term_base;       // [G] its first term in tg_terms
  const int32_t* tg_nterm;           // [G] its terms (ORed: MakeTopologyNodeFilter over the required terms)
  int32_t* tg_live;                  // [G] 1: the group exists (mutable: a relaxation's Topology.Update makes it)
  const uint64_t* tg_filt_tol;       // [G] bit ts: node filter admits taint set ts (NodeTaintsPolicy)
  const uint8_t* tg_terms;           // KReqs
  const uint64_t* tg_terms_negop;
  int32_t* tg_cnt;                   // [G][64] (mutable)
  uint64_t* tg_reg;                  // [G] (mutable)
  uint8_t* hcnt_ex;                  // [GH][E] (mutable)
  uint8_t* hcnt_nc;                  // [GH][hnc_stride] (zeroed per run)
  int32_t hnc_stride;
  const int32_t* shape_rec_base;     // [S] groups that select the shape's pods (Topology.Record)
  const int32_t* shape_rec_n;        // [S]
  const int32_t* rec_list;
  const int32_t* sl_own_base;        // [SL] groups the shape-level owns (AddRequirements)
  const int32_t* sl_own_n;           // [SL] (<= 8)
  const int32_t* own_group;
  const int32_t* own_self;           // the group's selector matches the owner pod
  const uint64_t* own_pd;            // podDomains (strict requirements) over the key's value ordinals
  const int32_t* rec_aux;            // per rec_list entry: hostname row, else -1 - key slot (static)
  const int32_t* sl_fast_topo;       // [SL] 1: the fast lane may place the level's pods
  const int4* own_rec;               // [O][2] group, self, key, maxSkew | minDomains, row, key slot, 0 (static)
  const uint64_t* sl_topo_keys;      // [SL] dictionary keys of the owned groups
  const int32_t* sl_stage;           // [SL][64] the fast lane's stage record (topology Solves; kp_host StageRecords)
  // first-fit cursors (exact): cur_*[sl] = {k, t}: the first k candidates of the scan order were known to
  // fail for shape-level sl at mutation time t; a mutation stack (t, position, in LDS) clamps k to the lowest
  // position changed since (monotone stack: suffix minimum by binary search). Shape-levels that own
  // topology groups do not use them (their outcome depends on the counts).
  int32_t* cur_nc;                   // [SL][2] in-flight NodeClaims (positions in the sorted order)
  int32_t* cur_ex;                   // [SL][2] existing nodes (upstream order)
  // [SL] unschedulable memo: the NodeClaim count when a pod of the shape-level last failed every placement (-1:
  // never). Without topology or reservations and with no positive custom key at the level, every failure is
  // permanent (existing nodes and NodeClaims only fill up and narrow, limits only shrink as NodeClaims are created),
  // so a later pod of the level fails again exactly while no NodeClaim was created since
  int32_t* sl_fail;
  int32_t n_tk;                      // topology keys (dictionary keys some group spreads over)
  const int32_t* tk_keys;            // [TK]
  uint8_t* nc_tcode;                 // [TK][hnc_stride] pinned value ordinal per NodeClaim (store_tcodes)
  const uint8_t* ex_static_ok;       // [E] every unrequested resource fits and nothing available is negative
  int32_t n_req_res;                 // popcount(req_res_mask)
  const int32_t* tkey_slot;          // [64] row of a topology key in ex_tcode
  const uint8_t* ex_tcode;           // [TK][E] value ordinal of the existing node's label (0xFF: none)
  // host ports (upstream HostPortUsage, one bit per distinct port entry of the batch): a candidate conflicts when
  // its used bits meet the pod's conflict mask; a placement ORs in the pod's add mask (used bits only grow)
  int32_t hp_any;                    // some shape or existing node names a host port
  const uint64_t* shape_hp_conf;     // [S]
  const uint64_t* shape_hp_add;      // [S]
  uint64_t* ex_hp;                   // [E] (mutable)
  uint64_t* nc_hp;                   // [P] set when the NodeClaim is created
  // precomputed template options per (shape-level, template) (tmpl_feas_kernel), or null
  const uint64_t* tfeas;             // [SL][NT] entries of tfeas_words
  int32_t tfeas_words;
  // outputs
  int32_t* placement;                // [P]
  int32_t* events;                   // [P] pods in placement order
  uint64_t* stats;                   // [KP_SOLVE_STATS]: attempts, bytes, pops, n_nc, n_events, scanned, starts; [7] runaway;
                                     // [8..15] phases, [16..23] attempt split, [24] fast-lane pods, [25..30] fast-lane
                                     // cycles, [31] literal pdqsorts, [32..39] fast-lane hand-offs by reason (FB_*),
                                     // [40] pops whose addToNewNodeClaim failed on a ReservedOfferingError
  // capacity reservations (upstream ReservationManager + NodeClaim.reserveOfferings): res_mode 0 none, 1 fallback,
  // 2 strict. A reservation id is one offering class (res_cls); its remaining capacity lives in LDS during the Solve,
  // starting from res_cap0; nc_held[nc] = the classes NodeClaim nc holds (zeroed per run)
  int32_t res_mode;
  int32_t rqc_empty;                 // requirement class of the empty requirement set (see sl_rqc), -1: none
  uint64_t res_cls;
  uint64_t* nc_held;                 // [P]
  // [S] request class (the fast lane's run-length commit): equal iff the shapes' request rows are equal over all
  // KP_NRES entries; a shape with host ports (shape_hp_conf != 0) has a class of its own
  const int32_t* shape_rclass;
  // requirement classes: sl_rqc[sl] = the class of shape-level sl, equal iff the levels' compiled requirements (KReqs
  // bytes, negop, PVP rows) are equal; the members of class c are rqc_mem[rqc_off[c] .. rqc_off[c + 1]). Intersecting a
  // requirement set into a NodeClaim a second time changes nothing, so a merge of one member tags every member merged
  // on that NodeClaim (nc_fail NC_MERGED), and a permanent failure of Compatible fails every member (NC_NEVER). A
  // shape with host ports, and every level of a Solve with topology groups, is a class of its own.
  const int32_t* sl_rqc;             // [SL]
  const int32_t* rqc_off;            // [classes + 1]
  const int32_t* rqc_mem;            // [SL]
  int32_t res_cap0[KP_MAX_CLASSES];
};

// tmpl_feas_kernel: rows [row_lo, row_hi) of shape-levels x every template
struct TfeasArgs {
  const DevDict* dict;
  const DevCatalog* cats;
  int32_t n_catalogs;
  const int64_t* vint;
  int32_t n_tmpl;
  const uint8_t* tmpl_reqs;
  const int32_t* tmpl_catalog;
  const uint64_t* tmpl_X;
  const int64_t* tmpl_daemon;
  const uint8_t* shape_reqs;         // [SL] KReqs
  const uint64_t* shape_negop;       // [SL]
  const int32_t* sl_shape;           // [SL] shape of the shape-level
  const int64_t* shape_requests;     // [S][NRES]
  const uint64_t* shape_pvp;
  const int32_t* pvp_base;
  const int32_t* pvp_slot;
  const int32_t* sl_own_n;
  uint32_t req_res_mask;
  int32_t row_lo, row_hi;
  int32_t words;                     // u64 per entry: TW + KP_NRES / 2 + 1
  uint64_t* out;                     // [SL][NT] entries (this call writes rows [row_lo, row_hi))
};
hipError_t launch_tmpl_feas(const TfeasArgs& a, hipStream_t s);

// The explanation step behind a Solve (kp_solve_run_explained): why addToNewNodeClaim fails, per NodePool template, for
// the shape-levels the Solve left pods of unscheduled, at the state solve_kernel ended in. One record per (shape-level,
// template); mirrors kp_pool_reason's numeric half (codes: enum kp_why).
struct ExplainRec {
  int32_t code;
  int32_t n_types;      // the template's options after filterByRemainingResources
  int32_t n_req, n_fits, n_off;  // options passing one criterion alone: Intersects / Fits / an available offering
  int32_t n_rf, n_ro, n_fo;      // ... each pair
  int32_t n_remaining;  // ... all three
  int32_t pad_;
  uint64_t keys;        // KP_WHY_REQUIREMENTS: the dictionary keys Compatible fails on
};
struct ExplainArgs {
  const DevDict* dict;
  const DevCatalog* cats;
  int32_t n_catalogs;
  const int64_t* vint;
  // the Solve's final state (read only)
  int32_t n_pods;
  const int32_t* pod_shape;          // [P]
  const int32_t* pod_level;          // [P]
  const int32_t* placement;          // [P]
  const int64_t* tmpl_remaining;     // [NT][NRES]
  const int32_t* tg_cnt;             // [G][64]
  const uint64_t* tg_reg;            // [G]
  // the batch (as SolveArgs / TfeasArgs)
  int32_t n_sl, n_tmpl;
  const int32_t* shape_level_base;   // [S]
  const int32_t* sl_shape;           // [SL]
  const uint8_t* shape_reqs;         // [SL] KReqs
  const uint64_t* shape_negop;       // [SL]
  const uint64_t* shape_tolerates;   // [SL]
  const int64_t* shape_requests;     // [S][NRES]
  const uint64_t* shape_pvp;
  const int32_t* pvp_base;
  const int32_t* pvp_slot;
  const uint8_t* tmpl_reqs;
  const int32_t* tmpl_taintset;
  const int32_t* tmpl_catalog;
  const uint64_t* tmpl_X;
  const int64_t* tmpl_daemon;
  const uint32_t* tmpl_limit_present;
  const int32_t* sl_own_base;        // [SL]
  const int32_t* sl_own_n;           // [SL] (<= 8)
  const int4* own_rec;
  const uint64_t* own_pd;
  const uint64_t* sl_topo_keys;      // [SL]
  uint32_t req_res_mask;
  // outputs: the only words the two kernels write
  uint8_t* mark;                     // [SL] 1: some unscheduled pod ended at this shape-level (zeroed before the launch)
  int32_t* pod_row;                  // [P] the pod's shape-level when it is unscheduled, else -1
  ExplainRec* rec;                   // [SL][NT], rows of marked shape-levels only
};
hipError_t launch_explain(const ExplainArgs& a, hipStream_t s);

struct FinalizeArgs {
  const DevDict* dict;
  const DevCatalog* cats;
  const int64_t* vint;
  int32_t n_nc;
  const int32_t* nc_tmpl;
  const int32_t* tmpl_catalog;
  const uint8_t* nc_reqs;
  const uint64_t* nc_X;
  int32_t max_types;
  int32_t opt_stride;
  uint32_t* out_options;     // [n_nc][opt_stride]
  uint32_t* out_n_remaining; // [n_nc]
  uint32_t* out_n_options;   // [n_nc]
  const uint64_t* nc_held;   // [n_nc] reservation classes held (FinalizeScheduling: reservation-id In {..}), or null
  const uint64_t* solve_stats;  // batched finalize: the Solve's stats (n_nc = [3]); unused otherwise
};

// batch_init_kernel: per-arena initialisation of batched Solves (pristine copy + byte fills)
constexpr int BATCH_INIT_FILLS = 12;
struct BatchInitArgs {
  uint8_t* base;
  size_t stride;
  const uint8_t* pristine;
  size_t dst_off, n_copy;  // [dst_off, dst_off + n_copy) of every arena from pristine
  size_t skip_off, skip_len;  // except [dst_off + skip_off, + skip_len) (16-byte multiples; 0: none)
  int32_t n_fill;
  uint32_t fill_byte[BATCH_INIT_FILLS];
  size_t fill_off[BATCH_INIT_FILLS], fill_len[BATCH_INIT_FILLS];
};

struct FeasArgs {
  const DevDict* dict;
  const DevCatalog* cat;
  const int64_t* vint;
  int32_t T;
  int32_t n_queries;
  int32_t mode_compatible;   // 1: Compatible(q, type, WK) (CompatibleAvailableFilter); 0: type.Intersects(q)
  int32_t pad_;              // bits kernel: bit 0 = write the cheapest-price stream with non-temporal stores
  const uint8_t* q_reqs;     // [Q] KReqs
  const int64_t* q_requests; // [Q][NRES]
  uint64_t* out_mask;        // [Q][tiles]
  double* out_cheapest;      // [Q][ch_stride] (the first T of each row) or null
  int32_t bits;              // 1: bitsets over the catalogue (feasibility_quad_kernel when T <= 1024, else
                             // feasibility_bits_kernel), 0: feasibility_kernel
  int32_t blocks;            // its grid (rows are strided over the waves)
  int32_t one_row;           // 1: feasibility_bits_kernel at any T (its cross-check, KP_FEAS_ONE_ROW)
  int32_t ch_stride;         // doubles per out_cheapest row: T rounded up to whole 128-byte lines (rows start aligned)
  uint64_t* out_classes;     // [Q] compact result: the row's compatible offering classes (kp_filter_run_compact), or null
};

// ---- launch-side selection (kp_launch_select) ------------------------------------------------------
#define LAUNCH_CAP 1024  // instance types per request on the device path
struct LaunchOut {  // kp_launch_result as the device writes it
  int32_t status, capacity_type;
  uint32_t n_types, n_overrides;
  int32_t failed_filter;
  uint32_t n_compatible, rejected_exotic, rejected_spot;
  int32_t od_fallback_warning, reservation_type;
  uint32_t rejected_reservation;
  int32_t pad_;
};
struct LaunchArgs {
  const DevDict* dict;
  const DevCatalog* cat;
  const int64_t* vint;
  int32_t n;                  // requests
  int32_t max_types;          // Truncate limit (0: none)
  int32_t spot_bit, od_bit;   // dictionary value bits of karpenter.sh/capacity-type spot / on-demand (-1: absent)
  int32_t ct_key;             // dictionary key of karpenter.sh/capacity-type
  int32_t MO;                 // offerings per type (stride of ofs_cls)
  uint64_t cls_spot, cls_od;  // offering classes whose capacity type is spot / on-demand
  int32_t res_bit, pad0_;     // dictionary value bit of karpenter.sh/capacity-type reserved (-1: absent)
  uint64_t cls_res;           // offering classes whose capacity type is reserved
  uint64_t cls_rt0, cls_rt1;  // classes whose capacity-reservation-type is default / capacity-block
  const double* price_all;    // [T][C] cheapest offering of each class, any availability (CapacityBlockFilter)
  const int32_t* rcap;        // [T][C] greatest reservation capacity over the class's available offerings
  const uint8_t* q_reqs;      // [n] KReqs
  const int64_t* q_requests;  // [n][NRES]
  const uint32_t* list_off;   // [n+1] CSR of the requests' instance-type lists
  const uint32_t* list;
  const uint64_t* exotic;     // [TW] ExoticInstanceTypeFilter's exotic types (metal size or accelerator capacity)
  const int8_t* cls_zone;     // [C] index of the class's zone in the subnet zones, -1: no subnet
  const uint8_t* ofs_cls;     // [T][MO] offering classes of each type in offering order, 0xFF: end
  uint32_t ovr_stride;        // out_overrides entries per request
  LaunchOut* out;
  uint32_t* out_types;        // [n][max_types]
  uint32_t* out_overrides;    // [n][ovr_stride]
  uint64_t* stats;            // [2]: types evaluated, algorithmic bytes
};
hipError_t launch_launch(const LaunchArgs& a, hipStream_t s);

// ---- consolidation simulations (kp_cluster_simulate) -------------------------------------------
// One in-flight NodeClaim (a simulation with a second one is a no-op, so it stops there).
struct SimNC {
  KReqs reqs;
  uint64_t X[KP_MAX_TYPE_WORDS];
  int64_t requests[KP_NRES];
  int64_t maxalloc[KP_NRES];
  int32_t fitj[KP_NRES];
  int32_t tmpl, taintset, ver, pad_;
  uint64_t hp;  // used host-port bits
};

// kp_sim_result as the device writes it (same layout as the ABI struct)
struct SimOut {
  int32_t decision;
  uint32_t nodepool;
  double candidate_price, replacement_price, savings;
  uint32_t n_options, n_pods;
};

struct SimArgs {
  const DevDict* dict;
  const DevCatalog* cats;
  int32_t n_catalogs;
  int32_t SL;                        // shape-levels
  const int64_t* vint;
  // shapes (x relaxation levels), as in SolveArgs
  const int32_t* shape_level_base;
  const int32_t* shape_nlevels;
  const int32_t* sl_shape;           // [SL] shape of a shape-level
  const uint8_t* shape_reqs;
  const uint64_t* shape_negop;
  const int64_t* shape_requests;
  const uint64_t* shape_tolerates;
  const uint64_t* shape_pvp;
  const int32_t* pvp_base;
  const int32_t* pvp_slot;
  // templates
  int32_t n_tmpl;
  const uint8_t* tmpl_reqs;
  const int32_t* tmpl_taintset;
  const int32_t* tmpl_catalog;
  const int32_t* tmpl_nodepool;
  const uint64_t* tmpl_X;
  const int64_t* tmpl_daemon;
  const uint32_t* tmpl_limit_present;  // [NT] NodePool limits: filterByRemainingResources for the new NodeClaim
  const int64_t* tmpl_remaining;       // [NT][NRES]
  // existing nodes in upstream order (initialized first, then name); position e
  int32_t E, EW;
  const uint16_t* ex_code;           // [K][E] value bit of the node's label for key k, 0xFFFF: no label
  const int32_t* ex_taintset;        // [E]
  const int64_t* ex_available;       // [E][NRES]
  const int64_t* ex_requests;        // [E][NRES]
  const uint8_t* ex_init;            // [E]
  // host ports (see SolveArgs): static used bits per node; touched nodes keep theirs in s_ovlhp
  int32_t hp_any;
  const uint64_t* shape_hp_conf;     // [S]
  const uint64_t* shape_hp_add;      // [S]
  const uint64_t* ex_hp;             // [E]
  uint64_t* s_ovlhp;                 // [slot][E] (valid where the node is touched)
  // precomputed per shape-level (sim_prep_kernel / sim_usable_kernel)
  uint64_t* usable;                  // [SL][EW] CanAdd on the snapshot: tolerated, compatible, fits
  SimNC* tres;                       // [SL] addToNewNodeClaim outcome (tmpl -1: none)
  // pods every simulation schedules besides those of S: the deleting nodes' and the pending ones
  const uint64_t* base_excl;         // [EW] deleting nodes (never destinations)
  const uint32_t* base_keys;         // [n_base] their queue ranks
  int32_t n_base;
  const uint8_t* pod_kind;           // [P] 0 on a node, 1 on a deleting node, 2 pending
  // pods (all pods of the cluster)
  const int32_t* pod_shape;          // [P]
  const uint32_t* pod_rank;          // [P] position in byCPUAndMemoryDescending order
  const uint32_t* rank_pod;          // [P]
  // cluster nodes, input order
  const int32_t* node_pos;           // [N] existing position
  const uint32_t* node_pod_off;      // [N+1]
  const uint32_t* node_pods;
  const double* node_price;          // [N] cheapest label-compatible offering of its type
  const uint8_t* node_flags;         // [N] bit0 priced, bit1 capacity-type label = spot
  const uint32_t* node_name;         // [N] type-name id
  const uint32_t* type_name;         // [n_catalogs][T] type-name id
  int32_t spot_bit, od_bit, ct_key;
  uint32_t req_res_mask;
  int32_t RU;                        // requested resources (popcount of req_res_mask)
  int8_t ru_res[KP_NRES];            // resource of overlay column u
  int32_t max_types;
  int32_t multi_node;
  int32_t spot_to_spot;              // SpotToSpotConsolidation feature gate
  int32_t wave_lds;                  // dynamic LDS bytes per wave (bitmaps + pod queue / option sort)
  // batch
  int32_t n_subsets;
  const uint32_t* sub_off;
  const uint32_t* sub_nodes;
  int32_t cap;                       // pods per simulation the LDS region holds
  int32_t cap2;                      // power of two >= max(cap, 2 * sorted types)
  // per-wave scratch (slot = global wave id)
  int32_t n_slots;
  uint64_t* s_pod;                   // [slot][cap] epoch<<40 | level<<32 | lastLen
  int32_t* s_start;                  // [slot][SL] first existing position not yet known to fail
  int64_t* s_ovl;                    // [slot][E][RU] requests of existing nodes touched by the simulation
  SimNC* s_nc;                       // [slot]
  int32_t* s_ncfail;                 // [slot][SL]
  SimOut* out;                       // [n_subsets]
  uint64_t* stats;                   // [8] attempts, bytes, pops, existing words scanned, -, cancelled
  const int32_t* cancel;             // kp_cancel flag (host-mapped) or null: polled between a wave's subsets
};

// sim_kernel's second argument: SimAll walks every subset of the batch, SimLive (the budget-gated instantiation) the
// admissible ones, ascending
struct SimAll {
  static constexpr bool gated = false;
  static constexpr bool emit = false;
  static constexpr bool check = false;
  static constexpr bool why = false;
  static constexpr const uint32_t* live = nullptr;
};
struct SimLive {
  static constexpr bool gated = true;
  static constexpr bool emit = false;
  static constexpr bool check = false;
  static constexpr bool why = false;
  const uint32_t* live;
};
// The emitting instantiation (kp_cluster_command): gated as SimLive, and every simulation also leaves the command it
// decided on in its subset's record, rec + stride * subset: a SimCmdHdr, then three [cap] arrays over the simulation's
// queue positions (the order its pods were sorted into): the pod's global queue rank (uint32), its placement at commit
// (int32: 0 the NodeClaim, <= -2 existing position -2 - p, -1 never placed), and the NodeClaim's add order (uint32 queue
// positions, n_added of them). Each word has one writer and is a plain vector store.
#define SIM_CMD_OPTS 128  // >= SimArgs.max_types (100): the two 64-lane halves of the truncated option list
struct SimCmdHdr {
  int32_t tmpl;          // REPLACE: the NodeClaim's template
  uint32_t n_remaining;  // its instance-type options before truncation
  uint32_t n_kept;       // options[] entries: what the price filters (and the spot-to-spot cut) kept, price order
  uint32_t s2s;          // the decision was taken as spot-to-spot
  uint32_t n_queue;      // pods the simulation queued (every decision)
  uint32_t n_added;      // pods the NodeClaim took (every decision)
  uint32_t pad_[2];
  uint32_t options[SIM_CMD_OPTS];
  int64_t requests[KP_NRES];
  KReqs reqs;
};
struct SimEmit {
  static constexpr bool gated = true;
  static constexpr bool emit = true;
  static constexpr bool check = false;
  static constexpr bool why = false;
  const uint32_t* live;
  uint8_t* rec;
  size_t stride;  // sim_cmd_stride(cap)
};
// The checking instantiation (kp_cluster_validate): gated as SimEmit (the identity list without budgets). A simulation
// takes no consolidation decision: it runs to its end (a candidate pod on an uninitialized node is counted, not a
// stop), and one that made exactly one NodeClaim tests the caller's options - want, one type bitmask of TW words per
// (subset, catalogue), names resolved on the host; unknown the count of names that catalogue does not hold - against
// the NodeClaim's whole truncated option list. It leaves one ValOut (kp_validation) at the caller's subset index: six
// words, lane w writes word w, plain vector stores.
struct ValOut {
  int32_t verdict;
  uint32_t n_nodeclaims, n_pods, n_unscheduled, n_missing, blocked;
};
struct SimCheck {
  static constexpr bool gated = true;
  static constexpr bool emit = false;
  static constexpr bool check = true;
  static constexpr bool why = false;
  const uint32_t* live;
  const uint64_t* want;     // [n_subsets][n_catalogs][TW]
  const uint32_t* unknown;  // [n_subsets][n_catalogs]
  const uint8_t* replace;   // [n_subsets] 1: the command carries a replacement
  uint32_t* val;            // [n_subsets] ValOut
};
// The explaining instantiation (kp_cluster_simulate_explained): gated as SimLive (the identity list without budgets),
// decides as SimLive decides and also leaves, at the caller's subset index, which exit of computeConsolidation the
// simulation took: one WhyOut (kp_sim_why), twelve words, lane w writes word w, plain vector stores. Like SimCheck it
// counts a candidate pod on an uninitialized node and goes on, and truncates whatever the candidates' prices and the
// spot-to-spot gate say (Truncate's minValues check is the Solve's, so it is judged before either); unlike SimCheck it
// then runs the price stages.
struct WhyOut {
  int32_t reason, stage;
  uint32_t n_nodeclaims, n_unscheduled;
  int32_t first_unscheduled, unpriced;
  uint32_t n_truncated, n_cheaper, n_same_type, reserved_;
  double cheapest_launch;
};
#define WHY_WORDS 12
static_assert(sizeof(WhyOut) == 4 * WHY_WORDS, "WhyOut is twelve words");
struct SimWhy {
  static constexpr bool gated = true;
  static constexpr bool emit = false;
  static constexpr bool check = false;
  static constexpr bool why = true;
  const uint32_t* live;
  uint32_t* rec;  // [n_subsets] WhyOut
};
// why_count_kernel: the histogram of the records' reasons in two stages (blocks count contiguous ranges, one block
// sums the partials; integers, no atomics). A subset the budget gate blocked (gate[s] == 0; gate null: none) was not
// simulated: the first stage writes its KP_UNCONS_BUDGET record.
#define WHY_REASONS 10
#define WHY_COUNT_THREADS 256
#define WHY_COUNT_MAX_BLOCKS 64
hipError_t launch_why_count(uint32_t* rec, const uint8_t* gate, int n, uint64_t* part, uint64_t* counts, hipStream_t s);
inline int why_count_blocks(int n) {
  const int b = (n + WHY_COUNT_THREADS - 1) / WHY_COUNT_THREADS;
  return b < 1 ? 1 : (b > WHY_COUNT_MAX_BLOCKS ? WHY_COUNT_MAX_BLOCKS : b);
}
inline size_t sim_cmd_stride(int cap) { return (sizeof(SimCmdHdr) + (size_t)12 * cap + 15) & ~(size_t)15; }
// budget gate over the resident CSR batch (budget_gate_kernel, gate_scan_kernel, gate_scatter_kernel)
#define GATE_WAVES 4
#define GATE_PER_WAVE 16
#define GATE_BLOCK (GATE_WAVES * GATE_PER_WAVE)  // subsets per block, contiguous
#define GATE_MAX_POOLS 256
struct GateArgs {
  int32_t n_subsets;
  int32_t n_pools;                   // <= GATE_MAX_POOLS
  int32_t n_nodes;                   // N
  const uint32_t* sub_off;           // [n_subsets + 1]
  const uint32_t* sub_nodes;
  const uint16_t* node_pool;         // [N], every member's entry < n_pools (checked on the host)
  const uint32_t* allowed;           // [n_pools] KP_BUDGET_UNLIMITED: no limit
  uint8_t* gate;                     // [n_subsets] 1 admissible, 0 blocked
  SimOut* out;                       // blocked subsets: the zero no-op
  uint32_t* blk_cnt;                 // [n_blocks] admissible subsets of the block
  uint32_t* blk_off;                 // [n_blocks] exclusive scan of blk_cnt
  uint32_t* live;                    // [n_subsets] ascending admissible subset indices
  uint32_t* n_live;                  // [1]
};
hipError_t launch_budget_gate(const GateArgs& g, hipStream_t s);

// Drift (kp_cluster_drift): the verdict of every simulation of a general-path launch, and the launch's record.
// DriftOut mirrors kp_drift_result.
struct DriftOut {
  int32_t feasible;
  uint32_t n_nodeclaims, n_pods, n_unscheduled;
  int32_t first_unscheduled;
  uint32_t blocked;
};
// drift_first_kernel's record of one launch (the host combines the few launches' records)
struct DriftRec {
  int64_t first;      // lowest caller-order subset index among the launch's feasible simulations, -1: none
  int64_t local;      // that simulation's index in the launch, -1
  uint64_t feasible;  // feasible simulations
  uint64_t attempts, bytes, pops;  // the Solves' counters, summed
  int64_t runaway;    // caller-order index of a simulation that exceeded its Queue.Pop bound, -1: none
  uint64_t cancelled; // simulations that ended on the kp_cancel flag
};
#define DRIFT_WAVES 4
#define DRIFT_FIRST_THREADS 256
struct DriftArgs {
  int32_t n;                     // simulations of the launch
  int32_t Pc;                    // queue positions an arena holds (stride of qpod)
  int32_t n_existing;            // E: existing positions of the superset Solve
  int32_t n_super;               // pods of the superset Solve
  const uint8_t* arenas;         // the launch's arenas
  size_t stride;                 // bytes per arena
  size_t off_place, off_stats;   // the Solve's placements [Pc] and stats [KP_SOLVE_STATS] within an arena
  const int32_t* qpod;           // [n][Pc] superset pod of each queue position
  const int32_t* qlen;           // [n] pods queued
  const int32_t* cidx;           // [n] caller-order subset index
  const uint8_t* pod_kind;       // [n_super] 2 pending, 1 a deleting node's, 0 a node's (per plan)
  const int32_t* pod_cluster;    // [n_super] cluster pod index (per plan)
  const uint8_t* pos_uninit;     // [E] 1: the existing position's node is not initialized (per plan)
  DriftOut* out;                 // [n_subsets] caller order
  DriftRec* rec;                 // [1] this launch's record
};
// kp_cluster_validate on general-path plans: validate_verdict_kernel and validate_sum_kernel behind a launch's
// solve_kernel and finalize_kernel (d.out unused; d.rec: the launch's counters)
struct ValidateArgs {
  DriftArgs d;
  size_t off_nct, off_nopt, off_opts, off_ncr;  // NodeClaim 0 within an arena: template, option count, options, final KReqs
  int32_t opt_stride;            // options an arena holds per NodeClaim
  int32_t n_tmpl, n_catalogs;
  const DevDict* dict;
  const DevCatalog* cats;
  const int32_t* tmpl_catalog;   // [n_tmpl]
  const uint64_t* want;          // [n_subsets][n_catalogs][TW], caller order (as SimCheck)
  const uint32_t* unknown;       // [n_subsets][n_catalogs]
  const uint8_t* replace;        // [n_subsets]
  ValOut* out;                   // [n_subsets] caller order
};
hipError_t launch_validate_verdict(const ValidateArgs& a, hipStream_t s);
hipError_t launch_drift_verdict(const DriftArgs& a, hipStream_t s);
hipError_t launch_drift_first(const DriftArgs& a, hipStream_t s);
// finalize over every NodeClaim of the launch's first feasible simulation (rec->local), `max_nc` workgroups
hipError_t launch_finalize_drift(const FinalizeArgs* dev_args, const DriftRec* rec, int max_nc, hipStream_t s);

// kp_consolidate_argmin: per-block partial bests, and the record each rank contributes to the all-gather
struct ArgmaxPart {
  double savings;
  int64_t index;  // -1: no non-no-op decision in the range
  uint64_t counts[4];  // no-op, delete, replace, pod-queue overflows
};
struct CommBest {
  int64_t index;  // global subset index, -1: every decision of the rank was a no-op
  uint64_t counts[4];  // no-op, delete, replace, pod-queue overflows
  SimOut rec;
};
hipError_t launch_argmax(const SimOut* out, int n, ArgmaxPart* part, int n_parts, int64_t base, CommBest* dst,
                         hipStream_t s);

hipError_t launch_sim_prep(const SimArgs& a, hipStream_t s);
hipError_t launch_sim(const SimArgs& a, int blocks, size_t dyn_lds, hipStream_t s);
// the gated instantiation (disruption budgets): the waves walk live[0 .. n_live), the admissible subsets, ascending
hipError_t launch_sim_gated(const SimArgs& a, const uint32_t* live, int n_live, int blocks, size_t dyn_lds, hipStream_t s);
const void* sim_kernel_ptr(bool gated = false);
// the emitting instantiation (kp_cluster_command): as launch_sim_gated, with the command records
hipError_t launch_sim_emit(const SimArgs& a, const SimEmit& em, int n_live, int blocks, size_t dyn_lds, hipStream_t s);
const void* sim_emit_kernel_ptr();
// the checking instantiation (kp_cluster_validate): as launch_sim_gated, with the checks and the verdict records
hipError_t launch_sim_check(const SimArgs& a, const SimCheck& ck, int n_live, int blocks, size_t dyn_lds, hipStream_t s);
const void* sim_check_kernel_ptr();
// the explaining instantiation (kp_cluster_simulate_explained): as launch_sim_gated, with the reason records
hipError_t launch_sim_why(const SimArgs& a, const SimWhy& wy, int n_live, int blocks, size_t dyn_lds, hipStream_t s);
const void* sim_why_kernel_ptr();
#define SIM_WAVES 4

hipError_t launch_solve(const SolveArgs& a, int nw, size_t dyn_lds, hipStream_t s);
hipError_t launch_finalize(const FinalizeArgs& a, hipStream_t s);
hipError_t launch_solve_batch(const SolveArgs& a0, const SolveArgs* dev_args, int n, size_t dyn_lds, hipStream_t s);
hipError_t launch_finalize_batch(const FinalizeArgs& a0, const FinalizeArgs* dev_args, int n, hipStream_t s);
hipError_t launch_batch_init(const BatchInitArgs& a, int n_arenas, hipStream_t s);
hipError_t launch_feasibility(const FeasArgs& a, hipStream_t s);

