// kp_host.cpp — host side of the C ABI (include/kp/kp_abi.h).
//
// Compiles the string-keyed reference objects (InstanceType, NodePool, Pod, Node) into the device data
// model of kp_model.h, owns device memory and the HIP stream, launches the kernels of kp_kernels.hip and
// copies results back. There is no CPU fallback: without a HIP device every compute entry point returns
// KP_E_DEVICE (the Go shim's own CPU path is the fallback).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <arpa/inet.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "kp/kp_abi.h"
#include "kp_cand.h"
#include "kp_catcomp.h"
#include "kp_driftdet.h"
#include "kp_interrupt.h"
#include "kp_ltgroup.h"
#include "kp_schedin.h"
#include "kp_device.h"
#include "kp_model.h"

using std::map;
using std::string;
using std::vector;

namespace {

thread_local string g_err;
std::atomic<bool> g_host_timing{false};  // kp_overrides.host_timing of the last context that set it (stderr only)
int32_t fail(int32_t code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) return fail(KP_E_DEVICE, "%s: %s", #x, hipGetErrorString(e_));   \
  } while (0)

const char* kHostname = "kubernetes.io/hostname";
const char* kZone = "topology.kubernetes.io/zone";
const char* kCapType = "karpenter.sh/capacity-type";
const char* kZoneID = "topology.k8s.aws/zone-id";
const char* kResID = "karpenter.k8s.aws/capacity-reservation-id";
const char* kResType = "karpenter.k8s.aws/capacity-reservation-type";
const char* kNodePool = "karpenter.sh/nodepool";

// karpv1.WellKnownLabels + R:pkg/apis/v1/labels.go:31-56
const std::set<string>& WellKnown() {
  static const std::set<string> s = {
      "karpenter.sh/nodepool", "topology.kubernetes.io/zone", "topology.kubernetes.io/region",
      "node.kubernetes.io/instance-type", "kubernetes.io/arch", "kubernetes.io/os", "karpenter.sh/capacity-type",
      "node.kubernetes.io/windows-build", "karpenter.k8s.aws/capacity-reservation-id",
      "karpenter.k8s.aws/capacity-reservation-type", "karpenter.k8s.aws/instance-hypervisor",
      "karpenter.k8s.aws/instance-encryption-in-transit-supported", "karpenter.k8s.aws/instance-category",
      "karpenter.k8s.aws/instance-family", "karpenter.k8s.aws/instance-generation", "karpenter.k8s.aws/instance-size",
      "karpenter.k8s.aws/instance-local-nvme", "karpenter.k8s.aws/instance-cpu",
      "karpenter.k8s.aws/instance-cpu-manufacturer", "karpenter.k8s.aws/instance-cpu-sustained-clock-speed-mhz",
      "karpenter.k8s.aws/instance-memory", "karpenter.k8s.aws/instance-ebs-bandwidth",
      "karpenter.k8s.aws/instance-network-bandwidth", "karpenter.k8s.aws/instance-gpu-name",
      "karpenter.k8s.aws/instance-gpu-manufacturer", "karpenter.k8s.aws/instance-gpu-count",
      "karpenter.k8s.aws/instance-gpu-memory", "karpenter.k8s.aws/instance-accelerator-name",
      "karpenter.k8s.aws/instance-accelerator-manufacturer", "karpenter.k8s.aws/instance-accelerator-count",
      "topology.k8s.aws/zone-id"};
  return s;
}
string Normalize(const string& k) {  // karpv1.NormalizedLabels (+ R:kwok/operator/operator.go:73)
  static const map<string, string> m = {
      {"failure-domain.beta.kubernetes.io/zone", "topology.kubernetes.io/zone"},
      {"beta.kubernetes.io/arch", "kubernetes.io/arch"},
      {"beta.kubernetes.io/os", "kubernetes.io/os"},
      {"beta.kubernetes.io/instance-type", "node.kubernetes.io/instance-type"},
      {"failure-domain.beta.kubernetes.io/region", "topology.kubernetes.io/region"},
      {"topology.ebs.csi.aws.com/zone", "topology.kubernetes.io/zone"},
  };
  auto it = m.find(k);
  return it == m.end() ? k : it->second;
}
bool Atoi(const string& s, int64_t* out) {  // Go strconv.Atoi
  if (s.empty()) return false;
  size_t i = 0;
  bool neg = false;
  if (s[0] == '+' || s[0] == '-') {
    neg = s[0] == '-';
    if (s.size() == 1) return false;
    i = 1;
  }
  unsigned __int128 v = 0;
  const unsigned __int128 lim = (unsigned __int128)std::numeric_limits<int64_t>::max() + (neg ? 1 : 0);
  for (; i < s.size(); i++) {
    if (s[i] < '0' || s[i] > '9') return false;
    v = v * 10 + (unsigned)(s[i] - '0');
    if (v > lim) return false;
  }
  *out = neg ? (int64_t)(-(__int128)v) : (int64_t)v;
  return true;
}

// ------------------------------------------------------------------------------------------------
// raw (string) model
// ------------------------------------------------------------------------------------------------
struct RawReq {
  string key;
  int op;
  vector<string> values;
  int minv;  // < 0 nil
};
using RawReqs = vector<RawReq>;

RawReqs ParseReqs(const kp_requirements& in) {
  RawReqs out;
  for (uint32_t i = 0; i < in.n; i++) {
    const kp_requirement& q = in.items[i];
    RawReq r;
    r.key = Normalize(q.key ? q.key : "");
    r.op = q.op;
    r.minv = q.min_values;
    for (uint32_t j = 0; j < q.n_values; j++) r.values.push_back(q.values[j] ? q.values[j] : "");
    out.push_back(std::move(r));
  }
  return out;
}
RawReqs LabelReqs(const kp_label* l, uint32_t n, bool drop_hostname) {
  RawReqs out;
  out.reserve(n + 1);
  for (uint32_t i = 0; i < n; i++) {
    string k = Normalize(l[i].key ? l[i].key : "");
    if (drop_hostname && k == kHostname) continue;
    out.push_back({k, KP_OP_IN, {l[i].value ? l[i].value : ""}, -1});
  }
  return out;
}

// scheduling.GetHostPorts entries in a canonical form: (protocol, port) group + 16-byte IP (IPv4 as ::ffff:a.b.c.d,
// the form net.ParseIP returns, so IP.Equal of a v4 and its v4-in-v6 spelling holds). Entries with hostPort 0 are
// skipped, as GetHostPorts skips them; an unparsable IP is KP_E_INVAL (the API server validates hostIP).
struct HostPortKey {
  int proto, port;
  std::array<uint8_t, 16> ip;
  bool unspec;
};
bool ParseHostPorts(const kp_host_port* hp, uint32_t n, vector<HostPortKey>* out, string* err) {
  for (uint32_t i = 0; i < n; i++) {
    if (hp[i].port == 0) continue;
    if (hp[i].port < 0 || hp[i].port > 65535 || hp[i].protocol < KP_PROTO_TCP || hp[i].protocol > KP_PROTO_SCTP) {
      *err = "host port " + std::to_string(hp[i].port) + "/" + std::to_string(hp[i].protocol);
      return false;
    }
    HostPortKey k;
    k.proto = hp[i].protocol;
    k.port = hp[i].port;
    k.ip.fill(0);
    const string ip = hp[i].ip && hp[i].ip[0] ? hp[i].ip : "0.0.0.0";
    uint8_t v4[4];
    if (inet_pton(AF_INET, ip.c_str(), v4) == 1) {
      k.ip[10] = k.ip[11] = 0xFF;
      memcpy(&k.ip[12], v4, 4);
    } else if (inet_pton(AF_INET6, ip.c_str(), k.ip.data()) != 1) {
      *err = "host IP '" + ip + "'";
      return false;
    }
    static const uint8_t v4z[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xFF, 0xFF, 0, 0, 0, 0};
    static const uint8_t v6z[16] = {0};
    k.unspec = memcmp(k.ip.data(), v4z, 16) == 0 || memcmp(k.ip.data(), v6z, 16) == 0;
    out->push_back(k);
  }
  return true;
}

struct HostOffering {
  string ct, zone, zid;
  bool has_zone, has_zid;
  double price;
  bool available;
  string rid, rt;  // capacity-reservation-id / -type In {..}; DoesNotExist when !has_rid / !has_rt
  bool has_rid = false, has_rt = false;
  int32_t rcap = 0;  // ReservationCapacity
};
struct HostType {
  string name;
  RawReqs reqs;
  int64_t cap[KP_NRES];
  int64_t ovh[KP_NRES];
  uint32_t cap_present;
  vector<HostOffering> offs;
};

}  // namespace

namespace {
struct SolveBase;
}

struct kp_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
  kp_options opts;
  kp_overrides ov{};  // kp_ctx_set_overrides (tests, measurement); all 0 = production
  std::recursive_mutex mu;  // recursive: the general simulation path runs whole Solves under the cluster plan's lock
  // resident compiled catalogues + templates of recent Solves (most recent last), see SolveBase
  vector<std::shared_ptr<SolveBase>> bases;
  uint64_t base_hits = 0, base_misses = 0;
  // per-Solve device arena handed back by kp_solve_plan_destroy and reused by the next kp_solve_prepare
  void* spare = nullptr;
  size_t spare_bytes = 0;
  // kp_scheduler_inputs' device arena, kept across calls (grown, never shrunk)
  void* schedin = nullptr;
  size_t schedin_bytes = 0;
  // kp_catalog_compile's, likewise
  void* catcomp = nullptr;
  size_t catcomp_bytes = 0;
  // kp_ctx_destroy's reference plus one per live dependent (catalogue, plan, communicator): the context is freed
  // when the last goes, so a dependent may be destroyed after the context (any order, e.g. a garbage collector's)
  std::atomic<int> refs{1};
};
static void CtxFree(kp_ctx* c) {
  (void)hipSetDevice(c->device);
  c->bases.clear();
  if (c->spare) (void)hipFree(c->spare);
  if (c->schedin) (void)hipFree(c->schedin);
  if (c->catcomp) (void)hipFree(c->catcomp);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->ev2) (void)hipEventDestroy(c->ev2);
  if (c->ev3) (void)hipEventDestroy(c->ev3);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}
inline void CtxUnref(kp_ctx* c) {
  if (c && c->refs.fetch_sub(1) == 1) CtxFree(c);
}
// A dependent's context pointer holding a reference (assignment takes one, destruction drops it).
struct CtxRef {
  kp_ctx* p = nullptr;
  CtxRef() = default;
  CtxRef(const CtxRef&) = delete;
  CtxRef& operator=(const CtxRef&) = delete;
  CtxRef& operator=(kp_ctx* c) {
    if (c) c->refs.fetch_add(1);
    CtxUnref(p);
    p = c;
    return *this;
  }
  ~CtxRef() { CtxUnref(p); }
  kp_ctx* operator->() const { return p; }
  operator kp_ctx*() const { return p; }
};

struct kp_catalog {
  CtxRef ctx;
  uint64_t seqnum;
  uint64_t uid;  // process-unique identity (a new upload never reuses one, unlike its address)
  vector<HostType> types;
  bool reservations = false;  // some offering carries a capacity-reservation id or type
  // false once kp_catalog_destroy ran: plans and cached bases that compiled this catalogue hold the token and refuse
  // to run (or refresh) instead of reading a freed catalogue
  std::shared_ptr<bool> alive = std::make_shared<bool>(true);
};

namespace {

// ------------------------------------------------------------------------------------------------
// dictionary
// ------------------------------------------------------------------------------------------------
struct Dict {
  vector<string> keys;
  std::unordered_map<string, int> key_id;
  vector<vector<string>> vals;
  vector<std::unordered_map<string, int>> val_id;  // value -> bit (global)
  DevDict dd;
  vector<int64_t> vint;  // [W*64]
  int key(const string& k) const {
    auto it = key_id.find(k);
    return it == key_id.end() ? -1 : it->second;
  }
  int bit(int k, const string& v) const {
    auto it = val_id[k].find(v);
    return it == val_id[k].end() ? -1 : it->second;
  }
};

struct DictBuilder {
  map<string, bool> bounded;  // key -> needs bound slot
  map<string, std::set<string>> values;
  void addReqs(const RawReqs& rs) {
    for (auto& r : rs) {
      auto& b = bounded[r.key];
      if (r.op == KP_OP_GT || r.op == KP_OP_LT || r.minv >= 0) b = true;
      auto& s = values[r.key];
      if (r.op == KP_OP_IN || r.op == KP_OP_NOT_IN) s.insert(r.values.begin(), r.values.end());
    }
  }
  void addLabel(const string& k, const string& v) {
    bounded[k];
    values[k].insert(v);
  }
  int32_t build(Dict& d) {
    vector<string> order;
    for (auto& kv : bounded)
      if (kv.second) order.push_back(kv.first);
    const int KB = (int)order.size();
    if (KB > KP_MAX_BOUND_KEYS) return fail(KP_E_UNSUPPORTED, "%d keys with Gt/Lt/minValues (max %d)", KB, KP_MAX_BOUND_KEYS);
    for (auto& kv : bounded)
      if (!kv.second) order.push_back(kv.first);
    if ((int)order.size() > KP_MAX_KEYS) return fail(KP_E_UNSUPPORTED, "%zu label keys (max %d)", order.size(), KP_MAX_KEYS);
    memset(&d.dd, 0, sizeof(d.dd));
    d.keys = order;
    d.vals.assign(order.size(), {});
    d.val_id.assign(order.size(), {});
    const int K = (int)order.size();
    int w = K;  // words 0..K-1 are the keys' first words; overflow words follow
    for (int k = 0; k < K; k++) {
      d.key_id[order[k]] = k;
      auto& s = values[order[k]];
      d.vals[k].assign(s.begin(), s.end());
      const int nw = std::max<int>(1, (int)((s.size() + 63) / 64));
      d.dd.wofs[k] = k;
      d.dd.ovf[k] = nw > 1 ? w : -1;
      d.dd.nval[k] = (int)s.size();
      d.dd.wkey[k] = (int8_t)k;
      if (nw > 1) {
        if (w + nw - 1 > KP_MAX_WORDS) return fail(KP_E_UNSUPPORTED, "label values need > %d words", KP_MAX_WORDS);
        d.dd.multiword |= 1ull << k;
        for (int i = 0; i < nw - 1; i++) {
          d.dd.wkey[w + i] = (int8_t)k;
          d.dd.ovfmask[k] |= 1ull << (w + i);
        }
        w += nw - 1;
      }
      int b = 0;
      for (auto& v : d.vals[k]) {
        const int word = b < 64 ? k : d.dd.ovf[k] + b / 64 - 1;
        d.val_id[k][v] = word * 64 + b % 64;
        d.dd.validbits[word] |= 1ull << (b % 64);
        b++;
      }
    }
    d.dd.firstmask = K >= 64 ? ~0ull : ((1ull << K) - 1);
    for (int i = w; i < KP_MAX_WORDS; i++) d.dd.wkey[i] = -1;
    d.dd.K = (int)order.size();
    d.dd.W = w;
    d.dd.KB = KB;
    d.vint.assign((size_t)std::max(w, 1) * 64, 0);
    for (size_t k = 0; k < order.size(); k++)
      for (auto& kv : d.val_id[k]) {
        int64_t x;
        if (Atoi(kv.first, &x)) {
          d.vint[kv.second] = x;
          d.dd.vint_ok[kv.second / 64] |= 1ull << (kv.second % 64);
        }
      }
    for (size_t k = 0; k < order.size(); k++)
      if (WellKnown().count(order[k])) d.dd.wellknown |= 1ull << k;
    int rk = d.key(kResID), tk = d.key(kResType);
    d.dd.resid_key_bit = rk >= 0 ? 1ull << rk : 0;
    d.dd.restype_key_bit = tk >= 0 ? 1ull << tk : 0;
    d.dd.offer_keys = d.dd.resid_key_bit | d.dd.restype_key_bit;
    for (const char* k : {kCapType, kZone, kZoneID})
      if (d.key(k) >= 0) d.dd.offer_keys |= 1ull << d.key(k);
    return KP_OK;
  }
};

// ------------------------------------------------------------------------------------------------
// host requirement algebra on KReqs (same encoding the device uses)
// ------------------------------------------------------------------------------------------------
bool Within(const Dict& d, int bit, bool hg, int64_t gt, bool hl, int64_t lt) {
  if (!hg && !hl) return true;
  if (!((d.dd.vint_ok[bit / 64] >> (bit % 64)) & 1)) return false;
  int64_t x = d.vint[bit];
  if (hg && gt >= x) return false;
  if (hl && lt <= x) return false;
  return true;
}
int nwords(const Dict& d, int k) { return std::max(1, (d.dd.nval[k] + 63) / 64); }
int kw(const Dict& d, int k, int i) { return i == 0 ? k : d.dd.ovf[k] + i - 1; }  // i-th word of key k

KReqs Single(const Dict& d, const RawReq& r) {
  KReqs q;
  memset(&q, 0, sizeof q);
  const int k = d.key(r.key);
  q.present = 1ull << k;
  if (r.minv >= 0) {
    q.hmin = 1ull << k;
    q.minv[k] = r.minv;
  }
  auto setvals = [&]() {
    for (auto& v : r.values) {
      int b = d.bit(k, v);
      q.vals[b / 64] |= 1ull << (b % 64);
    }
  };
  switch (r.op) {
    case KP_OP_IN:
      setvals();
      break;
    case KP_OP_NOT_IN:
      q.compl_ = 1ull << k;
      setvals();
      break;
    case KP_OP_EXISTS:
      q.compl_ = 1ull << k;
      break;
    case KP_OP_DOES_NOT_EXIST:
      break;
    case KP_OP_GT:
    case KP_OP_LT: {
      q.compl_ = 1ull << k;
      int64_t x = 0;
      Atoi(r.values.empty() ? string() : r.values[0], &x);
      if (r.op == KP_OP_GT) {
        q.hgt = 1ull << k;
        q.gt[k] = x;
      } else {
        q.hlt = 1ull << k;
        q.lt[k] = x;
      }
      break;
    }
  }
  return q;
}

// A = A.Add(B) per key (Requirement.Intersection for shared keys).
void HostAdd(const Dict& d, KReqs& A, const KReqs& B) {
  // B's keys in increasing order (each key is independent of the others)
  for (uint64_t km = B.present & (d.dd.K >= 64 ? ~0ull : (1ull << d.dd.K) - 1); km; km &= km - 1) {
    const int k = __builtin_ctzll(km);
    const uint64_t kb = 1ull << k;
    const int nw = nwords(d, k);
    const bool bnd = k < KP_MAX_BOUND_KEYS;
    if (!(A.present & kb)) {
      A.present |= kb;
      A.compl_ = (A.compl_ & ~kb) | (B.compl_ & kb);
      A.hgt = (A.hgt & ~kb) | (B.hgt & kb);
      A.hlt = (A.hlt & ~kb) | (B.hlt & kb);
      A.hmin = (A.hmin & ~kb) | (B.hmin & kb);
      if (bnd) {
        A.gt[k] = B.gt[k];
        A.lt[k] = B.lt[k];
        A.minv[k] = B.minv[k];
      }
      for (int i = 0; i < nw; i++) A.vals[kw(d, k, i)] = B.vals[kw(d, k, i)];
      continue;
    }
    const bool c1 = A.compl_ & kb, c2 = B.compl_ & kb;
    const bool ag = A.hgt & kb, bg = B.hgt & kb, al = A.hlt & kb, bl = B.hlt & kb;
    const bool hg = ag || bg, hl = al || bl;
    int64_t gt = 0, lt = 0;
    if (bnd) {
      gt = ag && bg ? std::max(A.gt[k], B.gt[k]) : (ag ? A.gt[k] : B.gt[k]);
      lt = al && bl ? std::min(A.lt[k], B.lt[k]) : (al ? A.lt[k] : B.lt[k]);
      const bool am = A.hmin & kb, bm = B.hmin & kb;
      A.minv[k] = am && bm ? std::max(A.minv[k], B.minv[k]) : (am ? A.minv[k] : B.minv[k]);
    }
    A.hmin |= B.hmin & kb;
    if (hg && hl && gt >= lt) {  // DoesNotExist
      A.compl_ &= ~kb;
      A.hgt &= ~kb;
      A.hlt &= ~kb;
      for (int i = 0; i < nw; i++) A.vals[kw(d, k, i)] = 0;
      continue;
    }
    for (int i = 0; i < nw; i++) {
      const int w = kw(d, k, i);
      const uint64_t a = A.vals[w], b = B.vals[w];
      uint64_t v = (c1 && c2) ? (a | b) : c1 ? (b & ~a) : c2 ? (a & ~b) : (a & b);
      if (hg || hl) {
        uint64_t m = v, o = 0;
        while (m) {
          int bb = __builtin_ctzll(m);
          m &= m - 1;
          if (Within(d, w * 64 + bb, hg, gt, hl, lt)) o |= 1ull << bb;
        }
        v = o;
      }
      A.vals[w] = v;
    }
    const bool c = c1 && c2;
    if (c) {
      A.compl_ |= kb;
      if (hg) A.hgt |= kb, A.gt[k] = gt;
      if (hl) A.hlt |= kb, A.lt[k] = lt;
    } else {
      A.compl_ &= ~kb;
      A.hgt &= ~kb;
      A.hlt &= ~kb;
    }
  }
}

KReqs Compile(const Dict& d, const RawReqs& rs) {
  KReqs q;
  memset(&q, 0, sizeof q);
  for (auto& r : rs) HostAdd(d, q, Single(d, r));
  return q;
}
bool KeyNonEmptyVals(const Dict& d, const KReqs& q, int k) {
  for (int i = 0; i < nwords(d, k); i++)
    if (q.vals[kw(d, k, i)]) return true;
  return false;
}
uint64_t NegOp(const Dict& d, const KReqs& q) {
  uint64_t m = 0;
  for (int k = 0; k < d.dd.K; k++) {
    if (!((q.present >> k) & 1)) continue;
    bool c = (q.compl_ >> k) & 1, nz = KeyNonEmptyVals(d, q, k);
    if ((c && nz) || (!c && !nz)) m |= 1ull << k;
  }
  return m;
}
bool Has(const Dict& d, const KReqs& q, int k, int bit) {
  if (!((q.present >> k) & 1)) return true;
  bool in = (q.vals[bit / 64] >> (bit % 64)) & 1;
  if ((q.compl_ >> k) & 1) {
    const bool bnd = k < KP_MAX_BOUND_KEYS;
    return !in && Within(d, bit, bnd && ((q.hgt >> k) & 1), bnd ? q.gt[k] : 0, bnd && ((q.hlt >> k) & 1),
                         bnd ? q.lt[k] : 0);
  }
  return in;
}

// ------------------------------------------------------------------------------------------------
// catalogue compile (per solve dictionary)
// ------------------------------------------------------------------------------------------------
struct HostCat {
  int T = 0, S = 0;
  vector<KReqs> treqs;
  vector<uint64_t> TM, DNE, NOKEY;    // [nbits][TW], [K][TW], [K][TW]
  vector<int64_t> alloc, cap;         // [R][T]
  vector<uint64_t> nonneg;            // [TW]
  vector<int64_t> fit_vals;           // [R][T]
  vector<int32_t> fit_n;              // [R]
  vector<uint64_t> fit_mask;          // [R][T][TW]
  vector<uint64_t> offer_avail;       // [C][TW]
  vector<double> price;               // [T][C]
  vector<double> price_cm;            // [C][S]
  vector<double> price_sub;           // [2^C][S] (C <= KP_SUB_MAX_C)
  vector<uint32_t> name_rank;         // [T]
  vector<uint16_t> code;              // [K][T]
  vector<uint64_t> multi;             // [K][T]
  vector<uint64_t> custom_nonneg;     // [T]
  uint64_t multi_valued = 0;
  uint64_t custom_any = 0;            // OR of custom_nonneg
};

struct ClassKey {
  int ct, zone, zid, rid = -1, rt = -1;
  bool operator<(const ClassKey& o) const {
    return std::tie(ct, zone, zid, rid, rt) < std::tie(o.ct, o.zone, o.zid, o.rid, o.rt);
  }
};
// An offering's class: its label values as dictionary bits (-1: no such requirement / DoesNotExist).
ClassKey ClassOf(const Dict& d, const HostOffering& o) {
  return {d.bit(d.key(kCapType), o.ct), o.has_zone ? d.bit(d.key(kZone), o.zone) : -1,
          o.has_zid ? d.bit(d.key(kZoneID), o.zid) : -1, o.has_rid ? d.bit(d.key(kResID), o.rid) : -1,
          o.has_rt ? d.bit(d.key(kResType), o.rt) : -1};
}
OfferClass ClassOfKey(const ClassKey& k) {
  return {(int16_t)k.ct, (int16_t)k.zone, (int16_t)k.zid, (int16_t)k.rid, (int16_t)k.rt, {0, 0, 0}};
}
ClassKey KeyOfClass(const OfferClass& c) { return {c.ct_bit, c.zone_bit, c.zid_bit, c.rid_bit, c.rt_bit}; }

// Offering section of a compiled catalogue: available classes per type, cheapest price per (type, class), and the
// class-major copy (offering.go:115-147 createOfferings: Available = !ICE && hasPrice && zone offered). Also the
// whole of an ICE refresh (kp_filter_refresh): availability and price are the only inputs an ICE mark changes.
void FillOfferings(const Dict& d, const vector<HostType>& types, int TW, const map<ClassKey, int>& classes,
                   HostCat& hc) {
  const int T = hc.T, S = hc.S;
  const int C = (int)classes.size();
  hc.offer_avail.assign((size_t)C * TW, 0);
  hc.price.assign((size_t)T * C, std::numeric_limits<double>::infinity());
  for (int t = 0; t < T; t++)
    for (auto& o : types[t].offs) {
      const int c = classes.at(ClassOf(d, o));
      if (!o.available) continue;
      hc.offer_avail[(size_t)c * TW + t / 64] |= 1ull << (t % 64);
      double& p = hc.price[(size_t)t * C + c];
      if (o.price < p) p = o.price;
    }
  hc.price_cm.assign((size_t)C * S, std::numeric_limits<double>::infinity());  // row stride S (= D.T)
  for (int t = 0; t < T; t++)
    for (int c = 0; c < C; c++) hc.price_cm[(size_t)c * S + t] = hc.price[(size_t)t * C + c];
  // cheapest over a row's compatible class set in one gather: min over each subset m, built from m & (m - 1)
  hc.price_sub.clear();
  if (C <= KP_SUB_MAX_C) {
    hc.price_sub.assign((size_t)S << C, std::numeric_limits<double>::infinity());
    for (size_t m = 1; m < ((size_t)1 << C); m++) {
      const int c = __builtin_ctzll(m);
      const double* prev = &hc.price_sub[(m & (m - 1)) * S];
      double* cur = &hc.price_sub[m * S];
      for (int t = 0; t < T; t++) cur[t] = std::min(prev[t], hc.price[(size_t)t * C + c]);
    }
  }
}

int32_t CompileCatalog(const Dict& d, const vector<HostType>& types, int TW, map<ClassKey, int>& classes, HostCat& hc) {
  const int T = (int)types.size(), K = d.dd.K, NB = d.dd.W * 64;
  const int S = std::max(d.dd.T, T);  // row stride shared by every catalogue of the solve (device uses D.T)
  hc.T = T;
  hc.S = S;
  hc.treqs.resize(T);
  hc.TM.assign((size_t)NB * TW, 0);
  hc.DNE.assign((size_t)K * TW, 0);
  hc.NOKEY.assign((size_t)K * TW, 0);
  hc.code.assign((size_t)K * S, 0xFFFF);
  hc.multi.assign((size_t)K * S, 0);
  hc.custom_nonneg.assign(S, 0);
  for (int t = 0; t < T; t++) {
    KReqs q = Compile(d, types[t].reqs);
    hc.treqs[t] = q;
    const uint64_t tb = 1ull << (t % 64);
    const int tw = t / 64;
    const uint64_t neg = NegOp(d, q);
    for (int k = 0; k < K; k++) {
      const uint64_t kb = 1ull << k;
      if (!(q.present & kb)) {
        hc.NOKEY[(size_t)k * TW + tw] |= tb;
        continue;
      }
      if ((q.compl_ & kb) || (q.hgt & kb) || (q.hlt & kb))
        return fail(KP_E_UNSUPPORTED, "instance type %s: requirement %s is not In/DoesNotExist", types[t].name.c_str(),
                    d.keys[k].c_str());
      if (!(d.dd.wellknown & kb) && !(neg & kb)) {
        hc.custom_nonneg[t] |= kb;
        hc.custom_any |= kb;
      }
      int cnt = 0, last = -1;
      for (int wi = 0, w = kw(d, k, 0); wi < nwords(d, k); wi++, w = wi < nwords(d, k) ? kw(d, k, wi) : 0) {
        uint64_t m = q.vals[w];
        while (m) {
          int b = __builtin_ctzll(m);
          m &= m - 1;
          int bit = w * 64 + b;
          hc.TM[(size_t)bit * TW + tw] |= tb;
          cnt++;
          last = bit;
        }
      }
      if (cnt == 0) {
        hc.DNE[(size_t)k * TW + tw] |= tb;
        hc.code[(size_t)k * S + t] = 0xFFFE;
      } else if (cnt == 1) {
        hc.code[(size_t)k * S + t] = (uint16_t)last;
      } else {
        if (d.dd.nval[k] > 64) return fail(KP_E_UNSUPPORTED, "multi-valued key %s has > 64 values", d.keys[k].c_str());
        hc.multi_valued |= kb;
        hc.code[(size_t)k * S + t] = 0xFFFD;
        hc.multi[(size_t)k * S + t] = q.vals[d.dd.wofs[k]];
      }
    }
  }
  for (int k = 0; k < K; k++)  // keys whose types are multi-valued keep multi masks for every type
    if ((hc.multi_valued >> k) & 1)
      for (int t = 0; t < T; t++) {
        uint16_t& c = hc.code[(size_t)k * S + t];
        if (c < 0xFFFD) {
          hc.multi[(size_t)k * S + t] = 1ull << (c % 64);
          c = 0xFFFD;
        }
      }
  // resources
  hc.alloc.assign((size_t)KP_NRES * S, 0);
  hc.cap.assign((size_t)KP_NRES * S, 0);
  hc.nonneg.assign(TW, 0);
  for (int t = 0; t < T; t++) {
    bool nn = true;
    for (int r = 0; r < KP_NRES; r++) {
      const bool pr = (types[t].cap_present >> r) & 1;
      const int64_t c = pr ? types[t].cap[r] : 0;
      const int64_t a = pr ? c - types[t].ovh[r] : 0;  // resources.Subtract(capacity, overhead): capacity keys
      hc.cap[(size_t)r * S + t] = c;
      hc.alloc[(size_t)r * S + t] = a;
      if (pr && a < 0) nn = false;
    }
    if (nn) hc.nonneg[t / 64] |= 1ull << (t % 64);
  }
  hc.fit_vals.assign((size_t)KP_NRES * S, 0);
  hc.fit_n.assign(KP_NRES, 0);
  hc.fit_mask.assign((size_t)KP_NRES * S * TW, 0);
  for (int r = 0; r < KP_NRES; r++) {
    vector<int64_t> v(hc.alloc.begin() + (size_t)r * S, hc.alloc.begin() + (size_t)r * S + T);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    hc.fit_n[r] = (int)v.size();
    std::copy(v.begin(), v.end(), hc.fit_vals.begin() + (size_t)r * S);
    // fit_mask[r][j] = types with alloc >= v[j]: build from the top down
    vector<uint64_t> acc(TW, 0);
    vector<std::pair<int64_t, int>> byv;
    for (int t = 0; t < T; t++) byv.push_back({hc.alloc[(size_t)r * S + t], t});
    std::sort(byv.begin(), byv.end());
    int p = T - 1;
    for (int j = (int)v.size() - 1; j >= 0; j--) {
      while (p >= 0 && byv[p].first >= v[j]) {
        acc[byv[p].second / 64] |= 1ull << (byv[p].second % 64);
        p--;
      }
      std::copy(acc.begin(), acc.end(), hc.fit_mask.begin() + ((size_t)r * S + j) * TW);
    }
  }
  FillOfferings(d, types, TW, classes, hc);
  vector<int> idx(T);
  for (int t = 0; t < T; t++) idx[t] = t;
  std::sort(idx.begin(), idx.end(), [&](int a, int b) { return types[a].name < types[b].name; });
  hc.name_rank.assign(S, 0);
  for (int i = 0; i < T; i++) hc.name_rank[idx[i]] = (uint32_t)i;
  return KP_OK;
}

// Pass_k(q_k) over the catalogue (host version, every key of q): NOKEY ∪ ∪_{Has(v)} TM[v] ∪ (negop ? DNE)
void HostFilterTypes(const Dict& d, const HostCat& hc, const KReqs& q, int TW, const int64_t* total,
                     vector<uint64_t>& X) {
  const uint64_t neg = NegOp(d, q);
  for (int k = 0; k < d.dd.K; k++) {
    if (!((q.present >> k) & 1)) continue;
    vector<uint64_t> acc(TW, 0);
    for (int w = 0; w < TW; w++) acc[w] = hc.NOKEY[(size_t)k * TW + w] | (((neg >> k) & 1) ? hc.DNE[(size_t)k * TW + w] : 0);
    for (int wi = 0, w = kw(d, k, 0); wi < nwords(d, k); wi++, w = wi < nwords(d, k) ? kw(d, k, wi) : 0) {
      uint64_t m = d.dd.validbits[w];
      while (m) {
        int b = __builtin_ctzll(m);
        m &= m - 1;
        if (Has(d, q, k, w * 64 + b))
          for (int x = 0; x < TW; x++) acc[x] |= hc.TM[(size_t)(w * 64 + b) * TW + x];
      }
    }
    for (int w = 0; w < TW; w++) X[w] &= acc[w];
  }
  // Fits(total, allocatable)
  for (int t = 0; t < hc.T; t++) {
    bool ok = (hc.nonneg[t / 64] >> (t % 64)) & 1;
    for (int r = 0; r < KP_NRES && ok; r++)
      if (total[r] > 0 && total[r] > hc.alloc[(size_t)r * hc.S + t]) ok = false;
    if (!ok) X[t / 64] &= ~(1ull << (t % 64));
  }
}

uint64_t HostAllowedClasses(const Dict& d, const KReqs& q, const vector<OfferClass>& cls) {
  const uint64_t neg = NegOp(d, q);
  // a reservation key the offering does not carry is DoesNotExist: compatible when the query leaves the key out or
  // admits its absence (NotIn / DoesNotExist)
  const bool res_ok = !(q.present & d.dd.resid_key_bit) || (neg & d.dd.resid_key_bit);
  const bool rt_ok = !(q.present & d.dd.restype_key_bit) || (neg & d.dd.restype_key_bit);
  uint64_t m = 0;
  auto keyof = [&](int bit) { return (int)d.dd.wkey[bit / 64]; };
  for (size_t c = 0; c < cls.size(); c++) {
    bool ok = Has(d, q, keyof(cls[c].ct_bit), cls[c].ct_bit);
    if (cls[c].zone_bit >= 0) ok = ok && Has(d, q, keyof(cls[c].zone_bit), cls[c].zone_bit);
    if (cls[c].zid_bit >= 0) ok = ok && Has(d, q, keyof(cls[c].zid_bit), cls[c].zid_bit);
    ok = ok && (cls[c].rid_bit >= 0 ? Has(d, q, keyof(cls[c].rid_bit), cls[c].rid_bit) : res_ok);
    ok = ok && (cls[c].rt_bit >= 0 ? Has(d, q, keyof(cls[c].rt_bit), cls[c].rt_bit) : rt_ok);
    if (ok) m |= 1ull << c;
  }
  return m;
}

int CountDistinct(const Dict& d, const HostCat& hc, int k, const vector<int>& types) {
  std::set<int> vals;
  for (int t : types) {
    const KReqs& q = hc.treqs[t];
    for (int wi = 0, w = kw(d, k, 0); wi < nwords(d, k); wi++, w = wi < nwords(d, k) ? kw(d, k, wi) : 0) {
      uint64_t m = q.vals[w];
      while (m) {
        int b = __builtin_ctzll(m);
        m &= m - 1;
        vals.insert(w * 64 + b);
      }
    }
  }
  return (int)vals.size();
}
bool HostMinValuesOK(const Dict& d, const HostCat& hc, const KReqs& q, const vector<int>& types) {
  for (int k = 0; k < d.dd.K; k++) {
    if (!((q.hmin >> k) & 1) || !((q.present >> k) & 1)) continue;
    if (CountDistinct(d, hc, k, types) < q.minv[k]) return false;
  }
  return true;
}

// ------------------------------------------------------------------------------------------------
// device buffer arena: everything of one solve in one allocation
// ------------------------------------------------------------------------------------------------
// Host image of one device allocation: put()/reserve() lay out host-initialised regions (uploaded in one copy),
// reserve_dev() appends device-only regions after them (no host backing, nothing to zero or copy).
struct Blob {
  vector<uint8_t> host;
  size_t dev_end = 0;  // > 0 once device-only regions were appended
  template <class T>
  size_t put(const T* p, size_t n) {
    size_t off = (host.size() + 255) & ~(size_t)255;
    host.resize(off + n * sizeof(T));
    if (n) memcpy(host.data() + off, p, n * sizeof(T));
    return off;
  }
  template <class T>
  size_t put(const vector<T>& v) {
    return put(v.data(), v.size());
  }
  size_t reserve(size_t bytes) {
    size_t off = (host.size() + 255) & ~(size_t)255;
    host.resize(off + bytes);
    return off;
  }
  size_t reserve_dev(size_t bytes) {
    size_t off = (std::max(host.size(), dev_end) + 255) & ~(size_t)255;
    dev_end = off + bytes;
    return off;
  }
  size_t total() const { return std::max(host.size(), dev_end); }
};

struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  hipError_t alloc(size_t bytes) {
    reset();
    hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 1));
    if (e == hipSuccess) n = bytes;
    else p = nullptr;
    return e;
  }
};

}  // namespace

namespace {
// A NodeClaim's final requirements as upstream Requirements.NodeSelectorRequirements() renders them
// (Gt, then Lt, then NotIn/Exists, then In/DoesNotExist), keys in byte order, values sorted. The hostname
// placeholder is not part of the dictionary, as FinalizeScheduling drops it.
struct ReqOut {
  vector<string> keys;
  vector<vector<string>> vals;
  vector<vector<const char*>> ptrs;
  vector<kp_requirement> items;
};
std::shared_ptr<ReqOut> DecodeReqs(const Dict& d, const KReqs& q) {
  auto o = std::make_shared<ReqOut>();
  vector<int> ks;
  for (int k = 0; k < d.dd.K; k++)
    if (((q.present >> k) & 1) && d.keys[k] != kHostname) ks.push_back(k);  // (the NodeClaim's placeholder)
  std::sort(ks.begin(), ks.end(), [&](int a, int b) { return d.keys[a] < d.keys[b]; });
  for (int k : ks) {
    const bool bnd = k < KP_MAX_BOUND_KEYS, c = (q.compl_ >> k) & 1;
    kp_requirement it;
    memset(&it, 0, sizeof it);
    vector<string> v;
    if (c && bnd && ((q.hgt >> k) & 1)) {
      it.op = KP_OP_GT;
      v.push_back(std::to_string(q.gt[k]));
    } else if (c && bnd && ((q.hlt >> k) & 1)) {
      it.op = KP_OP_LT;
      v.push_back(std::to_string(q.lt[k]));
    } else {
      for (int i = 0; i < nwords(d, k); i++) {
        const int w = kw(d, k, i);
        uint64_t m = q.vals[w];
        while (m) {
          const int b = __builtin_ctzll(m);
          m &= m - 1;
          v.push_back(d.vals[k][(size_t)i * 64 + b]);  // ordinal = i*64 + b; dictionary values are sorted
        }
      }
      it.op = c ? (v.empty() ? KP_OP_EXISTS : KP_OP_NOT_IN) : (v.empty() ? KP_OP_DOES_NOT_EXIST : KP_OP_IN);
    }
    it.min_values = (bnd && ((q.hmin >> k) & 1)) ? q.minv[k] : -1;
    o->keys.push_back(d.keys[k]);
    o->vals.push_back(std::move(v));
    o->items.push_back(it);
  }
  o->ptrs.resize(o->vals.size());
  for (size_t i = 0; i < o->items.size(); i++) {
    for (auto& x : o->vals[i]) o->ptrs[i].push_back(x.c_str());
    o->items[i].key = o->keys[i].c_str();
    o->items[i].values = o->ptrs[i].data();
    o->items[i].n_values = (uint32_t)o->ptrs[i].size();
  }
  return o;
}
}  // namespace

struct kp_solve_result {
  vector<int32_t> placement;
  struct NC {
    uint32_t nodepool, n_remaining;
    vector<uint32_t> pods, options;
    kp_resource_list requests;
    std::shared_ptr<ReqOut> reqs;
  };
  vector<NC> ncs;
  kp_solve_stats stats;
  vector<KReqs> fin;     // per NodeClaim: final requirements (device encoding), for in-library callers
  vector<int> nc_cat;    // per NodeClaim: catalogue of its template
  // explained results (kp_solve_run_explained): one record per (shape-level row, template); pod_row[p] = the row of an
  // unscheduled pod, else -1. why_keys[row * n_tmpl + t]: the failing label keys of a KP_WHY_REQUIREMENTS record,
  // pointers into key_names (the result's own copy of the dictionary's key strings)
  bool explained = false;
  int n_tmpl = 0;
  vector<int32_t> pod_row;
  vector<ExplainRec> why;
  vector<int32_t> why_taint;             // [rows][n_tmpl] first untolerated taint of the NodePool, -1: tolerated
  vector<uint32_t> why_nodepool;         // [n_tmpl]
  vector<string> key_names;
  std::unordered_map<size_t, vector<const char*>> why_keys;
};

extern "C" {

const char* kp_last_error(void) { return g_err.c_str(); }
int32_t kp_abi_version(void) { return KP_ABI_VERSION; }

int32_t kp_ctx_create(const kp_options* opts, kp_ctx** out) {
  if (!out) return fail(KP_E_INVAL, "out is null");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) return fail(KP_E_DEVICE, "no HIP device: %s", hipGetErrorString(e));
  auto* c = new kp_ctx();
  c->opts = opts ? *opts : kp_options{0.075, 0, 0};
  c->device = c->opts.device;
  if (c->device < 0 || c->device >= n) {
    delete c;
    return fail(KP_E_INVAL, "device %d out of range", opts ? opts->device : 0);
  }
  if (hipSetDevice(c->device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
      hipEventCreate(&c->ev2) != hipSuccess || hipEventCreate(&c->ev3) != hipSuccess) {
    delete c;
    return fail(KP_E_DEVICE, "stream/event creation failed");
  }
  *out = c;
  return KP_OK;
}
void kp_ctx_destroy(kp_ctx* c) { CtxUnref(c); }

int32_t kp_ctx_set_overrides(kp_ctx* ctx, const kp_overrides* ov) {
  if (!ctx) return fail(KP_E_INVAL, "null argument");
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  ctx->ov = ov ? *ov : kp_overrides{};
  g_host_timing.store(ctx->ov.host_timing != 0);
  return KP_OK;
}
int32_t kp_ctx_get_overrides(const kp_ctx* ctx, kp_overrides* out) {
  if (!ctx || !out) return fail(KP_E_INVAL, "null argument");
  *out = ctx->ov;
  return KP_OK;
}


int32_t kp_catalog_upload(kp_ctx* ctx, const kp_catalog_desc* desc, uint64_t seqnum, kp_catalog** out) {
  if (!desc || !out) return fail(KP_E_INVAL, "null argument");  // ctx NULL: host-only (kp_solve_validate)
  if (desc->n_types > 4096) return fail(KP_E_UNSUPPORTED, "%u instance types (max 4096)", desc->n_types);
  // the price domain (kp_abi.h): the device orders prices by their bit patterns, which holds for p >= +0.0 only
  for (uint32_t i = 0; i < desc->n_types; i++)
    for (uint32_t j = 0; j < desc->types[i].n_offerings; j++) {
      const double p = desc->types[i].offerings[j].price;
      if (std::isnan(p) || p < 0)
        return fail(KP_E_INVAL, "type %u (%s): offering %u has price %g (a price is a number >= 0)", i,
                    desc->types[i].name ? desc->types[i].name : "", j, p);
    }
  static std::atomic<uint64_t> next_uid{1};
  auto* c = new kp_catalog();
  c->ctx = ctx;
  c->seqnum = seqnum;
  c->uid = next_uid.fetch_add(1);
  for (uint32_t i = 0; i < desc->n_types; i++) {
    const kp_instance_type& t = desc->types[i];
    HostType h;
    h.name = t.name ? t.name : "";
    h.reqs = ParseReqs(t.requirements);
    for (int r = 0; r < KP_NRES; r++) {
      h.cap[r] = t.capacity.milli[r];
      h.ovh[r] = (t.overhead.present >> r) & 1 ? t.overhead.milli[r] : 0;
    }
    h.cap_present = t.capacity.present;
    for (uint32_t j = 0; j < t.n_offerings; j++) {
      const kp_offering& o = t.offerings[j];
      h.offs.push_back({o.capacity_type ? o.capacity_type : "", o.zone ? o.zone : "", o.zone_id ? o.zone_id : "",
                        o.zone != nullptr, o.zone_id != nullptr, o.price + 0.0, o.available != 0});  // (-0.0 -> +0.0)
      HostOffering& ho = h.offs.back();
      ho.has_rid = o.reservation_id != nullptr;
      ho.has_rt = o.reservation_type != nullptr;
      if (ho.has_rid) ho.rid = o.reservation_id;
      if (ho.has_rt) ho.rt = o.reservation_type;
      ho.rcap = o.reservation_capacity;
      c->reservations = c->reservations || ho.has_rid || ho.has_rt;
    }
    c->types.push_back(std::move(h));
  }
  *out = c;
  return KP_OK;
}
uint64_t kp_catalog_seqnum(const kp_catalog* c) { return c ? c->seqnum : 0; }
uint32_t kp_catalog_size(const kp_catalog* c) { return c ? (uint32_t)c->types.size() : 0; }
namespace {
void DropBasesOf(kp_ctx* ctx, const kp_catalog* c);
}
// A catalogue may be destroyed while plans prepared on it still exist: they (and the ctx's cached bases, which are
// dropped here) see its alive token cleared and return KP_E_INVAL instead of reading it.
void kp_catalog_destroy(kp_catalog* c) {
  if (!c) return;
  std::unique_lock<std::recursive_mutex> lock;
  if (c->ctx) {
    lock = std::unique_lock<std::recursive_mutex>(c->ctx->mu);
    DropBasesOf(c->ctx, c);
  }
  *c->alive = false;
  if (lock.owns_lock()) lock.unlock();  // (the delete may drop the context's last reference)
  delete c;
}

// UnavailableOfferings.MarkUnavailable + SeqNum bump (R:pkg/cache/unavailableofferings.go:66-92) on the uploaded
// offerings; the next prepare (or kp_filter_refresh) rebuilds Available exactly as createOfferings does
// (R:offering.go:115-147). Validated in full before anything changes.
int32_t kp_catalog_update_offerings(kp_catalog* c, const kp_offering_update* ups, uint32_t n, uint64_t seqnum) {
  if (!c || (!ups && n)) return fail(KP_E_INVAL, "null argument");
  // serialized with every prepare / refresh / run of the catalogue's context (they read c->types)
  std::unique_lock<std::recursive_mutex> lock;
  if (c->ctx) lock = std::unique_lock<std::recursive_mutex>(c->ctx->mu);
  auto match = [](const HostOffering& o, const kp_offering_update& u) {
    if (o.ct != (u.capacity_type ? u.capacity_type : "")) return false;
    if (u.reservation_id && !(o.has_rid && o.rid == u.reservation_id)) return false;
    return u.zone ? (o.has_zone && o.zone == u.zone) : !o.has_zone;
  };
  for (uint32_t i = 0; i < n; i++) {
    if (ups[i].type >= c->types.size())
      return fail(KP_E_INVAL, "update %u: type %u of %zu", i, ups[i].type, c->types.size());
    if (ups[i].price < 0)  // (NaN: keep; the price domain of kp_abi.h otherwise)
      return fail(KP_E_INVAL, "update %u: type %u (%s) given price %g (a price is a number >= 0)", i, ups[i].type,
                  c->types[ups[i].type].name.c_str(), ups[i].price);
    bool any = false;
    for (auto& o : c->types[ups[i].type].offs) {
      if (!match(o, ups[i])) continue;
      any = true;
      // a reserved offering is Available only with capacity left (R:offering.go:178 ReservationCapacity != 0 &&
      // zone in itZones): an update giving capacity 0 with available set names a state upstream cannot reach
      if ((o.has_rid || o.ct == "reserved") && ups[i].reservation_capacity == 0 && ups[i].available)
        return fail(KP_E_INVAL, "update %u: reserved offering of type %u available with reservation capacity 0", i,
                    ups[i].type);
    }
    if (!any) return fail(KP_E_INVAL, "update %u names no offering of type %u", i, ups[i].type);
  }
  for (uint32_t i = 0; i < n; i++)
    for (auto& o : c->types[ups[i].type].offs)
      if (match(o, ups[i])) {
        o.available = ups[i].available != 0;
        if (!std::isnan(ups[i].price)) o.price = ups[i].price + 0.0;  // (-0.0 -> +0.0)
        if (ups[i].reservation_capacity >= 0) o.rcap = ups[i].reservation_capacity;
      }
  c->seqnum = seqnum;
  return KP_OK;
}

namespace {
int64_t EniLimitedPods(const kp_ec2_info* info, int reserved) {  // ENILimitedPods (R:types.go:461-475)
  int64_t usable = std::max<int64_t>((int64_t)info->max_enis - reserved, 0);
  return usable == 0 ? 0 : usable * ((int64_t)info->ipv4_per_eni - 1) + 2;
}
void SetRes(kp_resource_list* l, int r, int64_t v) {
  l->milli[r] = v;
  l->present |= 1u << r;
}
struct FamilyFlags;
int64_t PodsOf(const kp_options* opts, const kp_ec2_info* info, const kp_nodeclass* nc);
int64_t MemoryBytes(const kp_options* opts, const kp_ec2_info* info) {  // memory() (R:types.go:337-347)
  int64_t mib = info->memory_mib;
  if (info->arch && strcmp(info->arch, "arm64") == 0) mib -= 64;  // Graviton CMA
  const int64_t ovMiB = (int64_t)std::ceil((double)(mib * 1048576ll) * opts->vm_memory_overhead_percent / 1024 / 1024);
  return (mib - ovMiB) * 1048576ll;
}
// An AMI family's FeatureFlags and its default ephemeral volume (no blockDeviceMappings on the nodeclass):
// DefaultFamily (AL2023, AL2, Custom) R:amifamily/resolver.go:110-117; Bottlerocket :126-132 (/dev/xvdb, DefaultEBS);
// Windows windows.go:101-108 (/dev/sda1, 50Gi); the others DefaultEBS 20Gi (resolver.go:39-43).
struct FamilyFlags {
  bool eni_memory, pods_per_core, eviction_soft, eni_density, windows;
  int64_t storage_bytes;
};
// ephemeralStorage (R:pkg/providers/instancetype/types.go:349-385), in bytes: instanceStorePolicy RAID0 -> the
// instance store's total size ("%dG"); else the first root-volume BDM with a volumeSize; else for Custom the last
// BDM's volumeSize or DefaultEBS (20Gi), for the other families the first BDM on the family's ephemeral device
// (R:amifamily al2023.go:106-108, al2.go:114-116, bottlerocket.go:110-112, windows.go:97-99) with a volumeSize;
// else the family's default BDM on that device (Bottlerocket :95-108 and the DefaultEBS families 20Gi, Windows
// :88-95 50Gi, Custom none: DefaultEBS).
int64_t EphemeralBytes(const kp_ec2_info* info, const kp_nodeclass* nc) {
  const int64_t kDefaultEBS = 20ll << 30;
  const int f = nc ? nc->ami_family : KP_AMI_AL2023;
  const bool windows = f == KP_AMI_WINDOWS2019 || f == KP_AMI_WINDOWS2022;
  if (nc && nc->instance_store_policy == KP_INSTANCE_STORE_RAID0) {
    const int64_t gb = info->instance_storage_gb > 0 ? info->instance_storage_gb : info->local_nvme_gb;
    if (gb > 0) return gb * 1000000000ll;
  }
  if (nc && nc->n_block_device_mappings && nc->block_device_mappings) {
    const kp_block_device_mapping* b = nc->block_device_mappings;
    const uint32_t n = nc->n_block_device_mappings;
    for (uint32_t i = 0; i < n; i++)
      if (b[i].root_volume) {  // lo.Find: the first root volume only
        if (b[i].volume_size >= 0) return b[i].volume_size;
        break;
      }
    if (f == KP_AMI_CUSTOM) return b[n - 1].volume_size >= 0 ? b[n - 1].volume_size : kDefaultEBS;
    const char* dev = f == KP_AMI_BOTTLEROCKET ? "/dev/xvdb" : windows ? "/dev/sda1" : "/dev/xvda";
    for (uint32_t i = 0; i < n; i++)
      if (b[i].device_name && strcmp(b[i].device_name, dev) == 0) {
        if (b[i].volume_size >= 0) return b[i].volume_size;
        break;
      }
  }
  return windows ? 50ll << 30 : kDefaultEBS;
}

FamilyFlags Family(const kp_nodeclass* nc) {
  const int f = nc ? nc->ami_family : KP_AMI_AL2023;
  if (f == KP_AMI_BOTTLEROCKET) return {false, false, false, true, false, 20ll << 30};
  if (f == KP_AMI_WINDOWS2019 || f == KP_AMI_WINDOWS2022) return {false, true, true, false, true, 50ll << 30};
  return {true, true, true, true, false, 20ll << 30};
}

// pods() (R:types.go:553-569): maxPods, else ENI-limited when the family supports it, else 110; then podsPerCore
int64_t PodsOf(const kp_options* opts, const kp_ec2_info* info, const kp_nodeclass* nc) {
  const FamilyFlags fam = Family(nc);
  int64_t pods = (nc && nc->max_pods >= 0) ? nc->max_pods : fam.eni_density ? EniLimitedPods(info, opts->reserved_enis) : 110;
  if (nc && nc->pods_per_core > 0 && fam.pods_per_core) pods = std::min<int64_t>((int64_t)nc->pods_per_core * info->vcpu, pods);
  return pods;
}

// computeEvictionSignal (R:types.go:571-598) in milli-units: a percentage p of the capacity (100% disables the
// threshold) as ceil(capacity / 100 * p) whole units, else the quantity itself.
int64_t EvictionSignalMilli(int64_t capacity_units, const kp_eviction_value& v) {
  if (!v.is_percent) return v.milli;
  const double p = v.percent == 100.0 ? 0.0 : v.percent;
  return (int64_t)std::ceil((double)capacity_units / 100 * p) * 1000;
}
}  // namespace

int32_t kp_instance_type_overhead(const kp_options* opts, const kp_ec2_info* info, const kp_nodeclass* nc,
                                  kp_resource_list* kube, kp_resource_list* sys, kp_resource_list* ev) {
  if (!opts || !info || !kube || !sys || !ev) return fail(KP_E_INVAL, "null argument");
  const kp_kubelet* kl = nc ? nc->kubelet : nullptr;
  memset(kube, 0, sizeof *kube);
  memset(sys, 0, sizeof *sys);
  memset(ev, 0, sizeof *ev);
  const FamilyFlags fam = Family(nc);
  const int64_t kStorageBytes = EphemeralBytes(info, nc);
  // kubeReservedResources: UsesENILimitedMemoryOverhead -> memory from ENILimitedPods(info, 0), else from pods(); the
  // CPU ranges accumulate with a truncation per range; then the user's keys replace the computed ones (lo.Assign)
  SetRes(kube, KP_RES_MEMORY, (11 * (fam.eni_memory ? EniLimitedPods(info, 0) : PodsOf(opts, info, nc)) + 255) * 1048576ll * 1000ll);
  SetRes(kube, KP_RES_EPHEMERAL_STORAGE, (1ll << 30) * 1000);
  const struct {
    int64_t s, e;
    double p;
  } rg[4] = {{0, 1000, 0.06}, {1000, 2000, 0.01}, {2000, 4000, 0.005}, {4000, 1ll << 31, 0.0025}};
  const int64_t cpuM = (int64_t)info->vcpu * 1000;
  int64_t cpuOverhead = 0;
  for (auto& x : rg)
    if (cpuM >= x.s) cpuOverhead += (int64_t)((double)(cpuM < x.e ? cpuM - x.s : x.e - x.s) * x.p);
  SetRes(kube, KP_RES_CPU, cpuOverhead);
  if (kl)
    for (int r = 0; r < KP_NUM_RESOURCES; r++)
      if (kl->kube_reserved.present & (1u << r)) SetRes(kube, r, kl->kube_reserved.milli[r]);
  // systemReservedResources: exactly the user's map
  if (kl)
    for (int r = 0; r < KP_NUM_RESOURCES; r++)
      if (kl->system_reserved.present & (1u << r)) SetRes(sys, r, kl->system_reserved.milli[r]);
  // evictionThreshold: defaults, then MaxResources over the signal maps (hard, then soft), assigned over them
  SetRes(ev, KP_RES_MEMORY, 100ll * 1048576ll * 1000ll);
  SetRes(ev, KP_RES_EPHEMERAL_STORAGE, (int64_t)std::ceil((double)kStorageBytes / 100 * 10) * 1000);
  if (kl) {
    const int64_t memBytes = MemoryBytes(opts, info);
    kp_resource_list ov{};
    auto fold = [&](const kp_eviction_value& mem, const kp_eviction_value& fs) {
      if (mem.set) {
        const int64_t v = EvictionSignalMilli(memBytes, mem);
        if (!(ov.present & (1u << KP_RES_MEMORY)) || v > ov.milli[KP_RES_MEMORY]) SetRes(&ov, KP_RES_MEMORY, v);
      }
      if (fs.set) {
        const int64_t v = EvictionSignalMilli(kStorageBytes, fs);
        if (!(ov.present & (1u << KP_RES_EPHEMERAL_STORAGE)) || v > ov.milli[KP_RES_EPHEMERAL_STORAGE])
          SetRes(&ov, KP_RES_EPHEMERAL_STORAGE, v);
      }
    };
    if (kl->has_eviction_hard) fold(kl->hard_memory_available, kl->hard_nodefs_available);
    if (kl->has_eviction_soft && fam.eviction_soft) fold(kl->soft_memory_available, kl->soft_nodefs_available);
    for (int r = 0; r < KP_NUM_RESOURCES; r++)
      if (ov.present & (1u << r)) SetRes(ev, r, ov.milli[r]);
  }
  return KP_OK;
}

// instancetype.NewInstanceType capacity + Overhead.Total() for the nodeclass's AMI family (R:types.go:123-155, 313-598).
int32_t kp_instance_type_resolve(const kp_options* opts, const kp_ec2_info* info, const kp_nodeclass* nc,
                                 kp_resource_list* capacity, kp_resource_list* overhead) {
  if (!opts || !info || !capacity || !overhead) return fail(KP_E_INVAL, "null argument");
  memset(capacity, 0, sizeof *capacity);
  memset(overhead, 0, sizeof *overhead);
  SetRes(capacity, KP_RES_CPU, (int64_t)info->vcpu * 1000);
  SetRes(capacity, KP_RES_MEMORY, MemoryBytes(opts, info) * 1000);
  const FamilyFlags fam = Family(nc);
  SetRes(capacity, KP_RES_EPHEMERAL_STORAGE, EphemeralBytes(info, nc) * 1000);
  SetRes(capacity, KP_RES_PODS, PodsOf(opts, info, nc) * 1000);
  SetRes(capacity, KP_RES_POD_ENI, (info->in_limits_table && info->trunking) ? (int64_t)info->branch_enis * 1000 : 0);
  const string gm = info->gpu_manufacturer ? info->gpu_manufacturer : "";
  SetRes(capacity, KP_RES_NVIDIA_GPU, gm == "nvidia" ? info->gpu_count * 1000ll : 0);
  SetRes(capacity, KP_RES_AMD_GPU, gm == "amd" ? info->gpu_count * 1000ll : 0);
  SetRes(capacity, KP_RES_NEURON, (int64_t)info->neuron_devices * 1000);
  SetRes(capacity, KP_RES_NEURONCORE, (int64_t)info->neuron_devices * info->neuron_cores_per_device * 1000);
  SetRes(capacity, KP_RES_GAUDI, gm == "habana" ? info->gpu_count * 1000ll : 0);
  SetRes(capacity, KP_RES_EFA, (int64_t)info->efa * 1000);
  // Windows: the os requirement is windows only for amd64 types (getOS), which then get PrivateIPv4Address
  if (fam.windows && info->arch && strcmp(info->arch, "amd64") == 0)
    SetRes(capacity, KP_RES_PRIVATE_IPV4, info->in_limits_table ? ((int64_t)info->ipv4_per_eni - 1) * 1000 : 0);
  kp_resource_list parts[3];
  int32_t rc = kp_instance_type_overhead(opts, info, nc, &parts[0], &parts[1], &parts[2]);
  if (rc != KP_OK) return rc;
  for (auto& l : parts)  // InstanceTypeOverhead.Total(): resources.Merge of the three lists
    for (int r = 0; r < KP_NUM_RESOURCES; r++)
      if (l.present & (1u << r)) SetRes(overhead, r, overhead->milli[r] + l.milli[r]);
  return KP_OK;
}

}  // extern "C"

// ==================================================================================================
// Solve
// ==================================================================================================
namespace {

struct TaintT {
  string key, value;
  int effect;
  bool operator<(const TaintT& o) const { return std::tie(key, value, effect) < std::tie(o.key, o.value, o.effect); }
};

// The part of a Solve's compiled form that depends only on the catalogues (identity + seqnum) and the NodePools:
// the string dictionary, every catalogue SoA, the offering classes and the NodeClaimTemplates (upstream
// NewScheduler's per-template pre-filter). It is built on a cache miss and kept resident (host + device) in the
// kp_ctx across Solves, keyed by that fingerprint (R:pkg/providers/instancetype/instancetype.go:225-237 cacheKey:
// the reference likewise rebuilds its InstanceType list only when a seqnum changes). A Solve whose pods or nodes
// name a label key or value the dictionary lacks triggers a rebuild that adds them (the dictionary only grows).
// Device offsets of one catalogue's arrays inside an upload blob.
struct CatOffsets {
  size_t TM, DNE, NOKEY, alloc, cap, nonneg, fit_vals, fit_n, fit_mask, cls, offer, price, price_cm, price_sub, rank, code, multi, custom;
};

struct SolveBase {
  Dict d;
  int TW = 1, C = 0;
  vector<HostCat> cats;
  vector<OfferClass> classes;
  // templates (weight desc, name asc; pools whose requirements filter out every type are skipped)
  vector<int> tmpl_nodepool;          // index into kp_solve_in.nodepools
  vector<KReqs> tmpl_reqs;
  vector<int32_t> tmpl_taintset, tmpl_catalog;
  vector<uint64_t> tmpl_X;
  vector<int64_t> tmpl_daemon;
  vector<vector<TaintT>> tsets;       // the NodePools' taint sets in id order
  vector<int> np_taintset;            // per input NodePool
  // the NodePools as the templates need them (input order; np_order = weight desc, name asc), so that an ICE update
  // can rebuild the templates' options without the caller's kp_solve_in
  vector<KReqs> np_q;
  vector<int32_t> np_catalog;
  vector<int> np_order;
  vector<int64_t> np_daemon;          // [n_nodepools][NRES]
  vector<const kp_catalog*> catalogs; // the catalogues compiled in (caller-owned; see alive)
  vector<std::shared_ptr<bool>> alive; // their kp_catalog::alive tokens: a destroyed one makes the base unusable
  vector<uint64_t> seqnums;           // their seqnums the offering arrays reflect
  string ident;                       // cache fingerprint without the seqnums
  string key;                         // cache fingerprint: ident + seqnums
  uint64_t version = 0;               // bumped by every in-place offering refresh (RefreshOfferings)
  // device copy (Solve plans): dict, parsed integers, catalogue SoA + descriptors, templates
  DevBuf dev;
  bool on_device = false;
  size_t o_dict = 0, o_vint = 0, o_cats = 0, o_treqs = 0, o_tts = 0, o_tcat = 0, o_tX = 0, o_tdm = 0;
  vector<CatOffsets> coffs;
  double build_ms = 0;
  // capacity reservations (NewReservationManager): the reserved offering classes (one per reservation id) and the
  // least ReservationCapacity the NodePools' catalogues report for each
  uint64_t res_cls = 0;
  vector<int32_t> res_cap0;
};

// NewReservationManager's starting capacities (UP reservationmanager.go: the least ReservationCapacity any NodePool's
// instance types report for an id). Requires one class per reservation id (a reservation is one type in one zone).
int32_t ReservationTables(SolveBase& b) {
  b.res_cls = 0;
  b.res_cap0.assign(KP_MAX_CLASSES, 0);
  const int ct = b.d.key(kCapType), res = ct >= 0 ? b.d.bit(ct, "reserved") : -1;
  if (res < 0) return KP_OK;
  map<int, int> rid_class;
  for (int c = 0; c < b.C; c++) {
    if (b.classes[c].ct_bit != res) continue;
    if (b.classes[c].rid_bit < 0) return fail(KP_E_UNSUPPORTED, "reserved offering class without a reservation id");
    if (!rid_class.emplace(b.classes[c].rid_bit, c).second)
      return fail(KP_E_UNSUPPORTED, "one capacity reservation in two offering classes");
    b.res_cls |= 1ull << c;
    b.res_cap0[c] = INT32_MAX;
  }
  if (!b.res_cls) return KP_OK;
  map<ClassKey, int> classes;
  for (int c = 0; c < b.C; c++) classes[KeyOfClass(b.classes[c])] = c;
  for (int np = 0; np < (int)b.np_catalog.size(); np++)
    for (auto& t : b.catalogs[b.np_catalog[np]]->types)
      for (auto& o : t.offs) {
        const int c = classes.at(ClassOf(b.d, o));
        if ((b.res_cls >> c) & 1) b.res_cap0[c] = std::min(b.res_cap0[c], std::max(o.rcap, 0));
      }
  for (int c = 0; c < b.C; c++)
    if (b.res_cap0[c] == INT32_MAX) b.res_cap0[c] = 0;  // only in catalogues no NodePool uses
  return KP_OK;
}

struct Compiled {
  kp_overrides ov{};  // the context's overrides at compile time (CompileSolve with a ctx)
  std::shared_ptr<SolveBase> B = std::make_shared<SolveBase>();
  bool base_hit = false;              // the base came from the ctx cache
  bool base_refreshed = false;        // ... after an in-place offering refresh (a new catalogue seqnum)
  vector<uint32_t> tmpl_limit_present;
  vector<int64_t> tmpl_remaining;
  // shapes
  vector<int32_t> shape_level_base, shape_nlevels;
  int32_t cont_hint = 0;  // SolveArgs::cont: 1 most queue neighbours share their shape, 3 their request class
  vector<KReqs> shape_reqs;
  vector<uint64_t> shape_negop, shape_tolerates;  // per shape-level (tolerations change at the PreferNoSchedule level)
  vector<char> sl_pns;                             // per shape-level: toleratePreferNoScheduleTaints' level
  vector<int64_t> shape_requests;
  vector<int32_t> shape_rclass;  // per shape: request class (SolveArgs::shape_rclass)
  int32_t n_rclass = 0;          // ... and how many there are
  // requirement classes (SolveArgs::sl_rqc): class per shape-level, CSR of each class's member levels, and the class
  // of the empty requirement set (-1: none)
  vector<int32_t> sl_rqc, rqc_off, rqc_mem;
  int32_t rqc_empty = -1;
  vector<uint64_t> pvp;
  vector<int32_t> pvp_base, pvp_slot, pvp_n;  // pvp_n: rows of catalogue 0 per shape-level
  // existing (sorted)
  vector<int> ex_input;
  vector<KReqs> ex_reqs;
  vector<int32_t> ex_taintset;
  vector<int64_t> ex_available, ex_requests;
  // host ports (HostPortUsage): conflict / add masks per shape over the batch's port bits, used bits per node
  vector<uint64_t> shape_hp_conf, shape_hp_add, ex_hp;
  bool hp_any = false;
  // pods
  vector<int32_t> pod_shape, queue;
  // topology spread (TopologyTypeSpread groups; see SolveArgs)
  int G = 0, GH = 0, TK = 0;
  vector<int32_t> tg_key, tg_row, tg_maxskew, tg_mindom, tg_aff, tg_term_base, tg_nterm;
  vector<uint64_t> tg_filt_tol, tg_reg, tg_terms_negop;
  vector<KReqs> tg_terms;
  vector<int32_t> tg_cnt;    // [G][64]
  vector<int32_t> tg_live;   // [G] 1: the group exists (NewTopology, or a Topology.Update made it); Record skips others
  vector<uint8_t> hcnt0;     // [GH][E]
  vector<int32_t> shape_rec_base, shape_rec_n, rec_list;
  vector<int32_t> sl_own_base, sl_own_n, own_group, own_self;
  vector<int32_t> sl_fast_topo;  // [SL] 1: the fast lane may place the level's pods (append path; see CompileTopology)
  vector<int32_t> rec_aux;       // per rec_list entry: the group's hostname row, else -1 - its key's slot
  vector<int32_t> own_rec;  // [O][8] static part of an owned group: group, self, key, maxSkew, minDomains, row, key slot, 0
  vector<uint64_t> own_pd, sl_topo_keys;
  vector<int32_t> tkey_slot;  // [64]
  vector<int32_t> tk_keys;    // [TK]
  vector<uint8_t> ex_tcode;   // [TK][E]
  // What each existing node (input index) contributes to the topology state, recorded by CompileTopology when
  // track_nodes is set: the batched general-path simulations (GeneralBatch) remove a subset's nodes from it.
  bool track_nodes = false;
  vector<vector<int32_t>> node_cnt;  // [n_existing] tg_cnt entries (g * 64 + ordinal), one per bound pod counted
  vector<vector<int32_t>> node_reg;  // [n_existing] (g * 64 + ordinal): a domain the node registers in dictionary-key group g
  vector<vector<int32_t>> node_hrec; // [n_existing] hostname-row groups a bound pod on the node was recorded into
  vector<vector<int32_t>> node_inv;  // [n_existing] inverse anti-affinity groups a bound pod on the node owns
  vector<uint64_t> tg_reg_static;    // [G] domains registered without any existing node (NodePool / type offerings)
  vector<int32_t> tg_hrec_total, tg_inv_total;  // [G]
  vector<vector<int32_t>> shape_l0;  // [S] the spread groups each shape makes at level 0 (NewTopology, if it has pods)
  vector<char> tg_spread;            // [G] 1: a topology-spread group
  vector<vector<int32_t>> tg_unreg;  // [G] hostname spread groups: positions (sorted order) unregistered (255) when the
                                     // group is created not live
};

// Requirements.Compatible(A, B, allowUndefinedWellKnown) on the host encoding.
bool HostCompatible(const Dict& d, const KReqs& A, const KReqs& B, bool allow) {
  const uint64_t negB = NegOp(d, B), negA = NegOp(d, A);
  uint64_t undef = B.present & ~A.present & ~negB;
  if (allow) undef &= ~d.dd.wellknown;
  if (undef) return false;
  KReqs m = A;
  HostAdd(d, m, B);
  const uint64_t shared = A.present & B.present;
  for (int k = 0; k < d.dd.K; k++) {
    if (!((shared >> k) & 1)) continue;
    const bool empty = !((m.compl_ >> k) & 1) && !KeyNonEmptyVals(d, m, k);  // Len() == 0
    if (empty && !(((negA & negB) >> k) & 1)) return false;
  }
  return true;
}

// Semantic canonical form of a requirement set (identity of a topology node filter).
string KCanon(const Dict& d, const KReqs& q) {
  string o;
  for (int k = 0; k < d.dd.K; k++) {
    if (!((q.present >> k) & 1)) continue;
    const bool bnd = k < KP_MAX_BOUND_KEYS;
    o += std::to_string(k) + ((q.compl_ >> k) & 1 ? "!" : "=");
    for (int i = 0; i < nwords(d, k); i++) o += std::to_string(q.vals[kw(d, k, i)]) + ",";
    if (bnd && ((q.hgt >> k) & 1)) o += ">" + std::to_string(q.gt[k]);
    if (bnd && ((q.hlt >> k) & 1)) o += "<" + std::to_string(q.lt[k]);
    if (bnd && ((q.hmin >> k) & 1)) o += "#" + std::to_string(q.minv[k]);
    o += ";";
  }
  return o;
}

// metav1.LabelSelector.Matches (nil selects nothing)
bool SelectorMatches(const kp_label_selector& sel, const std::map<string, string>& labels) {
  if (sel.is_nil) return false;
  for (uint32_t i = 0; i < sel.n_match_labels; i++) {
    auto it = labels.find(sel.match_labels[i].key ? sel.match_labels[i].key : "");
    if (it == labels.end() || it->second != (sel.match_labels[i].value ? sel.match_labels[i].value : "")) return false;
  }
  for (uint32_t i = 0; i < sel.n_match_expressions; i++) {
    const kp_selector_requirement& r = sel.match_expressions[i];
    auto it = labels.find(r.key ? r.key : "");
    const bool has = it != labels.end();
    bool in = false;
    for (uint32_t j = 0; has && j < r.n_values && !in; j++) in = it->second == (r.values[j] ? r.values[j] : "");
    switch (r.op) {
      case KP_SEL_IN:
        if (!in) return false;
        break;
      case KP_SEL_NOT_IN:
        if (in) return false;
        break;
      case KP_SEL_EXISTS:
        if (!has) return false;
        break;
      default:
        if (has) return false;
    }
  }
  return true;
}
string SelectorCanon(const kp_label_selector& sel) {
  if (sel.is_nil) return "nil";
  vector<string> parts;
  for (uint32_t i = 0; i < sel.n_match_labels; i++)
    parts.push_back(string(sel.match_labels[i].key) + "/0," + (sel.match_labels[i].value ? sel.match_labels[i].value : ""));
  for (uint32_t i = 0; i < sel.n_match_expressions; i++) {
    const kp_selector_requirement& r = sel.match_expressions[i];
    std::set<string> vs;
    for (uint32_t j = 0; j < r.n_values; j++) vs.insert(r.values[j] ? r.values[j] : "");
    string x = string(r.key) + "/" + std::to_string(r.op);
    for (auto& v : vs) x += "," + v;
    parts.push_back(x);
  }
  std::sort(parts.begin(), parts.end());
  string o;
  for (auto& x : parts) o += x + ";";
  return o;
}
std::map<string, string> LabelMap(const kp_label* l, uint32_t n) {
  std::map<string, string> m;
  for (uint32_t i = 0; i < n; i++) m[l[i].key ? l[i].key : ""] = l[i].value ? l[i].value : "";
  return m;
}

// Topology spread groups (upstream NewTopology / TopologyGroup / countDomains / buildDomainGroups), in the
// device encoding: one group per distinct (key, maxSkew, namespace, selector, node filter, policies) in order
// of first appearance over the pods; dictionary-key groups keep a count per value ordinal + a registered-
// domain mask, hostname groups a saturating u8 count per node (existing positions, then NodeClaims).
// A pod's podAntiAffinity terms in one list: required terms, then preferred ones (spec order).
// A pod's inter-pod terms in one list: required anti-affinity, preferred anti-affinity, required affinity, preferred
// affinity (spec order within each). *aff: the term is a podAffinity term.
uint32_t PodTermCount(const kp_pod_shape& sh) {
  return sh.n_required_anti_affinity + sh.n_preferred_anti_affinity + sh.n_required_affinity + sh.n_preferred_affinity;
}
const kp_pod_affinity_term* PodTermAt(const kp_pod_shape& sh, int a, bool* aff = nullptr) {
  const uint32_t n[4] = {sh.n_required_anti_affinity, sh.n_preferred_anti_affinity, sh.n_required_affinity,
                         sh.n_preferred_affinity};
  const kp_pod_affinity_term* p[4] = {sh.required_anti_affinity, sh.preferred_anti_affinity, sh.required_affinity,
                                      sh.preferred_affinity};
  for (int i = 0; i < 4; i++) {
    if (a < (int)n[i]) {
      if (aff) *aff = i >= 2;
      return &p[i][a];
    }
    a -= (int)n[i];
  }
  return nullptr;
}
int32_t CheckAntiTerm(const kp_pod_affinity_term& t, const char* who, uint32_t i) {
  if (!t.topology_key || !t.topology_key[0]) return fail(KP_E_INVAL, "%s %u: pod (anti-)affinity without topologyKey", who, i);
  return KP_OK;
}

// HostPortUsage.Conflicts as bit masks. Bits: U(g) per (protocol, port) group g some unspecified-IP entry names,
// S(g, ip) per specific entry. An entry (g, unspecified) conflicts with every used bit of g and adds U(g); an
// entry (g, ip) conflicts with U(g) and S(g, ip) and adds S(g, ip) — HostPort.Matches (same protocol and port, and
// an unspecified IP on either side or equal IPs). A node's used bits only grow, so a conflict is permanent.
int32_t EncodeHostPorts(const vector<vector<HostPortKey>>& shapes, const vector<vector<HostPortKey>>& nodes,
                        Compiled& cp) {
  std::map<std::pair<int, int>, int> ubit;                               // group -> U bit
  std::map<std::pair<std::pair<int, int>, std::array<uint8_t, 16>>, int> sbit;  // (group, ip) -> S bit
  std::map<std::pair<int, int>, uint64_t> gmask;                         // every bit of a group
  int nb = 0;
  auto visit = [&](const vector<HostPortKey>& v) {
    for (auto& k : v) {
      const auto g = std::make_pair(k.proto, k.port);
      if (k.unspec) {
        if (!ubit.count(g)) ubit[g] = nb++;
      } else if (!sbit.count({g, k.ip})) {
        sbit[{g, k.ip}] = nb++;
      }
    }
  };
  for (auto& v : shapes) visit(v);
  for (auto& v : nodes) visit(v);
  if (nb > 64) return fail(KP_E_UNSUPPORTED, "%d distinct host port entries (max 64)", nb);
  for (auto& kv : ubit) gmask[kv.first] |= 1ull << kv.second;
  for (auto& kv : sbit) gmask[kv.first.first] |= 1ull << kv.second;
  auto masks = [&](const vector<HostPortKey>& v, uint64_t* conf, uint64_t* add) {
    *conf = *add = 0;
    for (auto& k : v) {
      const auto g = std::make_pair(k.proto, k.port);
      auto u = ubit.find(g);
      const uint64_t ub = u == ubit.end() ? 0 : 1ull << u->second;
      if (k.unspec) {
        *conf |= gmask[g];
        *add |= ub;
      } else {
        const uint64_t sb = 1ull << sbit[{g, k.ip}];
        *conf |= ub | sb;
        *add |= sb;
      }
    }
  };
  cp.shape_hp_conf.assign(shapes.size(), 0);
  cp.shape_hp_add.assign(shapes.size(), 0);
  for (size_t i = 0; i < shapes.size(); i++) masks(shapes[i], &cp.shape_hp_conf[i], &cp.shape_hp_add[i]);
  cp.ex_hp.assign(nodes.size(), 0);
  for (size_t i = 0; i < nodes.size(); i++) {
    uint64_t c;
    masks(nodes[i], &c, &cp.ex_hp[i]);
  }
  cp.hp_any = nb > 0;
  return KP_OK;
}

// the toleration Preferences.toleratePreferNoScheduleTaints appends, and whether the pod already carries it
// (corev1 Toleration.MatchToleration: equal key, operator, value and effect)
const kp_toleration kPnsToleration = {"", "", KP_TOL_EXISTS, KP_EFFECT_PREFER_NO_SCHEDULE};
bool HasPnsToleration(const kp_pod_shape& sh) {
  for (uint32_t j = 0; j < sh.n_tolerations; j++) {
    const kp_toleration& t = sh.tolerations[j];
    if ((!t.key || !t.key[0]) && (!t.value || !t.value[0]) && t.op == KP_TOL_EXISTS &&
        t.effect == KP_EFFECT_PREFER_NO_SCHEDULE)
      return true;
  }
  return false;
}

// kp_overrides.host_timing: host compile phases on stderr (diagnostics only)
struct PhaseTimer {
  bool on = g_host_timing.load(std::memory_order_relaxed);
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void lap(const char* what) {
    if (!on) return;
    const auto n = std::chrono::steady_clock::now();
    fprintf(stderr, "[kp compile] %-22s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
    t = n;
  }
};

int32_t CompileTopology(const kp_solve_in* in, Compiled& cp, const vector<vector<RawReqs>>& strict_levels,
                        const vector<vector<vector<int>>>& spread_levels, const vector<int>& np_taintset,
                        const vector<vector<vector<RawReqs>>>& filter_levels) {
  const Dict& d = cp.B->d;
  const int E = (int)cp.ex_input.size();
  cp.tkey_slot.assign(KP_MAX_KEYS, -1);
  cp.shape_rec_base.assign(in->n_shapes, 0);
  cp.shape_rec_n.assign(in->n_shapes, 0);
  const size_t SL = cp.shape_reqs.size();
  cp.sl_own_base.assign(SL, 0);
  cp.sl_own_n.assign(SL, 0);
  cp.sl_topo_keys.assign(SL, 0);
  cp.sl_fast_topo.assign(SL, 1);
  bool any = false;
  for (uint32_t s = 0; s < in->n_shapes; s++)
    any |= in->shapes[s].n_topology_spread + PodTermCount(in->shapes[s]) > 0;
  for (uint32_t b = 0; b < in->n_bound_pods; b++) {
    for (uint32_t j = 0; j < in->bound_pods[b].n_anti_affinity; j++) {
      const int32_t rc = CheckAntiTerm(in->bound_pods[b].anti_affinity[j], "bound pod", b);
      if (rc) return rc;
    }
    any |= in->bound_pods[b].n_anti_affinity > 0;
  }
  if (!any) return KP_OK;
  PhaseTimer pt;
  if (cp.track_nodes) {
    cp.node_cnt.assign(in->n_existing, {});
    cp.node_reg.assign(in->n_existing, {});
    cp.node_hrec.assign(in->n_existing, {});
    cp.node_inv.assign(in->n_existing, {});
    cp.shape_l0.assign(in->n_shapes, {});
  }
  vector<int> ex_pos(in->n_existing);
  for (int e = 0; e < E; e++) ex_pos[cp.ex_input[e]] = e;
  vector<KReqs> node_reqs(in->n_existing);
  for (uint32_t i = 0; i < in->n_existing; i++) node_reqs[i] = cp.ex_reqs[ex_pos[i]];
  // the existing nodes' value of one label key (LabelMap's: the last entry wins; nullptr: no such label), computed
  // once per key that some group reads (a few keys against thousands of nodes)
  std::unordered_map<string, vector<const char*>> node_kv;
  auto node_vals = [&](const string& key) -> const vector<const char*>& {
    auto it = node_kv.find(key);
    if (it != node_kv.end()) return it->second;
    vector<const char*> v(in->n_existing, nullptr);
    for (uint32_t i = 0; i < in->n_existing; i++) {
      const kp_existing_node& e = in->existing[i];
      for (uint32_t j = 0; j < e.n_labels; j++)
        if (key == (e.labels[j].key ? e.labels[j].key : "")) v[i] = e.labels[j].value ? e.labels[j].value : "";
    }
    return node_kv.emplace(key, std::move(v)).first->second;
  };
  // ... and its value ordinal for a dictionary key k (-1: no such label)
  std::unordered_map<int, vector<int>> node_ko;
  auto node_ords = [&](int k) -> const vector<int>& {
    auto it = node_ko.find(k);
    if (it != node_ko.end()) return it->second;
    const vector<const char*>& v = node_vals(d.keys[k]);
    vector<int> o(in->n_existing, -1);
    for (uint32_t i = 0; i < in->n_existing; i++)
      if (v[i]) o[i] = d.bit(k, v[i]) - k * 64;
    return node_ko.emplace(k, std::move(o)).first->second;
  };
  // buildDomainGroups for one key: value ordinal -> taint sets of the NodePools offering it
  std::map<int, vector<uint64_t>> domain_tsets;  // key -> [64] taint-set masks
  auto domains_of = [&](int k) -> const vector<uint64_t>& {
    auto it = domain_tsets.find(k);
    if (it != domain_tsets.end()) return it->second;
    vector<uint64_t> m(64, 0);
    auto insert = [&](const KReqs& r, int ts) {
      if (!((r.present >> k) & 1) || ((r.compl_ >> k) & 1)) return;  // Operator() == In
      uint64_t v = r.vals[k];
      while (v) {
        const int b = __builtin_ctzll(v);
        v &= v - 1;
        m[b] |= 1ull << ts;
      }
    };
    for (uint32_t i = 0; i < in->n_nodepools; i++) {
      const kp_nodepool& np = in->nodepools[i];
      const HostCat& hc = cp.B->cats[np.catalog];
      if (hc.T == 0) continue;
      RawReqs base_raw = ParseReqs(np.requirements);
      RawReqs l = LabelReqs(np.labels, np.n_labels, false);
      base_raw.insert(base_raw.end(), l.begin(), l.end());
      const KReqs base = Compile(d, base_raw);
      for (int t = 0; t < hc.T; t++) {
        KReqs r = base;
        HostAdd(d, r, hc.treqs[t]);
        insert(r, np_taintset[i]);
      }
      insert(base, np_taintset[i]);
    }
    return domain_tsets[k] = m;
  };
  // bound pods grouped by (namespace, labels): deployments repeat one label set over many pods
  struct BoundSet {
    string ns;
    std::map<string, string> labels;
    vector<uint32_t> nodes;  // input indices, one entry per bound pod
  };
  vector<BoundSet> bsets;
  // the sets indexed by (namespace, label) and by namespace: a matchLabels selector only tests the sets carrying its
  // first label (index lists are in set order, so a group visits its sets in the order a full scan would)
  std::unordered_map<string, vector<int>> bs_by_label, bs_by_ns;
  {
    std::unordered_map<string, int> idx;  // canonical (namespace, LabelMap) -> set
    vector<std::pair<const char*, const char*>> kv;
    string canon;
    for (uint32_t b = 0; b < in->n_bound_pods; b++) {
      const kp_bound_pod& bp = in->bound_pods[b];
      if (bp.node >= in->n_existing) return fail(KP_E_INVAL, "bound pod %u: node %u", b, bp.node);
      // LabelMap without the map: the entries by key, stable, the last of equal keys kept
      kv.clear();
      for (uint32_t j = 0; j < bp.n_labels; j++)
        kv.push_back({bp.labels[j].key ? bp.labels[j].key : "", bp.labels[j].value ? bp.labels[j].value : ""});
      std::stable_sort(kv.begin(), kv.end(), [](const auto& x, const auto& y) { return strcmp(x.first, y.first) < 0; });
      canon.assign(bp.namespace_ ? bp.namespace_ : "");
      for (size_t j = 0; j < kv.size(); j++) {
        if (j + 1 < kv.size() && strcmp(kv[j].first, kv[j + 1].first) == 0) continue;
        canon += '\x01';
        canon += kv[j].first;
        canon += '\x02';
        canon += kv[j].second;
      }
      auto it = idx.find(canon);
      if (it == idx.end()) {
        const int id = (int)bsets.size();
        it = idx.emplace(canon, id).first;
        const string ns = bp.namespace_ ? bp.namespace_ : "";
        bsets.push_back({ns, LabelMap(bp.labels, bp.n_labels), {}});
        bs_by_ns[ns].push_back(id);
        for (auto& l : bsets.back().labels) bs_by_label[ns + '\x01' + l.first + '\x01' + l.second].push_back(id);
      }
      bsets[it->second].nodes.push_back(bp.node);
    }
  }
  static const vector<int> kNoSets;
  // the bound-pod sets a selector can match in namespace ns (a superset; callers still test SelectorMatches)
  auto sets_for = [&](const kp_label_selector& sel, const string& ns) -> const vector<int>& {
    if (sel.is_nil) return kNoSets;
    if (sel.n_match_labels) {
      auto it = bs_by_label.find(ns + '\x01' + (sel.match_labels[0].key ? sel.match_labels[0].key : "") + '\x01' +
                                 (sel.match_labels[0].value ? sel.match_labels[0].value : ""));
      return it == bs_by_label.end() ? kNoSets : it->second;
    }
    auto it = bs_by_ns.find(ns);
    return it == bs_by_ns.end() ? kNoSets : it->second;
  };
  pt.lap("  topo: labels+bsets");
  std::map<string, int> ids;
  std::map<string, uint64_t> node_domains;
  vector<int> g_shape;  // shape that created the group (its tolerations / filter)
  vector<const kp_topology_spread*> g_spec;
  vector<const kp_label_selector*> g_sel;   // every group: its selector
  vector<std::set<string>> g_nss;           // namespaces it selects in (spread: the owner's)
  vector<char> g_inverse;                   // inverse anti-affinity group (bound pods own it; never recorded)
  // group identity per (shape, spread index)
  vector<vector<int>> sgroup(in->n_shapes);
  vector<char> seen(in->n_shapes, 0);
  // A spread group at relaxation level l of shape s. MakeTopologyNodeFilter: the nodeSelector with each remaining
  // required node-affinity term (ORed); relaxing a term (Preferences.removeRequiredNodeAffinityTerm) changes the
  // filter and so the group identity: Topology.Update then makes a new group, counted from the cluster alone, which
  // exists (is live: records count into it) from that first relaxation on (upstream Topology.Update).
  auto group_of = [&](uint32_t s, int j, int l, bool live) -> int32_t {
    const kp_pod_shape& sh = in->shapes[s];
    const kp_topology_spread& t = sh.topology_spread[j];
    const string key = t.topology_key ? t.topology_key : "";
    const bool aff = t.node_affinity_policy != KP_POLICY_IGNORE, taint = t.node_taints_policy == KP_POLICY_HONOR;
    vector<KReqs> filts;
    for (auto& fr : filter_levels[s][l]) filts.push_back(Compile(d, fr));
    bool nonempty = true;  // an empty term admits every node: the filter is vacuous
    for (auto& f : filts) nonempty = nonempty && f.present != 0;
    string fcanon;
    for (auto& f : filts) fcanon += "[" + KCanon(d, f) + "]";
    string id = key + "|" + std::to_string(t.max_skew) + "|" + (sh.namespace_ ? sh.namespace_ : "") + "|" +
                SelectorCanon(t.selector) + "|" + std::to_string(aff) + std::to_string(taint) + "|" + fcanon;
    const int sl = cp.shape_level_base[s] + l;
    const uint64_t ltol = cp.shape_tolerates[sl];  // the level's tolerations (Relax may have appended one)
    // upstream MakeTopologyNodeFilter keeps the pod's tolerations under every taint policy and TopologyGroup.Hash
    // hashes the whole filter: the tolerations are part of the identity even when the policy ignores them (a pod
    // relaxed to tolerate PreferNoSchedule makes a new group, counted from the cluster alone)
    for (uint32_t i = 0; i < sh.n_tolerations + (cp.sl_pns[sl] ? 1 : 0); i++) {
      const kp_toleration& x = i < sh.n_tolerations ? sh.tolerations[i] : kPnsToleration;
      id += string("(") + (x.key ? x.key : "") + "," + (x.value ? x.value : "") + "," + std::to_string(x.op) + "," +
            std::to_string(x.effect) + ")";
    }
    auto it = ids.find(id);
    if (it != ids.end()) {
      if (live) cp.tg_live[it->second] = 1;
      return it->second;
    }
    const int g = cp.G++;
    ids[id] = g;
    cp.tg_live.push_back(live ? 1 : 0);
    g_shape.push_back((int)s);
    g_spec.push_back(&t);
    g_sel.push_back(&t.selector);
    g_nss.push_back({sh.namespace_ ? sh.namespace_ : ""});
    g_inverse.push_back(0);
    int k = -1, row = -1;
    if (key == kHostname) {
      row = cp.GH++;
    } else {
      k = d.key(key);
      if (k < 0) return fail(KP_E_INVAL, "topology key %s missing from the dictionary", key.c_str()), -1;
      if (d.dd.nval[k] > 64) return fail(KP_E_UNSUPPORTED, "topology key %s has > 64 values", key.c_str()), -1;
      if (cp.tkey_slot[k] < 0) {
        cp.tkey_slot[k] = cp.TK++;
        cp.tk_keys.push_back(k);
      }
    }
    cp.tg_key.push_back(k);
    cp.tg_row.push_back(row);
    cp.tg_maxskew.push_back(t.max_skew);
    cp.tg_mindom.push_back(t.min_domains > 0 ? t.min_domains : 0);
    // filter: affinity terms, ORed (none when a term is empty: everything matches)
    cp.tg_term_base.push_back((int32_t)cp.tg_terms.size());
    cp.tg_aff.push_back(aff && nonempty ? 1 : 0);
    cp.tg_nterm.push_back(aff && nonempty ? (int32_t)filts.size() : 0);
    if (aff && nonempty)
      for (auto& f : filts) {
        cp.tg_terms.push_back(f);
        cp.tg_terms_negop.push_back(NegOp(d, f));
      }
    cp.tg_filt_tol.push_back(taint ? ltol : ~0ull);
    // NewTopologyGroup: every known domain of the key, with a zero count (ForEachDomain + taint policy)
    uint64_t reg = 0;
    if (k >= 0) {
      const vector<uint64_t>& dm = domains_of(k);
      for (int b = 0; b < 64; b++)
        if (dm[b] && (!taint || (dm[b] & ltol))) reg |= 1ull << b;
    }
    cp.tg_reg.push_back(reg);
    for (int b = 0; b < 64; b++) cp.tg_cnt.push_back(0);
    if (row >= 0) cp.hcnt0.resize((size_t)cp.GH * std::max(E, 1), 0);
    if (cp.track_nodes) {
      cp.tg_reg_static.push_back(reg);
      cp.tg_hrec_total.push_back(0);
      cp.tg_inv_total.push_back(0);
      cp.tg_spread.push_back(1);
      cp.tg_unreg.emplace_back();
    }
    // countDomains: bound pods the selector matches, on nodes the filter admits; then existing nodes' domains
    auto filter_ok = [&](uint32_t ni) {
      const int ts = cp.ex_taintset[ex_pos[ni]];
      if (taint && !((ltol >> ts) & 1)) return false;
      if (!(aff && nonempty)) return true;
      for (auto& f : filts)
        if (HostCompatible(d, node_reqs[ni], f, false)) return true;
      return false;
    };
    const string ns = sh.namespace_ ? sh.namespace_ : "";
    const vector<int>* ords = k >= 0 ? &node_ords(k) : nullptr;  // value ordinal per node (key k's values: word k)
    for (int bi : sets_for(t.selector, ns)) {
      const BoundSet& bs = bsets[bi];
      if (!SelectorMatches(t.selector, bs.labels)) continue;
      for (const uint32_t ni : bs.nodes) {
        if (row >= 0) {  // hostname: the node's label or, failing that, its name — one domain per node
          if (!filter_ok(ni)) continue;
          uint8_t& c = cp.hcnt0[(size_t)row * std::max(E, 1) + ex_pos[ni]];
          if (c < 254) c++;  // (255: an unregistered domain, below)
        } else {
          const int ord = (*ords)[ni];
          if (ord < 0 || !filter_ok(ni)) continue;
          cp.tg_cnt[(size_t)g * 64 + ord]++;
          cp.tg_reg[g] |= 1ull << ord;
          if (cp.track_nodes) cp.node_cnt[ni].push_back(g * 64 + ord);
        }
      }
    }
    if (k >= 0) {  // the existing nodes' domains depend only on (key, node filter): cached across groups
      string fid = key + "|" + std::to_string(aff && nonempty) + fcanon + (taint ? std::to_string(ltol) : string("-"));
      auto it = node_domains.find(fid);
      if (it == node_domains.end()) {
        uint64_t m = 0;
        for (uint32_t ni = 0; ni < in->n_existing; ni++)
          if ((*ords)[ni] >= 0 && filter_ok(ni)) m |= 1ull << (*ords)[ni];
        it = node_domains.emplace(fid, m).first;
      }
      cp.tg_reg[g] |= it->second;
      if (cp.track_nodes)
        for (uint32_t ni = 0; ni < in->n_existing; ni++)
          if ((*ords)[ni] >= 0 && filter_ok(ni)) cp.node_reg[ni].push_back(g * 64 + (*ords)[ni]);
    }
    if (row >= 0 && E && (cp.track_nodes || !live)) {
      // the nodes this group registers: the filter-matching ones with a hostname label, and the nodes of the pods it
      // counted (both uses below)
      const vector<const char*>& hn = node_vals(kHostname);
      vector<char> counted(in->n_existing, 0);
      for (int bi : sets_for(t.selector, ns))
        if (SelectorMatches(t.selector, bsets[bi].labels))
          for (const uint32_t ni : bsets[bi].nodes) counted[ni] = 1;
      // the positions a not-live creation leaves unregistered (below)
      if (cp.track_nodes)
        for (uint32_t ni = 0; ni < in->n_existing; ni++)
          if (!(filter_ok(ni) && (hn[ni] || counted[ni]))) cp.tg_unreg[g].push_back(ex_pos[ni]);
      // a hostname group a relaxation creates (Topology.Update after NewTopology): its domains are only what
      // countDomains registers (NewTopology's Register of every existing node came before it). An unregistered node
      // holds 255: the spread test fails on it until a Record registers it; the NodeClaims created before the group
      // get 255 on the device when the group comes to exist.
      if (!live)
        for (uint32_t ni = 0; ni < in->n_existing; ni++)
          if (!(filter_ok(ni) && (hn[ni] || counted[ni]))) cp.hcnt0[(size_t)row * E + ex_pos[ni]] = 255;
    }
    return g;
  };
  // TopologyTypePodAntiAffinity on the hostname key, as a hostname row whose acceptance test is count == 0 (the
  // pre-pass test count + self <= maxSkew with self = 0, maxSkew = 0); no node filter; identity = (type, key,
  // namespaces, selector). countDomains: bound pods it selects, per node. inverse: a bound pod's own required term
  // (updateInverseAntiAffinity): its counts are the owners' nodes, it constrains the pods it selects, and no
  // placement records into it.
  // the namespaces a term selects (upstream Topology.buildNamespaceList): none given and no namespaceSelector -> the
  // pod's own; else the listed ones plus every cluster namespace whose labels the namespaceSelector matches
  auto nss_of = [&](const kp_pod_affinity_term& t, const char* pod_ns) {
    std::set<string> n;
    for (uint32_t i = 0; i < t.n_namespaces; i++) n.insert(t.namespaces[i] ? t.namespaces[i] : "");
    if (t.has_namespace_selector) {
      for (uint32_t i = 0; i < in->n_namespaces; i++) {
        const kp_namespace& ns = in->namespaces[i];
        std::map<string, string> labels;
        for (uint32_t j = 0; j < ns.n_labels; j++)
          labels[ns.labels[j].key ? ns.labels[j].key : ""] = ns.labels[j].value ? ns.labels[j].value : "";
        if (SelectorMatches(t.namespace_selector, labels)) n.insert(ns.name ? ns.name : "");
      }
    } else if (n.empty()) {
      n.insert(pod_ns ? pod_ns : "");
    }
    return n;
  };
  // TopologyTypePodAffinity (aff): the same hostname row with maxSkew = -1, whose pre-pass test is count > 0, or,
  // while no domain has a count (tg_reg bit 0 clear), the self-selecting pod's bootstrap (nextDomainAffinity).
  // one bound pod counted in group g on input node ni: hostname rows count per node (bit 0 of tg_reg: some domain
  // has a count); dictionary keys count per value ordinal of the node's label (none: not counted)
  auto record_bound = [&](int g, uint32_t ni) {
    if (cp.tg_row[g] >= 0) {
      uint8_t& c = cp.hcnt0[(size_t)cp.tg_row[g] * std::max(E, 1) + ex_pos[ni]];
      if (c < 254) c++;
      cp.tg_reg[g] |= 1;
      if (cp.track_nodes) {
        cp.node_hrec[ni].push_back(g);
        cp.tg_hrec_total[g]++;
      }
    } else {
      const int k = cp.tg_key[g];
      const int ord = node_ords(k)[ni];
      if (ord < 0) return;
      cp.tg_cnt[(size_t)g * 64 + ord]++;
      cp.tg_reg[g] |= 1ull << ord;
      if (cp.track_nodes) cp.node_cnt[ni].push_back(g * 64 + ord);
    }
  };
  auto anti_group = [&](const kp_pod_affinity_term& t, const std::set<string>& nss, bool inverse, bool aff = false) -> int {
    string id = string(inverse ? "inv|" : aff ? "aff|" : "anti|") + (t.topology_key ? t.topology_key : "") + "|";
    for (auto& n : nss) id += n + ",";
    id += "|" + SelectorCanon(t.selector);
    auto it = ids.find(id);
    if (it != ids.end()) return it->second;
    const int g = cp.G++;
    ids[id] = g;
    cp.tg_live.push_back(1);
    g_shape.push_back(-1);
    g_spec.push_back(nullptr);
    g_sel.push_back(&t.selector);
    g_nss.push_back(nss);
    g_inverse.push_back(inverse ? 1 : 0);
    const string key = t.topology_key ? t.topology_key : "";
    int k = -1, row = -1;
    if (key == kHostname) {
      row = cp.GH++;
    } else {  // a dictionary key: counts per value ordinal, registered domains = every known value (no taint policy)
      k = d.key(key);
      if (k < 0) return fail(KP_E_INVAL, "topology key %s missing from the dictionary", key.c_str()), -1;
      if (d.dd.nval[k] > 64) return fail(KP_E_UNSUPPORTED, "topology key %s has > 64 values", key.c_str()), -1;
      if (cp.tkey_slot[k] < 0) {
        cp.tkey_slot[k] = cp.TK++;
        cp.tk_keys.push_back(k);
      }
    }
    cp.tg_key.push_back(k);
    cp.tg_row.push_back(row);
    cp.tg_maxskew.push_back(aff ? -1 : 0);
    cp.tg_mindom.push_back(0);
    cp.tg_term_base.push_back((int32_t)cp.tg_terms.size());
    cp.tg_aff.push_back(0);
    cp.tg_nterm.push_back(0);
    cp.tg_filt_tol.push_back(~0ull);
    uint64_t reg = 0;
    if (cp.track_nodes) {
      cp.tg_reg_static.push_back(0);
      cp.tg_hrec_total.push_back(0);
      cp.tg_inv_total.push_back(0);
      cp.tg_spread.push_back(0);
      cp.tg_unreg.emplace_back();
    }
    if (k >= 0) {
      const vector<uint64_t>& dm = domains_of(k);
      for (int b = 0; b < 64; b++)
        if (dm[b]) reg |= 1ull << b;
      if (cp.track_nodes) cp.tg_reg_static[g] = reg;
      const vector<int>& ords = node_ords(k);
      for (uint32_t ni = 0; ni < in->n_existing; ni++) {
        if (ords[ni] >= 0) {
          reg |= 1ull << ords[ni];
          if (cp.track_nodes) cp.node_reg[ni].push_back(g * 64 + ords[ni]);
        }
      }
    }
    cp.tg_reg.push_back(reg);
    for (int b = 0; b < 64; b++) cp.tg_cnt.push_back(0);
    if (row >= 0) cp.hcnt0.resize((size_t)cp.GH * std::max(E, 1), 0);
    if (!inverse) {  // (the sets of every namespace the term selects, in set order)
      vector<int> sets;
      for (const string& n : nss) {
        const vector<int>& v = sets_for(t.selector, n);
        sets.insert(sets.end(), v.begin(), v.end());
      }
      std::sort(sets.begin(), sets.end());
      for (int bi : sets)
        if (SelectorMatches(t.selector, bsets[bi].labels))
          for (const uint32_t ni : bsets[bi].nodes) record_bound(g, ni);
    }
    return g;
  };
  for (uint32_t p = 0; p < in->n_pods; p++) {  // NewTopology: Update(pod) in pod order
    const uint32_t s = in->pods[p].shape;
    if (seen[s]) continue;
    seen[s] = 1;
    const kp_pod_shape& sh = in->shapes[s];
    for (uint32_t j = 0; j < sh.n_topology_spread; j++) {
      const int g = group_of(s, (int)j, 0, true);
      if (g < 0) return KP_E_UNSUPPORTED;
      sgroup[s].push_back(g);
    }
    for (uint32_t a = 0; a < PodTermCount(sh); a++) {
      bool aff = false;
      const kp_pod_affinity_term& t = *PodTermAt(sh, (int)a, &aff);
      const int g = anti_group(t, nss_of(t, sh.namespace_), false, aff);
      if (g < 0) return KP_E_UNSUPPORTED;
      sgroup[s].push_back(g);
    }
  }
  pt.lap("  topo: NewTopology");
  vector<int> inverse_groups;  // updateInverseAffinities: after the batch's groups
  for (uint32_t b = 0; b < in->n_bound_pods; b++) {
    const kp_bound_pod& bp = in->bound_pods[b];
    for (uint32_t j = 0; j < bp.n_anti_affinity; j++) {
      const kp_pod_affinity_term& t = bp.anti_affinity[j];
      const int g = anti_group(t, nss_of(t, bp.namespace_), true);
      if (g < 0) return KP_E_UNSUPPORTED;
      if (std::find(inverse_groups.begin(), inverse_groups.end(), g) == inverse_groups.end()) inverse_groups.push_back(g);
      record_bound(g, bp.node);
      if (cp.track_nodes) {
        cp.node_inv[bp.node].push_back(g);
        cp.tg_inv_total[g]++;
      }
    }
  }
  // every other group a shape-level owns, before the recording lists are built: the groups of shapes without pods,
  // and the spread groups of relaxed levels (a relaxation makes them exist; records must reach them from then on)
  for (uint32_t s = 0; s < in->n_shapes; s++) {
    const kp_pod_shape& sh = in->shapes[s];
    const uint32_t n_terms = sh.n_topology_spread + PodTermCount(sh);
    if (sgroup[s].empty() && n_terms) {  // shape without pods: no groups were created for it
      for (uint32_t j = 0; j < sh.n_topology_spread; j++) {
        const int g = group_of(s, (int)j, 0, false);
        if (g < 0) return KP_E_UNSUPPORTED;
        sgroup[s].push_back(g);
      }
      for (uint32_t a = 0; a < PodTermCount(sh); a++) {
        bool aff = false;
        const kp_pod_affinity_term& t = *PodTermAt(sh, (int)a, &aff);
        const int g = anti_group(t, nss_of(t, sh.namespace_), false, aff);
        if (g < 0) return KP_E_UNSUPPORTED;
        sgroup[s].push_back(g);
      }
    }
    for (int l = 1; l < cp.shape_nlevels[s]; l++)
      for (int j : spread_levels[s][l])
        if (j < (int)sh.n_topology_spread && group_of(s, j, l, false) < 0) return KP_E_UNSUPPORTED;
    if (cp.track_nodes)  // sgroup: the level-0 spread groups first, then the pod (anti-)affinity groups
      cp.shape_l0[s].assign(sgroup[s].begin(), sgroup[s].begin() + std::min<size_t>(sgroup[s].size(), sh.n_topology_spread));
  }
  pt.lap("  topo: other groups");
  if (cp.G == 0) return KP_OK;
  if ((size_t)cp.GH * (size_t)(E + in->n_pods) > ((size_t)1 << 31))
    return fail(KP_E_UNSUPPORTED, "%d hostname topologies x %u nodes", cp.GH, E + in->n_pods);
  if (E == 0) cp.hcnt0.clear();
  // recording groups per shape (TopologyGroup.selects: namespace + selector on the pod's labels); shapes are
  // indexed by (namespace, label) so a matchLabels selector only tests the shapes carrying its first label
  vector<std::map<string, string>> shape_labels(in->n_shapes);
  std::map<string, vector<uint32_t>> by_label, by_ns;
  for (uint32_t s = 0; s < in->n_shapes; s++) {
    const kp_pod_shape& sh = in->shapes[s];
    shape_labels[s] = LabelMap(sh.labels, sh.n_labels);
    const string ns = sh.namespace_ ? sh.namespace_ : "";
    by_ns[ns].push_back(s);
    for (auto& kv : shape_labels[s]) by_label[ns + '\x01' + kv.first + '\x01' + kv.second].push_back(s);
  }
  vector<vector<int>> recs(in->n_shapes);
  static const vector<uint32_t> kNone;
  vector<vector<int>> inv_owned(in->n_shapes);  // inverse groups that select each shape
  for (int g = 0; g < cp.G; g++) {
    const kp_label_selector& sel = *g_sel[g];
    if (sel.is_nil) continue;
    for (const string& ns : g_nss[g]) {
      const vector<uint32_t>* cands;
      if (sel.n_match_labels) {
        auto it = by_label.find(ns + '\x01' + (sel.match_labels[0].key ? sel.match_labels[0].key : "") + '\x01' +
                                (sel.match_labels[0].value ? sel.match_labels[0].value : ""));
        cands = it == by_label.end() ? &kNone : &it->second;
      } else {
        auto it = by_ns.find(ns);
        cands = it == by_ns.end() ? &kNone : &it->second;
      }
      for (uint32_t s : *cands)
        if (SelectorMatches(sel, shape_labels[s])) (g_inverse[g] ? inv_owned[s] : recs[s]).push_back(g);
    }
  }
  for (uint32_t s = 0; s < in->n_shapes; s++) {
    // each group once: the device Record gives every group of a pod its own lane
    std::sort(recs[s].begin(), recs[s].end());
    recs[s].erase(std::unique(recs[s].begin(), recs[s].end()), recs[s].end());
    cp.shape_rec_base[s] = (int32_t)cp.rec_list.size();
    cp.shape_rec_n[s] = (int32_t)recs[s].size();
    cp.rec_list.insert(cp.rec_list.end(), recs[s].begin(), recs[s].end());
  }
  pt.lap("  topo: record lists");
  // owned groups per shape-level: (group, self-selecting, podDomains mask over the key's value ordinals)
  for (uint32_t s = 0; s < in->n_shapes; s++) {
    const kp_pod_shape& sh = in->shapes[s];
    const uint32_t n_terms = sh.n_topology_spread + PodTermCount(sh);
    if (!n_terms && inv_owned[s].empty()) continue;
    const std::map<string, string> lm = LabelMap(sh.labels, sh.n_labels);
    for (int l = 0; l < cp.shape_nlevels[s]; l++) {
      const int sl = cp.shape_level_base[s] + l;
      vector<int> sp = spread_levels[s][l];  // term ids, then the inverse groups selecting the shape (as -1 - g)
      for (int g : inv_owned[s]) sp.push_back(-1 - g);
      if (sp.size() > 8) return fail(KP_E_UNSUPPORTED, "> 8 topology constraints (spread / anti-affinity) on one pod");
      cp.sl_own_base[sl] = (int32_t)cp.own_group.size();
      cp.sl_own_n[sl] = (int32_t)sp.size();
      const KReqs strict = Compile(d, strict_levels[s][l]);
      for (int j : sp) {
        // spreads: the level's group (a relaxed required term makes another one, live once a pod relaxes to it)
        const int g = j < 0 ? -1 - j : j < (int)sh.n_topology_spread ? group_of(s, j, l, false) : sgroup[s][j];
        if (g < 0) return KP_E_UNSUPPORTED;
        cp.own_group.push_back(g);
        // self: the spread's / affinity term's selector matches the pod (spread: count + 1; affinity: it may
        // bootstrap); anti-affinity accepts count == 0 only
        bool aff = false;
        const kp_pod_affinity_term* pt = j >= (int)sh.n_topology_spread ? PodTermAt(sh, j - (int)sh.n_topology_spread, &aff) : nullptr;
        cp.own_self.push_back(j >= 0 && j < (int)sh.n_topology_spread ? (SelectorMatches(sh.topology_spread[j].selector, lm) ? 1 : 0)
                              : (pt && aff && nss_of(*pt, sh.namespace_).count(sh.namespace_ ? sh.namespace_ : "") &&
                                 SelectorMatches(pt->selector, lm)) ? 1 : 0);
        const int k = cp.tg_key[g];
        uint64_t pd = 0;
        if (k >= 0) {
          for (int b = 0; b < d.dd.nval[k]; b++)
            if (Has(d, strict, k, k * 64 + b)) pd |= 1ull << b;
          cp.sl_topo_keys[sl] |= 1ull << k;
        }
        cp.own_pd.push_back(pd);
        const int32_t rec[8] = {g, cp.own_self.back(), k, cp.tg_maxskew[g], cp.tg_mindom[g], cp.tg_row[g],
                                k >= 0 ? cp.tkey_slot[k] : -1, 0};
        cp.own_rec.insert(cp.own_rec.end(), rec, rec + 8);
      }
    }
  }
  pt.lap("  topo: owned");
  // shape-levels the fast lane may take: at most 4 owned groups, every owned and every recorded group a spread
  // (maxSkew > 0) and no recorded group with node-filter terms (the fast lane's Record reads the NodeClaim's value
  // codes); pods of other levels (affinity, anti-affinity, filtered groups) stay on the full path
  for (uint32_t s = 0; s < in->n_shapes; s++) {
    bool rec_ok = true;
    for (int i = 0; i < cp.shape_rec_n[s]; i++) {
      const int g = cp.rec_list[cp.shape_rec_base[s] + i];
      rec_ok = rec_ok && cp.tg_maxskew[g] > 0 && !cp.tg_aff[g];
    }
    for (int l = 0; l < cp.shape_nlevels[s]; l++) {
      const int sl = cp.shape_level_base[s] + l;
      bool ok = rec_ok && cp.sl_own_n[sl] <= 4;
      for (int j = 0; j < cp.sl_own_n[sl] && ok; j++) ok = cp.tg_maxskew[cp.own_group[cp.sl_own_base[sl] + j]] > 0;
      cp.sl_fast_topo[sl] = ok ? 1 : 0;
    }
  }
  cp.rec_aux.resize(cp.rec_list.size());
  for (size_t i = 0; i < cp.rec_list.size(); i++) {
    const int g = cp.rec_list[i];
    cp.rec_aux[i] = cp.tg_row[g] >= 0 ? cp.tg_row[g] : -1 - cp.tkey_slot[cp.tg_key[g]];
  }
  // existing nodes: value ordinal of each topology key (0xFF: no label)
  cp.ex_tcode.assign((size_t)std::max(cp.TK, 1) * std::max(E, 1), 0xFF);
  for (int k = 0; k < KP_MAX_KEYS; k++) {
    if (cp.tkey_slot[k] < 0) continue;
    const vector<int>& ords = node_ords(k);
    for (int e = 0; e < E; e++)
      if (ords[cp.ex_input[e]] >= 0) cp.ex_tcode[(size_t)cp.tkey_slot[k] * E + e] = (uint8_t)ords[cp.ex_input[e]];
  }
  if (cp.tg_terms.empty()) {
    KReqs z;
    memset(&z, 0, sizeof z);
    cp.tg_terms.push_back(z);
    cp.tg_terms_negop.push_back(0);
  }
  return KP_OK;
}

// An existing node's labels as requirements (NewExistingNode: each label `In {value}`, in input order), without the
// per-label strings of a RawReqs: views into the caller's kp_labels (keys normalized), plus the hostname requirement's
// value when some pod names kubernetes.io/hostname. Thousands of nodes × ~20 labels made the RawReqs form the largest
// part of a Solve's host compile.
struct NodeLabels {
  vector<std::pair<std::string_view, std::string_view>> kv;  // normalized key, value (the hostname label dropped)
  string host;                                               // the hostname requirement's value (has_host)
  bool has_host = false;
};
// karpv1.NormalizedLabels (Normalize) without a string copy: the alias's target or the key itself
std::string_view NormalizeSV(const char* k) {
  static const std::pair<const char*, string> aliases[] = {
      {"failure-domain.beta.kubernetes.io/zone", "topology.kubernetes.io/zone"},
      {"beta.kubernetes.io/arch", "kubernetes.io/arch"},
      {"beta.kubernetes.io/os", "kubernetes.io/os"},
      {"beta.kubernetes.io/instance-type", "node.kubernetes.io/instance-type"},
      {"failure-domain.beta.kubernetes.io/region", "topology.kubernetes.io/region"},
      {"topology.ebs.csi.aws.com/zone", "topology.kubernetes.io/zone"},
  };
  for (auto& a : aliases)
    if (strcmp(k, a.first) == 0) return a.second;
  return k;
}
// Dictionary ids of label keys and values by view, memoised per compile (the Dict's maps take strings)
struct LabelIds {
  const Dict& d;
  std::unordered_map<std::string_view, int> key;
  std::unordered_map<int, std::unordered_map<std::string_view, int>> val;
  explicit LabelIds(const Dict& dd) : d(dd) {}
  int k(std::string_view s) {
    auto it = key.find(s);
    if (it != key.end()) return it->second;
    return key.emplace(s, d.key(string(s))).first->second;
  }
  int b(int kk, std::string_view v) {
    auto& m = val[kk];
    auto it = m.find(v);
    if (it != m.end()) return it->second;
    return m.emplace(v, d.bit(kk, string(v))).first->second;
  }
};

// Compile(d, labels as RawReqs) for a NodeLabels: each label Single(In {value}) Added in order, then the hostname one
KReqs CompileNode(const Dict& d, const NodeLabels& nl, LabelIds& ids) {
  KReqs q, s;
  memset(&q, 0, sizeof q);
  memset(&s, 0, sizeof s);
  auto add = [&](int k, int bit) {  // Single(d, {key k, In, {value bit}}) then HostAdd, s back to zero after
    s.present = 1ull << k;
    s.vals[bit / 64] |= 1ull << (bit % 64);
    HostAdd(d, q, s);
    s.vals[bit / 64] = 0;
    s.present = 0;
  };
  for (auto& kv : nl.kv) {
    const int k = ids.k(kv.first);
    add(k, ids.b(k, kv.second));
  }
  if (nl.has_host) {
    const int k = d.key(kHostname);
    add(k, d.bit(k, nl.host));
  }
  return q;
}

// Inputs of one Solve that are not part of its SolveBase: the pods' relaxation levels, node labels, spread keys.
struct SolveRaw {
  vector<RawReqs> np_reqs;                        // per input NodePool (requirements + labels + nodepool key)
  vector<vector<TaintT>> np_taints;
  vector<vector<RawReqs>> levels, strict_levels;  // per shape: NewPodRequirements after successive Relax
  vector<vector<vector<int>>> spread_levels;      // per level: topology terms (j < n_topology_spread: spread j;
                                                  // n_topology_spread + a: anti-affinity term a of AntiTerms)
  vector<vector<vector<RawReqs>>> filter_levels;  // per level: MakeTopologyNodeFilter's terms (nodeSelector + each
                                                  // remaining required term; the nodeSelector alone when none)
  std::set<string> topo_keys;                     // non-hostname spread keys (need a dictionary id)
  bool tolerate_pns = false;                      // some NodePool taint has effect PreferNoSchedule (NewScheduler)
  vector<int> pns_level;                          // per shape: the level toleratePreferNoScheduleTaints adds, or -1
  vector<NodeLabels> ex_labels;                   // per input existing node (hostname: see HostnameValue)
  bool hostname = false;                          // some pod requirement names kubernetes.io/hostname
};

// kubernetes.io/hostname as a requirement key. Upstream gives every NodeClaim `hostname In {a unique placeholder}`
// (NewNodeClaim) and every existing node `hostname In {its hostname}` (NewExistingNode: the label, else the node
// name). A pod's hostname requirement only ever compares those values with the ones it names, so the dictionary
// holds the named values plus two stand-ins: kHostOther for every hostname no pod names, kHostPlaceholder for the
// NodeClaims' (templates carry it; the decoded NodeClaim requirements drop it, as FinalizeScheduling does).
const char* kHostOther = "\x01other-hostname";
const char* kHostPlaceholder = "\x01hostname-placeholder";

void HostnameNames(const kp_requirements& r, bool* used, std::set<string>* named) {
  for (uint32_t i = 0; i < r.n; i++) {
    const kp_requirement& x = r.items[i];
    if (!x.key || string(x.key) != kHostname) continue;
    *used = true;
    for (uint32_t j = 0; j < x.n_values; j++) named->insert(x.values[j] ? x.values[j] : "");
  }
}

void KeyReqs(string& o, const RawReqs& rs) {
  for (auto& r : rs) {
    o += r.key + '\x01' + std::to_string(r.op) + '\x01' + std::to_string(r.minv);
    for (auto& v : r.values) o += '\x02' + v;
    o += '\x03';
  }
  o += '\x04';
}

// The catalogues' seqnums as they are now, and that part of a cache fingerprint.
vector<uint64_t> SeqnumsOf(const vector<const kp_catalog*>& cats) {
  vector<uint64_t> v;
  for (auto* c : cats) v.push_back(c->seqnum);
  return v;
}
// the ctx's cached bases that compiled catalogue c (kp_catalog_destroy)
void DropBasesOf(kp_ctx* ctx, const kp_catalog* c) {
  auto& bases = ctx->bases;
  bases.erase(std::remove_if(bases.begin(), bases.end(),
                             [&](const std::shared_ptr<SolveBase>& b) {
                               return std::find(b->catalogs.begin(), b->catalogs.end(), c) != b->catalogs.end();
                             }),
              bases.end());
}
// KP_OK while every catalogue a base (or plan) compiled is alive, else the error a run or refresh returns.
int32_t CatalogsAlive(const vector<std::shared_ptr<bool>>& alive) {
  for (auto& a : alive)
    if (!*a) return fail(KP_E_INVAL, "a catalogue this plan was prepared on was destroyed (kp_catalog_destroy)");
  return KP_OK;
}
string SeqKey(const vector<uint64_t>& seqs) {
  string k = "#";
  for (uint64_t q : seqs) k += std::to_string(q) + ";";
  return k;
}
// Fingerprint of everything a SolveBase depends on but the seqnums: catalogue identities, the NodePools.
string BaseIdent(const kp_solve_in* in, const SolveRaw& raw) {
  string k;
  for (uint32_t c = 0; c < in->n_catalogs; c++) {
    const kp_catalog* cat = in->catalogs[c];
    k += std::to_string(cat->uid) + ":" + std::to_string(cat->types.size()) + ";";
  }
  for (uint32_t i = 0; i < in->n_nodepools; i++) {
    const kp_nodepool& np = in->nodepools[i];
    k += string(np.name ? np.name : "") + '\x05' + std::to_string(np.weight) + '\x05' + std::to_string(np.catalog);
    KeyReqs(k, raw.np_reqs[i]);
    for (auto& t : raw.np_taints[i]) k += t.key + '\x01' + t.value + '\x01' + std::to_string(t.effect) + '\x02';
    for (int r = 0; r < KP_NRES; r++)
      if ((np.daemon_requests.present >> r) & 1) k += std::to_string(r) + "=" + std::to_string(np.daemon_requests.milli[r]) + ",";
    k += '\x06';
  }
  return k;
}

// Every key / value / bound slot the requirement set needs is already in the dictionary.
bool Covers(const Dict& d, const RawReqs& rs) {
  for (auto& r : rs) {
    const int k = d.key(r.key);
    if (k < 0) return false;
    if ((r.op == KP_OP_GT || r.op == KP_OP_LT || r.minv >= 0) && k >= d.dd.KB) return false;
    if (r.op == KP_OP_IN || r.op == KP_OP_NOT_IN)
      for (auto& v : r.values)
        if (d.bit(k, v) < 0) return false;
  }
  return true;
}
bool BaseCovers(const SolveBase& b, const SolveRaw& raw) {
  for (auto& lv : raw.levels)
    for (auto& r : lv)
      if (!Covers(b.d, r)) return false;
  {  // the node labels: every key and value in the dictionary (In requirements: no bound slots needed)
    LabelIds ids(b.d);
    const int kh = raw.hostname ? b.d.key(kHostname) : -1;
    for (auto& nl : raw.ex_labels) {
      for (auto& kv : nl.kv) {
        const int k = ids.k(kv.first);
        if (k < 0 || ids.b(k, kv.second) < 0) return false;
      }
      if (nl.has_host && (kh < 0 || b.d.bit(kh, nl.host) < 0)) return false;
    }
  }
  for (auto& k : raw.topo_keys)
    if (b.d.key(k) < 0) return false;
  return true;
}

// Parse the NodePools, shapes (relaxation levels) and node labels of a Solve.
int32_t ParseSolve(const kp_solve_in* in, SolveRaw& raw) {
  if (in->n_catalogs == 0 || !in->catalogs) return fail(KP_E_INVAL, "no catalogues");
  for (uint32_t c = 0; c < in->n_catalogs; c++)
    if (!in->catalogs[c]) return fail(KP_E_INVAL, "null catalogue");
  std::set<string> host_named;  // hostname values the pods' requirements name
  for (uint32_t s = 0; s < in->n_shapes; s++) {
    const kp_pod_shape& sh = in->shapes[s];
    for (uint32_t j = 0; j < sh.n_node_selector; j++)
      if (sh.node_selector[j].key && string(sh.node_selector[j].key) == kHostname) {
        raw.hostname = true;
        host_named.insert(sh.node_selector[j].value ? sh.node_selector[j].value : "");
      }
    for (uint32_t j = 0; j < sh.n_required_terms; j++) HostnameNames(sh.required_terms[j], &raw.hostname, &host_named);
    for (uint32_t j = 0; j < sh.n_preferred_terms; j++) HostnameNames(sh.preferred_terms[j].preference, &raw.hostname, &host_named);
    HostnameNames(kp_requirements{sh.volume_requirements, sh.n_volume_requirements, 0}, &raw.hostname, &host_named);
  }
  raw.np_reqs.resize(in->n_nodepools);
  raw.np_taints.resize(in->n_nodepools);
  for (uint32_t i = 0; i < in->n_nodepools; i++) {
    const kp_nodepool& np = in->nodepools[i];
    if (np.catalog >= in->n_catalogs) return fail(KP_E_INVAL, "nodepool %u: catalogue %u", i, np.catalog);
    RawReqs r = ParseReqs(np.requirements);
    RawReqs l = LabelReqs(np.labels, np.n_labels, false);
    r.insert(r.end(), l.begin(), l.end());
    r.push_back({kNodePool, KP_OP_IN, {np.name ? np.name : ""}, -1});
    for (auto& x : r)
      if (x.key == kHostname) return fail(KP_E_UNSUPPORTED, "hostname requirement on nodepool");
    if (raw.hostname) r.push_back({kHostname, KP_OP_IN, {kHostPlaceholder}, -1});  // NewNodeClaim's placeholder
    raw.np_reqs[i] = std::move(r);
    for (uint32_t j = 0; j < np.n_taints; j++) {
      raw.np_taints[i].push_back({np.taints[j].key ? np.taints[j].key : "", np.taints[j].value ? np.taints[j].value : "",
                                  np.taints[j].effect});
      // upstream NewScheduler: Preferences{ToleratePreferNoSchedule} when any NodePool template taint has that effect
      if (np.taints[j].effect == KP_EFFECT_PREFER_NO_SCHEDULE) raw.tolerate_pns = true;
    }
  }
  raw.pns_level.assign(in->n_shapes, -1);
  raw.levels.assign(in->n_shapes, {});
  raw.strict_levels.assign(in->n_shapes, {});
  raw.spread_levels.assign(in->n_shapes, {});
  raw.filter_levels.assign(in->n_shapes, {});
  for (uint32_t s = 0; s < in->n_shapes; s++) {
    const kp_pod_shape& sh = in->shapes[s];
    for (uint32_t j = 0; j < sh.n_topology_spread; j++) {
      const kp_topology_spread& t = sh.topology_spread[j];
      const string key = t.topology_key ? t.topology_key : "";
      if (t.max_skew < 1 || t.max_skew > 250) return fail(KP_E_UNSUPPORTED, "topology spread maxSkew %d", t.max_skew);
      if (key != kHostname) raw.topo_keys.insert(key);  // the key gets a dictionary id even if no value names it
    }
    if (sh.n_preferred_terms > 12) return fail(KP_E_UNSUPPORTED, "> 12 preferred terms");
    if (sh.n_preferred_anti_affinity > 12 || sh.n_preferred_affinity > 12)
      return fail(KP_E_UNSUPPORTED, "> 12 preferred pod (anti-)affinity terms");
    for (uint32_t j = 0; j < PodTermCount(sh); j++) {
      const kp_pod_affinity_term& t = *PodTermAt(sh, (int)j);
      const int32_t rc = CheckAntiTerm(t, "shape", s);
      if (rc) return rc;
      if (t.topology_key != string(kHostname)) raw.topo_keys.insert(t.topology_key);
    }
    RawReqs ns = LabelReqs(sh.node_selector, sh.n_node_selector, false);
    vector<RawReqs> req;
    for (uint32_t j = 0; j < sh.n_required_terms; j++) req.push_back(ParseReqs(sh.required_terms[j]));
    if (sh.n_volume_requirements) {  // VolumeTopology.Inject: appended to every required term (one created if none)
      RawReqs v = ParseReqs(kp_requirements{sh.volume_requirements, sh.n_volume_requirements, 0});
      if (req.empty()) req.push_back(v);
      else
        for (auto& t : req) t.insert(t.end(), v.begin(), v.end());
    }
    vector<std::pair<int, RawReqs>> pref;
    for (uint32_t j = 0; j < sh.n_preferred_terms; j++)
      pref.push_back({sh.preferred_terms[j].weight, ParseReqs(sh.preferred_terms[j].preference)});
    auto byw = [](const std::pair<int, RawReqs>& a, const std::pair<int, RawReqs>& b) { return a.first > b.first; };
    std::stable_sort(pref.begin(), pref.end(), byw);  // sort.Slice on <= 12 = insertion sort (stable)
    vector<int> spreads;
    for (uint32_t j = 0; j < sh.n_topology_spread; j++) spreads.push_back((int)j);
    // preferred anti-affinity terms: removePreferredPodAntiAffinityTerm drops the heaviest first (sort.Slice by
    // weight desc on <= 12 terms: insertion sort, stable)
    vector<int> apref, fpref;  // removePreferredPodAffinityTerm, then removePreferredPodAntiAffinityTerm
    for (uint32_t a = 0; a < sh.n_preferred_anti_affinity; a++) apref.push_back((int)a);
    std::stable_sort(apref.begin(), apref.end(), [&](int x, int y) {
      return sh.preferred_anti_affinity[x].weight > sh.preferred_anti_affinity[y].weight;
    });
    for (uint32_t a = 0; a < sh.n_preferred_affinity; a++) fpref.push_back((int)a);
    std::stable_sort(fpref.begin(), fpref.end(), [&](int x, int y) {
      return sh.preferred_affinity[x].weight > sh.preferred_affinity[y].weight;
    });
    const int nS = (int)sh.n_topology_spread, nRA = (int)sh.n_required_anti_affinity,
              nPA = (int)sh.n_preferred_anti_affinity, nRF = (int)sh.n_required_affinity;
    for (;;) {
      RawReqs r = ns;
      if (!pref.empty()) r.insert(r.end(), pref[0].second.begin(), pref[0].second.end());
      if (!req.empty()) r.insert(r.end(), req[0].begin(), req[0].end());
      raw.levels[s].push_back(std::move(r));
      RawReqs strict = ns;  // NewStrictPodRequirements: without the preferred term
      if (!req.empty()) strict.insert(strict.end(), req[0].begin(), req[0].end());
      raw.strict_levels[s].push_back(std::move(strict));
      vector<RawReqs> filt;
      for (auto& t : req) {
        filt.push_back(ns);
        filt.back().insert(filt.back().end(), t.begin(), t.end());
      }
      if (filt.empty()) filt.push_back(ns);
      raw.filter_levels[s].push_back(std::move(filt));
      vector<int> terms = spreads;  // spreads, required anti-affinity terms, remaining preferred ones, affinity alike
      for (int a = 0; a < nRA; a++) terms.push_back(nS + a);
      for (int a : apref) terms.push_back(nS + nRA + a);
      for (int a = 0; a < nRF; a++) terms.push_back(nS + nRA + nPA + a);
      for (int a : fpref) terms.push_back(nS + nRA + nPA + nRF + a);
      raw.spread_levels[s].push_back(terms);
      if (req.size() > 1) {
        req.erase(req.begin());
      } else if (!fpref.empty()) {
        fpref.erase(fpref.begin());
      } else if (!apref.empty()) {
        apref.erase(apref.begin());
      } else if (!pref.empty()) {
        pref.erase(pref.begin());
      } else {  // removeTopologySpreadScheduleAnyway: first ScheduleAnyway constraint, swapped with the last
        size_t i = 0;
        while (i < spreads.size() && sh.topology_spread[spreads[i]].when_unsatisfiable != KP_SCHEDULE_ANYWAY) i++;
        if (i == spreads.size()) break;
        spreads[i] = spreads.back();
        spreads.pop_back();
      }
    }
    // toleratePreferNoScheduleTaints (the last relaxation, only with Preferences.ToleratePreferNoSchedule): appends
    // {Operator: Exists, Effect: PreferNoSchedule} unless a toleration already equals it (corev1 MatchToleration:
    // key, operator, value and effect equal), so the pod's requirements and terms stay those of the last level
    if (raw.tolerate_pns && !HasPnsToleration(sh)) {
      raw.pns_level[s] = (int)raw.levels[s].size();
      raw.levels[s].push_back(raw.levels[s].back());
      raw.strict_levels[s].push_back(raw.strict_levels[s].back());
      raw.filter_levels[s].push_back(raw.filter_levels[s].back());
      raw.spread_levels[s].push_back(raw.spread_levels[s].back());
    }
  }
  PhaseTimer pt;
  for (uint32_t b = 0; b < in->n_bound_pods; b++)  // inverse anti-affinity keys need a dictionary id too
    for (uint32_t j = 0; j < in->bound_pods[b].n_anti_affinity; j++) {
      const char* k = in->bound_pods[b].anti_affinity[j].topology_key;
      if (k && k[0] && string(k) != kHostname) raw.topo_keys.insert(k);
    }
  raw.ex_labels.resize(in->n_existing);
  for (uint32_t i = 0; i < in->n_existing; i++) {
    const kp_existing_node& e = in->existing[i];
    NodeLabels& nl = raw.ex_labels[i];
    nl.kv.reserve(e.n_labels);
    for (uint32_t j = 0; j < e.n_labels; j++) {
      const std::string_view k = NormalizeSV(e.labels[j].key ? e.labels[j].key : "");
      if (k == kHostname) continue;  // (NewExistingNode's hostname requirement, below)
      nl.kv.emplace_back(k, e.labels[j].value ? e.labels[j].value : "");
    }
    if (raw.hostname) {  // NewExistingNode: hostname In {HostName()} (the label, else the node name)
      string host;
      for (uint32_t j = 0; j < e.n_labels; j++)
        if (e.labels[j].key && string(e.labels[j].key) == kHostname && e.labels[j].value) host = e.labels[j].value;
      if (host.empty()) host = e.name ? e.name : "";
      nl.host = host_named.count(host) ? host : string(kHostOther);
      nl.has_host = true;
    }
  }
  pt.lap(" parse: node labels");
  return KP_OK;
}

// Dictionary (catalogues, NodePools + the values `raw` names), catalogue SoA, offering classes, templates.
// The NodeClaimTemplates' InstanceTypeOptions (upstream NewScheduler's pre-filter: the pool's requirements, empty
// requests, a compatible available offering, minValues); pools that keep no type are skipped. Depends on the
// offerings' availability, so an ICE update re-runs it (RefreshOfferings).
void BuildTemplates(const SolveBase& b, vector<int>& tnp, vector<uint64_t>& tX) {
  const Dict& d = b.d;
  const int TW = b.TW;
  tnp.clear();
  tX.clear();
  for (int i : b.np_order) {
    const KReqs& q = b.np_q[i];
    const HostCat& hc = b.cats[b.np_catalog[i]];
    vector<uint64_t> X(TW, 0);
    for (int t = 0; t < hc.T; t++) X[t / 64] |= 1ull << (t % 64);
    int64_t zero[KP_NRES] = {0};
    HostFilterTypes(d, hc, q, TW, zero, X);
    const uint64_t cls = HostAllowedClasses(d, q, b.classes);
    vector<uint64_t> offer(TW, 0);
    for (int c = 0; c < b.C; c++)
      if ((cls >> c) & 1)
        for (int w = 0; w < TW; w++) offer[w] |= hc.offer_avail[(size_t)c * TW + w];
    bool any = false;
    for (int w = 0; w < TW; w++) any |= (X[w] &= offer[w]) != 0;
    if (any && q.hmin) {
      vector<int> ts;
      for (int t = 0; t < hc.T; t++)
        if ((X[t / 64] >> (t % 64)) & 1) ts.push_back(t);
      if (!HostMinValuesOK(d, hc, q, ts)) any = false;
    }
    if (!any) continue;  // "skipping, nodepool requirements filtered out all instance types"
    tnp.push_back(i);
    tX.insert(tX.end(), X.begin(), X.end());
  }
}

int32_t BuildBase(const kp_solve_in* in, const SolveRaw& raw, SolveBase& b) {
  auto t0 = std::chrono::steady_clock::now();
  vector<const kp_catalog*> cats(in->catalogs, in->catalogs + in->n_catalogs);
  DictBuilder db;
  int maxT = 1;
  for (auto* c : cats) {
    maxT = std::max(maxT, (int)c->types.size());
    for (auto& t : c->types) {
      db.addReqs(t.reqs);
      for (auto& o : t.offs) {
        db.addLabel(kCapType, o.ct);
        if (o.has_zone) db.addLabel(kZone, o.zone);
        if (o.has_zid) db.addLabel(kZoneID, o.zid);
        if (o.has_rid) db.addLabel(kResID, o.rid);
        if (o.has_rt) db.addLabel(kResType, o.rt);
      }
    }
  }
  db.bounded[kResID];
  db.bounded[kResType];
  for (auto& r : raw.np_reqs) db.addReqs(r);
  for (auto& lv : raw.levels)
    for (auto& r : lv) db.addReqs(r);
  for (auto& k : raw.topo_keys) db.bounded[k];
  for (auto& nl : raw.ex_labels) {
    for (auto& kv : nl.kv) db.addLabel(string(kv.first), string(kv.second));
    if (nl.has_host) db.addLabel(kHostname, nl.host);
  }
  int32_t rc = db.build(b.d);
  if (rc) return rc;
  const Dict& d = b.d;
  const int TW = (maxT + 63) / 64;
  b.TW = TW;
  b.d.dd.TW = TW;
  b.d.dd.T = maxT;
  // offering classes
  map<ClassKey, int> classes;
  for (auto* c : cats)
    for (auto& t : c->types)
      for (auto& o : t.offs) {
        const ClassKey ck = ClassOf(d, o);
        if (!classes.count(ck)) {
          int id = (int)classes.size();
          classes[ck] = id;
        }
      }
  if (classes.size() > KP_MAX_CLASSES) return fail(KP_E_UNSUPPORTED, "%zu offering classes", classes.size());
  b.C = (int)classes.size();
  b.classes.resize(b.C);
  for (auto& kv : classes) b.classes[kv.second] = ClassOfKey(kv.first);
  b.d.dd.C = b.C;
  b.cats.resize(cats.size());
  uint64_t catalog_keys = 0, multi = 0;
  for (size_t i = 0; i < cats.size(); i++) {
    rc = CompileCatalog(d, cats[i]->types, TW, classes, b.cats[i]);
    if (rc) return rc;
    multi |= b.cats[i].multi_valued;
    for (int k = 0; k < d.dd.K; k++) {
      // NOKEY covers every type only if no type has the key (padding bits masked)
      bool all = true;
      for (int t = 0; t < b.cats[i].T && all; t++)
        if (!((b.cats[i].NOKEY[(size_t)k * TW + t / 64] >> (t % 64)) & 1)) all = false;
      if (!all) catalog_keys |= 1ull << k;
    }
  }
  b.d.dd.catalog_keys = catalog_keys;
  b.d.dd.single_valued = catalog_keys & ~multi;
  for (auto& hc : b.cats) hc.multi_valued = multi;
  // the NodePools' taint sets (ids 0.. in input order; a Solve's nodes add theirs after these)
  map<vector<TaintT>, int> tsets;
  b.np_taintset.resize(in->n_nodepools);
  for (uint32_t i = 0; i < in->n_nodepools; i++) {
    vector<TaintT> v = raw.np_taints[i];
    std::sort(v.begin(), v.end());
    auto it = tsets.find(v);
    if (it == tsets.end()) {
      it = tsets.emplace(v, (int)b.tsets.size()).first;
      b.tsets.push_back(v);
    }
    b.np_taintset[i] = it->second;
  }
  // templates: weight desc, name asc; pre-filter options with empty requests (upstream NewScheduler)
  vector<int> order(in->n_nodepools);
  for (uint32_t i = 0; i < in->n_nodepools; i++) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
    const kp_nodepool &p = in->nodepools[x], &q = in->nodepools[y];
    if (p.weight != q.weight) return p.weight > q.weight;
    return strcmp(p.name ? p.name : "", q.name ? q.name : "") < 0;
  });
  b.np_order = order;
  for (uint32_t i = 0; i < in->n_nodepools; i++) {
    const kp_nodepool& np = in->nodepools[i];
    b.np_q.push_back(Compile(d, raw.np_reqs[i]));
    b.np_catalog.push_back((int32_t)np.catalog);
    for (int r = 0; r < KP_NRES; r++)
      b.np_daemon.push_back((np.daemon_requests.present >> r) & 1 ? np.daemon_requests.milli[r] : 0);
  }
  b.catalogs = cats;
  for (auto* c : cats) b.alive.push_back(c->alive);
  b.seqnums = SeqnumsOf(cats);
  rc = ReservationTables(b);
  if (rc) return rc;
  b.d.dd.res_any = b.res_cls ? 1 : 0;
  BuildTemplates(b, b.tmpl_nodepool, b.tmpl_X);
  for (int i : b.tmpl_nodepool) {
    b.tmpl_reqs.push_back(b.np_q[i]);
    b.tmpl_taintset.push_back(b.np_taintset[i]);
    b.tmpl_catalog.push_back(b.np_catalog[i]);
    b.tmpl_daemon.insert(b.tmpl_daemon.end(), b.np_daemon.begin() + (size_t)i * KP_NRES,
                         b.np_daemon.begin() + (size_t)(i + 1) * KP_NRES);
  }
  b.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return KP_OK;
}

// Per-Solve half on a SolveBase: taint sets, limits, existing nodes, shapes (levels, PVP rows), topology, queue.
// Exact Queue keys from the pods' UIDs (upstream NewQueue's last tie-break compares metadata.uid as strings): each
// pod's rank in the batch sorted by UID, equal UIDs (invalid in a cluster) by batch index. false: a NULL UID.
bool ExactUidKeys(const char* const* uids, uint32_t n, vector<uint64_t>& key) {
  // sorted by the first 8 bytes as a big-endian integer (zero-padded: the string order), strcmp only between equal
  // prefixes; equal strings keep their input order
  struct Ent {
    uint64_t pre;
    uint32_t i;
  };
  vector<Ent> e(n);
  for (uint32_t i = 0; i < n; i++) {
    if (!uids[i]) return false;
    uint64_t p = 0;
    const unsigned char* u = (const unsigned char*)uids[i];
    for (int j = 0; j < 8; j++) {
      p = (p << 8) | u[j];
      if (!u[j]) {  // shorter: the rest stays zero
        p <<= 8 * (7 - j);
        break;
      }
    }
    e[i] = {p, i};
  }
  std::sort(e.begin(), e.end(), [&](const Ent& a, const Ent& b) {
    if (a.pre != b.pre) return a.pre < b.pre;
    const int c = strcmp(uids[a.i], uids[b.i]);
    return c != 0 ? c < 0 : a.i < b.i;
  });
  key.assign(n, 0);
  for (uint32_t r = 0; r < n; r++) key[e[r].i] = r;
  return true;
}

int32_t CompilePerCall(const kp_solve_in* in, const SolveRaw& raw, Compiled& cp) {
  const SolveBase& b = *cp.B;
  const Dict& d = b.d;
  const int TW = b.TW;
  PhaseTimer pt;
  map<vector<TaintT>, int> tsets;
  for (size_t i = 0; i < b.tsets.size(); i++) tsets[b.tsets[i]] = (int)i;
  auto tset = [&](vector<TaintT> v) {
    std::sort(v.begin(), v.end());
    auto it = tsets.find(v);
    if (it != tsets.end()) return it->second;
    int id = (int)tsets.size();
    tsets[v] = id;
    return id;
  };
  for (int np : b.tmpl_nodepool) {
    const kp_nodepool& p = in->nodepools[np];
    for (int r = 0; r < KP_NRES; r++) cp.tmpl_remaining.push_back((p.limits.present >> r) & 1 ? p.limits.milli[r] : 0);
    cp.tmpl_limit_present.push_back(p.limits.present);
  }
  // existing nodes: initialized first, then by name
  vector<int> ex(in->n_existing);
  for (uint32_t i = 0; i < in->n_existing; i++) ex[i] = (int)i;
  std::stable_sort(ex.begin(), ex.end(), [&](int x, int y) {
    const kp_existing_node &p = in->existing[x], &q = in->existing[y];
    if ((p.initialized != 0) != (q.initialized != 0)) return p.initialized != 0;
    return strcmp(p.name ? p.name : "", q.name ? q.name : "") < 0;
  });
  LabelIds lids(d);
  for (int i : ex) {
    const kp_existing_node& e = in->existing[i];
    cp.ex_input.push_back(i);
    cp.ex_reqs.push_back(CompileNode(d, raw.ex_labels[i], lids));
    vector<TaintT> ts;
    for (uint32_t j = 0; j < e.n_taints; j++)
      ts.push_back({e.taints[j].key ? e.taints[j].key : "", e.taints[j].value ? e.taints[j].value : "", e.taints[j].effect});
    cp.ex_taintset.push_back(tset(ts));
    for (int r = 0; r < KP_NRES; r++) {
      cp.ex_available.push_back((e.available.present >> r) & 1 ? e.available.milli[r] : 0);
      cp.ex_requests.push_back((e.requests.present >> r) & 1 ? e.requests.milli[r] : 0);
    }
  }
  if (tsets.size() > 64) return fail(KP_E_UNSUPPORTED, "%zu distinct taint sets (max 64)", tsets.size());
  pt.lap(" existing nodes");
  // shapes: levels, negop, tolerations, requests, per-catalogue PVP rows
  int sl = 0;
  for (uint32_t s = 0; s < in->n_shapes; s++) {
    const kp_pod_shape& sh = in->shapes[s];
    cp.shape_level_base.push_back(sl);
    cp.shape_nlevels.push_back((int32_t)raw.levels[s].size());
    for (int r = 0; r < KP_NRES; r++) cp.shape_requests.push_back((sh.requests.present >> r) & 1 ? sh.requests.milli[r] : 0);
    // Taints.ToleratesPod per taint set, with the pod's tolerations (+ toleratePreferNoScheduleTaints' at its level)
    auto tolerates = [&](bool pns) {
      uint64_t tol = 0;
      for (auto& kv : tsets) {
        bool all = true;
        for (auto& taint : kv.first) {
          bool ok = false;
          for (uint32_t j = 0; j < sh.n_tolerations + (pns ? 1 : 0) && !ok; j++) {
            const kp_toleration& t = j < sh.n_tolerations ? sh.tolerations[j] : kPnsToleration;
            const string tk = t.key ? t.key : "", tv = t.value ? t.value : "";
            if (t.effect != KP_EFFECT_ANY && t.effect != taint.effect) continue;
            if (!tk.empty() && tk != taint.key) continue;
            if (t.op == KP_TOL_EQUAL) ok = tv == taint.value;
            else if (t.op == KP_TOL_EXISTS) ok = true;
          }
          if (!ok) all = false;
        }
        if (all) tol |= 1ull << kv.second;
      }
      return tol;
    };
    const uint64_t tol0 = tolerates(false);
    for (size_t l = 0; l < raw.levels[s].size(); l++) {  // per shape-level: the PreferNoSchedule level differs
      const bool pns = (int)l == raw.pns_level[s];
      cp.shape_tolerates.push_back(pns ? tolerates(true) : tol0);
      cp.sl_pns.push_back(pns ? 1 : 0);
    }
    for (auto& lv : raw.levels[s]) {
      KReqs q = Compile(d, lv);
      cp.shape_reqs.push_back(q);
      cp.shape_negop.push_back(NegOp(d, q));
      vector<int32_t> slots(KP_MAX_KEYS, 0);
      for (size_t ci = 0; ci < b.cats.size(); ci++) {
        const HostCat& hc = b.cats[ci];
        cp.pvp_base.push_back((int32_t)(cp.pvp.size() / TW));
        int row = 0;
        if (ci == 0) cp.pvp_n.push_back(0);
        for (int k = 0; k < d.dd.K; k++) {
          if (!((q.present >> k) & 1) || !((d.dd.single_valued >> k) & 1)) continue;
          vector<uint64_t> acc(hc.NOKEY.begin() + (size_t)k * TW, hc.NOKEY.begin() + (size_t)(k + 1) * TW);
          for (int wi = 0, w = kw(d, k, 0); wi < nwords(d, k); wi++, w = wi < nwords(d, k) ? kw(d, k, wi) : 0) {
            uint64_t m = d.dd.validbits[w];
            while (m) {
              int bb = __builtin_ctzll(m);
              m &= m - 1;
              if (Has(d, q, k, w * 64 + bb))
                for (int x = 0; x < TW; x++) acc[x] |= hc.TM[(size_t)(w * 64 + bb) * TW + x];
            }
          }
          cp.pvp.insert(cp.pvp.end(), acc.begin(), acc.end());
          slots[k] = row++;  // same key order for every catalogue -> same relative slot
          if (ci == 0) cp.pvp_n.back() = row;
        }
      }
      cp.pvp_slot.insert(cp.pvp_slot.end(), slots.begin(), slots.end());
      sl++;
    }
  }
  if (cp.pvp.empty()) cp.pvp.assign(TW, 0);
  pt.lap(" shapes");
  {  // host ports: shapes, then the existing nodes in upstream order
    vector<vector<HostPortKey>> hs(in->n_shapes), hn;
    string err;
    for (uint32_t s2 = 0; s2 < in->n_shapes; s2++)
      if (!ParseHostPorts(in->shapes[s2].host_ports, in->shapes[s2].n_host_ports, &hs[s2], &err))
        return fail(KP_E_INVAL, "shape %u: %s", s2, err.c_str());
    for (int i : cp.ex_input) {
      hn.emplace_back();
      if (!ParseHostPorts(in->existing[i].host_ports, in->existing[i].n_host_ports, &hn.back(), &err))
        return fail(KP_E_INVAL, "existing node %d: %s", i, err.c_str());
    }
    const int32_t hrc = EncodeHostPorts(hs, hn, cp);
    if (hrc) return hrc;
  }
  {  // request classes: shapes with equal request rows share one (the run-length commit batches across them); a shape
     // with host ports is handed to the full path pod by pod, so it gets a class nothing else has
    std::map<vector<int64_t>, int32_t> cls;
    cp.shape_rclass.assign(in->n_shapes, 0);
    int32_t nc = 0;
    for (uint32_t s2 = 0; s2 < in->n_shapes; s2++) {
      if (cp.shape_hp_conf[s2]) {
        cp.shape_rclass[s2] = nc++;
        continue;
      }
      const vector<int64_t> row(cp.shape_requests.begin() + (size_t)s2 * KP_NRES,
                                cp.shape_requests.begin() + (size_t)(s2 + 1) * KP_NRES);
      auto it = cls.find(row);
      if (it == cls.end()) it = cls.emplace(row, nc++).first;
      cp.shape_rclass[s2] = it->second;
    }
    cp.n_rclass = nc;
  }
  pt.lap(" host ports");
  int32_t rc = CompileTopology(in, cp, raw.strict_levels, raw.spread_levels, b.np_taintset, raw.filter_levels);
  if (rc) return rc;
  pt.lap(" topology");
  {  // requirement classes: shape-levels whose compiled requirements (and so their negop and PVP rows) are equal share
     // one. Requirement.Intersection is idempotent, so once one member is merged into a NodeClaim, NodeClaim.Add of
     // every other member is Fits alone there: the device tags the whole class merged (SolveArgs::sl_rqc). A shape
     // with host ports is handed to the full path pod by pod and keeps a class of its own; with topology groups a
     // merge also narrows by the counts, so every level is its own class there
    const size_t SLn = cp.shape_reqs.size();
    std::map<string, int32_t> cls;
    cp.sl_rqc.assign(SLn, 0);
    cp.rqc_empty = -1;
    int32_t nc = 0;
    string key;
    for (uint32_t s2 = 0; s2 < in->n_shapes; s2++)
      for (int l = 0; l < cp.shape_nlevels[s2]; l++) {
        const size_t sl2 = (size_t)cp.shape_level_base[s2] + l;
        if (cp.G > 0 || cp.shape_hp_conf[s2]) {
          cp.sl_rqc[sl2] = nc++;
          continue;
        }
        key.assign(reinterpret_cast<const char*>(&cp.shape_reqs[sl2]), sizeof(KReqs));
        key.append(reinterpret_cast<const char*>(&cp.shape_negop[sl2]), sizeof(uint64_t));
        key.append(reinterpret_cast<const char*>(&cp.pvp_n[sl2]), sizeof(int32_t));
        auto it = cls.find(key);
        if (it == cls.end()) {
          it = cls.emplace(key, nc++).first;
          if (cp.shape_reqs[sl2].present == 0) cp.rqc_empty = it->second;
        }
        cp.sl_rqc[sl2] = it->second;
      }
    cp.rqc_off.assign((size_t)nc + 1, 0);
    for (size_t i = 0; i < SLn; i++) cp.rqc_off[(size_t)cp.sl_rqc[i] + 1]++;
    for (int32_t c = 0; c < nc; c++) cp.rqc_off[(size_t)c + 1] += cp.rqc_off[c];
    cp.rqc_mem.assign(std::max<size_t>(1, SLn), 0);
    vector<int32_t> fill(cp.rqc_off.begin(), cp.rqc_off.end() - 1);
    for (size_t i = 0; i < SLn; i++) cp.rqc_mem[fill[cp.sl_rqc[i]]++] = (int32_t)i;
  }
  pt.lap(" requirement classes");
  // pods: Queue order byCPUAndMemoryDescending (cpu desc, memory desc, creation asc, uid asc)
  cp.pod_shape.resize(in->n_pods);
  cp.queue.resize(in->n_pods);
  for (uint32_t p = 0; p < in->n_pods; p++) {
    if (in->pods[p].shape >= in->n_shapes) return fail(KP_E_INVAL, "pod %u: shape %u", p, in->pods[p].shape);
    cp.pod_shape[p] = (int32_t)in->pods[p].shape;
    cp.queue[p] = (int32_t)p;
  }
  // (cpu desc, memory desc) depends on the shape only: rank the shapes once, then sort the keys themselves
  // (rank, creation, uid, pod) in place, so the comparator reads contiguous memory instead of gathering per pod
  vector<int32_t> sorder(in->n_shapes), srank(in->n_shapes);
  for (uint32_t s2 = 0; s2 < in->n_shapes; s2++) sorder[s2] = (int32_t)s2;
  auto req_of = [&](int s2, int r) { return cp.shape_requests[(size_t)s2 * KP_NRES + r]; };
  std::sort(sorder.begin(), sorder.end(), [&](int x, int y) {
    if (req_of(x, KP_RES_CPU) != req_of(y, KP_RES_CPU)) return req_of(x, KP_RES_CPU) > req_of(y, KP_RES_CPU);
    return req_of(x, KP_RES_MEMORY) > req_of(y, KP_RES_MEMORY);
  });
  for (uint32_t i = 0, r = 0; i < in->n_shapes; i++) {  // equal (cpu, memory) share a rank
    if (i > 0 && (req_of(sorder[i], KP_RES_CPU) != req_of(sorder[i - 1], KP_RES_CPU) ||
                  req_of(sorder[i], KP_RES_MEMORY) != req_of(sorder[i - 1], KP_RES_MEMORY)))
      r = i;
    srank[sorder[i]] = (int32_t)r;
  }
  struct QKey {
    int32_t rank, pod;
    int64_t creation;
    uint64_t uid;
  };
  vector<uint64_t> uidk;  // the UIDs themselves (ABI v10): their rank in string order is the exact key
  if (in->pod_uids && !ExactUidKeys(in->pod_uids, in->n_pods, uidk)) return fail(KP_E_INVAL, "null pod uid");
  pt.lap(" queue: uid ranks");
  // the same order as one sort by (rank, creation, uid, pod): a counting sort by rank (ranks are < n_shapes), then each
  // rank's pods sorted by (creation, uid, pod) — short, cache-resident sorts instead of one over the whole batch
  vector<uint32_t> rstart(in->n_shapes + 1, 0);
  for (uint32_t p = 0; p < in->n_pods; p++) rstart[srank[cp.pod_shape[p]] + 1]++;
  for (uint32_t r = 0; r < in->n_shapes; r++) rstart[r + 1] += rstart[r];
  vector<QKey> qk(in->n_pods);
  {
    vector<uint32_t> fill(rstart.begin(), rstart.end() - 1);
    for (uint32_t p = 0; p < in->n_pods; p++) {
      const int32_t r = srank[cp.pod_shape[p]];
      qk[fill[r]++] = {r, (int32_t)p, in->pods[p].creation_unix, in->pod_uids ? uidk[p] : in->pods[p].uid_key};
    }
  }
  for (uint32_t r = 0; r < in->n_shapes; r++)
    if (rstart[r + 1] - rstart[r] > 1)
      std::sort(qk.begin() + rstart[r], qk.begin() + rstart[r + 1], [](const QKey& p, const QKey& q) {
        if (p.creation != q.creation) return p.creation < q.creation;
        if (p.uid != q.uid) return p.uid < q.uid;
        return p.pod < q.pod;
      });
  for (uint32_t p = 0; p < in->n_pods; p++) cp.queue[p] = qk[p].pod;
  {  // the fast lane's continuation round pays where most queue neighbours share their shape (deployments created in
     // bursts: runs of one shape-level); elsewhere its registers cost more than it saves (measured)
    // Its run-length commit also takes neighbours of different shapes with one request row (the queue is sorted by
    // cpu and memory, so shapes of one request class lie together): where most neighbours share their class and
    // some class holds more than one shape, the batches outweigh the registers
    uint32_t same = 0, same_rc = 0;
    for (uint32_t p = 1; p < in->n_pods; p++) {
      const int32_t s1 = cp.pod_shape[cp.queue[p]], s0 = cp.pod_shape[cp.queue[p - 1]];
      same += s1 == s0;
      same_rc += cp.shape_rclass[s1] == cp.shape_rclass[s0];
    }
    const bool runs = 2 * same >= in->n_pods;
    const bool mixed_runs = 2 * same_rc >= in->n_pods && cp.n_rclass < (int32_t)in->n_shapes;
    // (3: no continuation round, which only pays inside runs of one shape, and the open set's sequential loop in
    // place of the closed-form commit: the neighbours of one class mostly alternate between a few NodeClaims, which
    // the closed form on one NodeClaim cannot follow; config 2's kernel 160.3 -> 133.8 ms, measured. 2 stays built for
    // kp_overrides.fast_lane 3)
    cp.cont_hint = in->n_pods <= 1 ? 0 : runs ? 1 : mixed_runs ? 3 : 0;
  }
  pt.lap(" queue");
  return KP_OK;
}

// An ICE update (kp_catalog_update_offerings: availability, prices; never new offering classes) re-applied to a
// SolveBase in place: the offering arrays of every catalogue (FillOfferings with the base's class ids) and the
// templates' options (BuildTemplates), host side, then the same regions of the resident device copy. Returns 0 when
// done (version bumped), 1 when the base must be rebuilt instead (an offering of an unknown class, or the set of
// templates changed: a NodePool whose types all became unavailable, or the reverse), < 0 on a device error.
// Plans prepared on the base before the refresh see it through `version` (kp_solve_run refuses them until
// kp_solve_refresh).
// The refreshed state becomes current (stale checks pass) only here, after every device copy succeeded: a failed
// copy leaves the old seqnums, so the plans stay refused and a retried refresh copies again.
void CommitRefresh(SolveBase& b) {
  b.seqnums = SeqnumsOf(b.catalogs);
  b.key = b.ident + SeqKey(b.seqnums);
  b.version++;
}

int32_t RefreshOfferings(kp_ctx* ctx, SolveBase& b, bool commit = true) {
  map<ClassKey, int> classes;
  for (int c = 0; c < b.C; c++) classes[KeyOfClass(b.classes[c])] = c;
  for (auto* cat : b.catalogs)
    for (auto& t : cat->types)
      for (auto& o : t.offs)
        if (!classes.count(ClassOf(b.d, o))) return 1;
  vector<HostCat> saved;
  for (size_t i = 0; i < b.cats.size(); i++) {
    saved.push_back(HostCat());
    saved.back().offer_avail.swap(b.cats[i].offer_avail);
    saved.back().price.swap(b.cats[i].price);
    saved.back().price_cm.swap(b.cats[i].price_cm);
    saved.back().price_sub.swap(b.cats[i].price_sub);
    FillOfferings(b.d, b.catalogs[i]->types, b.TW, classes, b.cats[i]);
  }
  vector<int> tnp;
  vector<uint64_t> tX;
  BuildTemplates(b, tnp, tX);
  if (tnp != b.tmpl_nodepool) {  // restore: the caller rebuilds a fresh base (other plans may share this one)
    for (size_t i = 0; i < b.cats.size(); i++) {
      b.cats[i].offer_avail.swap(saved[i].offer_avail);
      b.cats[i].price.swap(saved[i].price);
      b.cats[i].price_cm.swap(saved[i].price_cm);
      b.cats[i].price_sub.swap(saved[i].price_sub);
    }
    return 1;
  }
  b.tmpl_X.swap(tX);
  if (ReservationTables(b)) return 1;  // (reservation classes are fixed by the dictionary: cannot fail here)
  if (b.on_device && ctx) {
    uint8_t* base = (uint8_t*)b.dev.p;
    hipStream_t st = ctx->stream;
    for (size_t i = 0; i < b.cats.size(); i++) {
      const HostCat& hc = b.cats[i];
      const CatOffsets& o = b.coffs[i];
      HIPCHK(hipMemcpyAsync(base + o.offer, hc.offer_avail.data(), hc.offer_avail.size() * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(base + o.price, hc.price.data(), hc.price.size() * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(base + o.price_cm, hc.price_cm.data(), hc.price_cm.size() * 8, hipMemcpyHostToDevice, st));
      if (!hc.price_sub.empty())
        HIPCHK(hipMemcpyAsync(base + o.price_sub, hc.price_sub.data(), hc.price_sub.size() * 8, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(base + b.o_tX, b.tmpl_X.data(), b.tmpl_X.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  if (commit) CommitRefresh(b);
  return 0;
}

// Compile a Solve. With a ctx, the SolveBase comes from (and goes to) the ctx cache when its fingerprint matches
// and its dictionary covers the batch; without one (kp_solve_validate) it is always built.
int32_t CompileSolve(const kp_solve_in* in, Compiled& cp, kp_ctx* cache = nullptr) {
  if (cache) cp.ov = cache->ov;
  SolveRaw raw;
  PhaseTimer pt;
  int32_t rc = ParseSolve(in, raw);
  if (rc) return rc;
  pt.lap("parse");
  const string ident = BaseIdent(in, raw);
  const string key = ident + SeqKey(SeqnumsOf(vector<const kp_catalog*>(in->catalogs, in->catalogs + in->n_catalogs)));
  if (cache) {
    for (int pass = 0; pass < 2; pass++)  // the exact fingerprint; then one whose catalogues only changed seqnum
      for (size_t i = 0; i < cache->bases.size(); i++) {
        auto& b = cache->bases[i];
        if ((pass == 0 ? b->key != key : b->ident != ident) || !BaseCovers(*b, raw)) continue;
        if (pass == 1) {  // an ICE update: re-apply the offerings in place (host + device) instead of a rebuild
          rc = RefreshOfferings(cache, *b);
          if (rc < 0) return rc;
          if (rc > 0) break;  // the templates changed: rebuild
          cp.base_refreshed = true;
        }
        cp.B = b;
        cp.base_hit = true;
        pt.lap("base lookup");
        rc = CompilePerCall(in, raw, cp);
        pt.lap("per-call compile");
        if (rc == KP_OK) {
          std::rotate(cache->bases.begin() + i, cache->bases.begin() + i + 1, cache->bases.end());  // most recent last
          cache->base_hits++;
          return KP_OK;
        }
        if (rc != KP_E_UNSUPPORTED) return rc;
        pass = 2;  // the cached dictionary's extra values may exceed a per-key limit: rebuild for this batch alone
        break;
      }
  }
  Compiled fresh;
  fresh.track_nodes = cp.track_nodes;
  fresh.ov = cp.ov;
  rc = BuildBase(in, raw, *fresh.B);
  if (rc) return rc;
  fresh.B->ident = ident;
  fresh.B->key = key;
  rc = CompilePerCall(in, raw, fresh);
  if (rc) return rc;
  cp = std::move(fresh);
  if (cache) {
    cache->base_misses++;
    for (size_t i = 0; i < cache->bases.size(); i++)
      if (cache->bases[i]->key == key) {
        cache->bases.erase(cache->bases.begin() + i);
        break;
      }
    cache->bases.push_back(cp.B);
    constexpr size_t kMaxBases = 4;
    if (cache->bases.size() > kMaxBases) cache->bases.erase(cache->bases.begin());
  }
  return KP_OK;
}

// Lays out dict + catalogues in `blob`; fills `catoffs` with the device DevCatalog array offset.

void PutCatalogs(Blob& blob, const Compiled& cp, vector<CatOffsets>& offs) {
  for (auto& hc : cp.B->cats) {
    CatOffsets o;
    o.TM = blob.put(hc.TM);
    o.DNE = blob.put(hc.DNE);
    o.NOKEY = blob.put(hc.NOKEY);
    o.alloc = blob.put(hc.alloc);
    o.cap = blob.put(hc.cap);
    o.nonneg = blob.put(hc.nonneg);
    o.fit_vals = blob.put(hc.fit_vals);
    o.fit_n = blob.put(hc.fit_n);
    o.fit_mask = blob.put(hc.fit_mask);
    o.cls = blob.put(cp.B->classes);
    o.offer = blob.put(hc.offer_avail);
    o.price = blob.put(hc.price);
    o.price_cm = blob.put(hc.price_cm);
    o.price_sub = blob.put(hc.price_sub);
    o.rank = blob.put(hc.name_rank);
    o.code = blob.put(hc.code);
    o.multi = blob.put(hc.multi);
    o.custom = blob.put(hc.custom_nonneg);
    offs.push_back(o);
  }
}
vector<DevCatalog> DevCats(uint8_t* base, const Compiled& cp, const vector<CatOffsets>& offs) {
  vector<DevCatalog> out;
  for (size_t i = 0; i < offs.size(); i++) {
    const CatOffsets& o = offs[i];
    DevCatalog c;
    c.TM = (const uint64_t*)(base + o.TM);
    c.DNE = (const uint64_t*)(base + o.DNE);
    c.NOKEY = (const uint64_t*)(base + o.NOKEY);
    c.vint = nullptr;
    c.alloc = (const int64_t*)(base + o.alloc);
    c.cap = (const int64_t*)(base + o.cap);
    c.nonneg = (const uint64_t*)(base + o.nonneg);
    c.fit_vals = (const int64_t*)(base + o.fit_vals);
    c.fit_n = (const int32_t*)(base + o.fit_n);
    c.fit_mask = (const uint64_t*)(base + o.fit_mask);
    c.cls = (const OfferClass*)(base + o.cls);
    c.offer_avail = (const uint64_t*)(base + o.offer);
    c.price = (const double*)(base + o.price);
    c.price_cm = (const double*)(base + o.price_cm);
    c.price_sub = cp.B->cats[i].price_sub.empty() ? nullptr : (const double*)(base + o.price_sub);
    c.name_rank = (const uint32_t*)(base + o.rank);
    c.code = (const uint16_t*)(base + o.code);
    c.multi = (const uint64_t*)(base + o.multi);
    c.custom_nonneg = (const uint64_t*)(base + o.custom);
    c.multi_valued = cp.B->cats[i].multi_valued;
    c.custom_any = cp.B->cats[i].custom_any;
    out.push_back(c);
  }
  return out;
}

// Device layout of one Solve. Offsets are relative to the shared region (the batch's read-only data: shapes, PVP
// rows, topology tables, the template-options table) or to the Solve's arena (its pods, the existing nodes it may
// use, its mutable state, device-only scratch). A single Solve keeps both in one allocation (shared == arena base);
// the batched general-path simulations (GeneralBatch) share one shared region between many arenas.
struct SolveOffs {
  // shared
  size_t slb = 0, snl = 0, sreqs = 0, sneg = 0, sreq = 0, stol = 0, pvp = 0, pvpb = 0, pvps = 0, pvpn = 0, tlp = 0,
         exts = 0, exav = 0, shpc = 0, shpa = 0, tgk = 0, tgr = 0, tgs = 0, tgm = 0, tga = 0, tgtb = 0, tgft = 0,
         tgt = 0, tgtn = 0, tgnt = 0, srb = 0, srn = 0, recl = 0, recx = 0, slft = 0, slob = 0, slon = 0, owng = 0,
         owns = 0, ownp = 0, ownr = 0, sltk = 0, tks = 0, extc = 0, tkk = 0, slsh = 0, tfeas = 0, exul = 0, exuo = 0,
         exui = 0, slst = 0, srcl = 0, rqcs = 0, rqco = 0, rqcm = 0;
  // arena: the Solve's inputs, then its mutable state [mut, mut_end) (restored before every run; [mut, common) is the
  // part a batched simulation patches, [common, mut_end) the part every simulation starts from alike), then
  // device-only regions
  size_t pod_shape = 0, exso = 0, mut = 0, queue = 0, tgc = 0, tglv = 0, tgreg = 0, hcx = 0, common = 0,
         pod_level = 0, lastlen = 0, lastlen_ep = 0, trem = 0, exr = 0, exrq = 0, exroom = 0, exhp = 0, mut_end = 0;
  size_t pristine = 0, ncr = 0, ncX = 0, ncrq = 0, nct = 0, npods = 0, order = 0, chkblk = 0, maxalloc = 0, fitj = 0,
         nchead = 0, nccat = 0, nchp = 0, place = 0, events = 0, stats = 0, ver0 = 0, exver = 0, tver = 0, curnc = 0,
         curex = 0, held = 0, exown = 0, ver_end = 0, fail0 = 0, ncfail = 0, exfail = 0, tfail = 0, chkdead = 0, fail_end = 0,
         opts = 0, nrem = 0, nopt = 0, hcnc = 0, nctc = 0, txl = 0, txlv = 0, slfail = 0, arena_end = 0;
  size_t n_hcnc = 0;
  int ncc = 0, chk_dead_rows = 0, sort_cap = 0, opt_stride = 0;
  bool chk_on = false;
};

// the resources some shape requests or some template's daemon overhead holds: Fits iterates every resource of the
// merged requests
uint32_t RequestedResources(const Compiled& C) {
  uint32_t m = 0;
  for (size_t i = 0; i < C.shape_requests.size(); i++)
    if (C.shape_requests[i] > 0) m |= 1u << (i % KP_NRES);
  for (size_t i = 0; i < C.B->tmpl_daemon.size(); i++)
    if (C.B->tmpl_daemon[i] > 0) m |= 1u << (i % KP_NRES);
  return m;
}

// per existing node: 1 when its unrequested resources never fail a pod (they never change), else 0
vector<uint8_t> ExStatic(const Compiled& C, uint32_t rmask) {
  const int E = (int)C.ex_reqs.size();
  vector<uint8_t> ok(std::max(E, 1), 0);
  for (int e = 0; e < E; e++) {
    bool good = true;
    for (int r = 0; r < KP_NRES; r++) {
      const int64_t av = C.ex_available[(size_t)e * KP_NRES + r], rq = C.ex_requests[(size_t)e * KP_NRES + r];
      if (av < 0 || (!((rmask >> r) & 1) && rq > av)) good = false;
    }
    ok[e] = good ? 1 : 0;
  }
  return ok;
}

// The fast lane's stage record of each shape-level (topology Solves; SolveArgs::sl_stage): everything static the pod
// loop reads at a pod's start in one 256-byte row, so that the next pod's row is one prefetched load (lane d holds
// dword d) instead of three dependent rounds (level -> owned-group base -> owned-group records -> counts).
//   [0] 0: the fast lane may take the level (sl_fast_topo, no host-port conflicts)  [1..2] tolerated taint sets
//   [3] owned groups  [4] 1: no requirements at the level  [5..6] recorded groups: count, rec_list base
//   [8 + 8j ..] owned group j < 4: own_rec's eight dwords  [40 + 2j ..] its podDomains  [48 + 2i ..] recorded
//   group i < 8: (group, rec_aux)
vector<int32_t> StageRecords(const Compiled& C) {
  const size_t SL = C.shape_reqs.size();
  if (!C.G) return vector<int32_t>(64, 0);
  vector<int32_t> st(std::max<size_t>(SL, 1) * 64, 0);
  for (size_t sh = 0; sh < C.shape_level_base.size(); sh++)
    for (int l = 0; l < C.shape_nlevels[sh]; l++) {
      const size_t sl = (size_t)C.shape_level_base[sh] + l;
      int32_t* r = &st[sl * 64];
      r[0] = (1 - C.sl_fast_topo[sl]) + (C.hp_any && C.shape_hp_conf[sh] ? 1 : 0);
      r[1] = (int32_t)(uint32_t)C.shape_tolerates[sl];
      r[2] = (int32_t)(uint32_t)(C.shape_tolerates[sl] >> 32);
      const int on = C.sl_own_n[sl], ob = C.sl_own_base[sl];
      r[3] = on;
      r[4] = C.shape_reqs[sl].present == 0 ? 1 : 0;
      r[5] = C.shape_rec_n[sh];
      r[6] = C.shape_rec_base[sh];
      for (int j = 0; j < std::min(on, 4); j++) {
        for (int k = 0; k < 8; k++) r[8 + 8 * j + k] = C.own_rec[(size_t)(ob + j) * 8 + k];
        r[40 + 2 * j] = (int32_t)(uint32_t)C.own_pd[ob + j];
        r[41 + 2 * j] = (int32_t)(uint32_t)(C.own_pd[ob + j] >> 32);
      }
      for (int i = 0; i < std::min(C.shape_rec_n[sh], 8); i++) {
        r[48 + 2 * i] = C.rec_list[(size_t)C.shape_rec_base[sh] + i];
        r[49 + 2 * i] = C.rec_aux[(size_t)C.shape_rec_base[sh] + i];
      }
    }
  return st;
}

void PutShared(Blob& blob, const Compiled& C, SolveOffs& o) {
  o.slb = blob.put(C.shape_level_base);
  o.snl = blob.put(C.shape_nlevels);
  o.sreqs = blob.put(C.shape_reqs);
  o.sneg = blob.put(C.shape_negop);
  o.sreq = blob.put(C.shape_requests);
  o.stol = blob.put(C.shape_tolerates);
  o.pvp = blob.put(C.pvp);
  o.pvpb = blob.put(C.pvp_base);
  o.pvps = blob.put(C.pvp_slot);
  o.pvpn = blob.put(C.pvp_n);
  o.tlp = blob.put(C.tmpl_limit_present);
  o.exts = blob.put(C.ex_taintset);
  o.exav = blob.put(C.ex_available);
  o.shpc = blob.put(C.shape_hp_conf);
  o.shpa = blob.put(C.shape_hp_add);
  o.srcl = blob.put(C.shape_rclass);
  o.rqcs = blob.put(C.sl_rqc), o.rqco = blob.put(C.rqc_off), o.rqcm = blob.put(C.rqc_mem);
  // topology (read-only part)
  o.tgk = blob.put(C.tg_key), o.tgr = blob.put(C.tg_row), o.tgs = blob.put(C.tg_maxskew), o.tgm = blob.put(C.tg_mindom);
  o.tga = blob.put(C.tg_aff), o.tgtb = blob.put(C.tg_term_base), o.tgft = blob.put(C.tg_filt_tol);
  o.tgt = blob.put(C.tg_terms), o.tgtn = blob.put(C.tg_terms_negop), o.tgnt = blob.put(C.tg_nterm);
  o.srb = blob.put(C.shape_rec_base), o.srn = blob.put(C.shape_rec_n), o.recl = blob.put(C.rec_list);
  o.recx = blob.put(C.rec_aux), o.slft = blob.put(C.sl_fast_topo), o.slob = blob.put(C.sl_own_base);
  o.slon = blob.put(C.sl_own_n), o.owng = blob.put(C.own_group), o.owns = blob.put(C.own_self);
  o.ownp = blob.put(C.own_pd), o.ownr = blob.put(C.own_rec), o.sltk = blob.put(C.sl_topo_keys);
  o.tks = blob.put(C.tkey_slot), o.extc = blob.put(C.ex_tcode), o.tkk = blob.put(C.tk_keys);
  // shape of each shape-level (tmpl_feas_kernel)
  vector<int32_t> sl_shape(std::max<size_t>(1, C.shape_reqs.size()), 0);
  for (size_t sh = 0; sh < C.shape_level_base.size(); sh++)
    for (int l = 0; l < C.shape_nlevels[sh]; l++) sl_shape[(size_t)C.shape_level_base[sh] + l] = (int32_t)sh;
  o.slsh = blob.put(sl_shape);
  o.slst = blob.put(StageRecords(C));
}

// The arena's host-initialised part: the pods (pod_shape / queue of Pc entries), the existing nodes' static check,
// then the mutable state.
void PutArena(Blob& blob, const Compiled& C, const vector<int32_t>& pod_shape, const vector<int32_t>& queue, int Pc,
              const vector<uint8_t>& ex_static, uint32_t rmask, SolveOffs& o) {
  const int E = (int)C.ex_reqs.size();
  o.pod_shape = blob.put(pod_shape);
  o.exso = blob.put(ex_static);
  o.mut = blob.reserve(0);
  o.queue = blob.put(queue);
  o.tgc = blob.put(C.tg_cnt);
  o.tglv = blob.put(C.tg_live);
  o.tgreg = blob.put(C.tg_reg);
  o.hcx = blob.put(C.hcnt0);
  o.common = blob.reserve(0);
  const vector<int32_t> zeros_p(Pc, 0);
  o.pod_level = blob.put(zeros_p);
  o.lastlen = blob.put(zeros_p);
  o.lastlen_ep = blob.put(zeros_p);
  o.trem = blob.put(C.tmpl_remaining);
  o.exrq = blob.put(C.ex_requests);
  // headroom rows of the existing nodes for the first four requested resources (req_res_mask order)
  vector<int64_t> ex_room((size_t)4 * std::max(E, 1), INT64_MAX);
  for (int r = 0, k = 0; r < KP_NRES && k < 4; r++) {
    if (!((rmask >> r) & 1)) continue;
    for (int e = 0; e < E; e++)
      ex_room[(size_t)k * E + e] = C.ex_available[(size_t)e * KP_NRES + r] - C.ex_requests[(size_t)e * KP_NRES + r];
    k++;
  }
  o.exroom = blob.put(ex_room);
  o.exhp = blob.put(C.ex_hp);
  // last of the mutable block: a batched simulation does not copy it (copy-on-write from the pristine block, ex_own)
  o.exr = blob.put(C.ex_reqs);
  o.mut_end = blob.host.size();
}

// The arena's device-only regions (after every put of the blob). with_pristine: a device copy of the mutable state
// (single Solves restore from it; batched simulations restore from the shared one).
void ReserveArenaDev(Blob& blob, const Compiled& C, int Pc, int opt_stride, int sort_cap, bool with_pristine, SolveOffs& o,
                     size_t ex_fail_entries = SIZE_MAX) {
  const int TW = C.B->TW, NT = (int)C.B->tmpl_reqs.size(), E = (int)C.ex_reqs.size();
  o.pristine = with_pristine ? blob.reserve_dev(o.mut_end - o.mut) : 0;
  o.ncr = blob.reserve_dev(sizeof(KReqs) * Pc);
  o.ncX = blob.reserve_dev(sizeof(uint64_t) * (size_t)Pc * TW);
  o.ncrq = blob.reserve_dev(sizeof(int64_t) * (size_t)Pc * KP_NRES);
  o.nct = blob.reserve_dev(sizeof(int32_t) * Pc);
  o.npods = blob.reserve_dev(sizeof(int32_t) * Pc);
  o.order = blob.reserve_dev(sizeof(int32_t) * Pc);
  // chunked newNodeClaims order past the LDS sort capacity (blocks + per (shape-level, block) dead marks): only when
  // the Solve can create more NodeClaims than the LDS holds
  o.sort_cap = sort_cap;
  o.chk_on = Pc > sort_cap;
  o.chkblk = blob.reserve_dev(o.chk_on ? sizeof(ChkBlk) * CHK_MAXC : 8);
  o.maxalloc = blob.reserve_dev(sizeof(int64_t) * (size_t)Pc * KP_NRES);
  o.fitj = blob.reserve_dev(sizeof(int32_t) * (size_t)Pc * KP_NRES);
  o.nchead = blob.reserve_dev(sizeof(NcHead) * (size_t)Pc + 64);
  o.nccat = blob.reserve_dev(sizeof(int32_t) * (size_t)Pc);
  o.nchp = blob.reserve_dev(C.hp_any ? sizeof(uint64_t) * (size_t)Pc : 8);
  o.place = blob.reserve_dev(sizeof(int32_t) * Pc);
  o.events = blob.reserve_dev(sizeof(int32_t) * Pc);
  o.stats = blob.reserve_dev(sizeof(uint64_t) * KP_SOLVE_STATS);
  // failure memo (see SolveArgs): versions start at 0, memo entries at -1
  const size_t SLn = std::max<size_t>(1, C.shape_reqs.size());
  o.ncc = (int)std::min<size_t>((size_t)Pc, std::max<size_t>(1, ((size_t)256 << 20) / (4 * SLn)));
  o.ver0 = blob.reserve_dev(0);
  o.exver = blob.reserve_dev(sizeof(int32_t) * std::max(E, 1));
  o.tver = blob.reserve_dev(sizeof(int32_t) * std::max(NT, 1));
  o.curnc = blob.reserve_dev(sizeof(int32_t) * 2 * SLn);  // cursors start at {0, 0} (zeroed per run)
  o.curex = blob.reserve_dev(sizeof(int32_t) * 2 * SLn);
  o.held = blob.reserve_dev(C.B->res_cls ? sizeof(uint64_t) * (size_t)Pc : 8);
  o.exown = blob.reserve_dev(sizeof(uint64_t) * (size_t)std::max(1, (E + 63) / 64));  // copy-on-write bits (zeroed)
  o.ver_end = blob.total();
  o.fail0 = blob.reserve_dev(0);
  o.ncfail = blob.reserve_dev(sizeof(int32_t) * SLn * o.ncc);
  // (batched simulations: one entry per usable-list entry of each shape-level, SolveArgs::ex_ulist)
  o.exfail = blob.reserve_dev(sizeof(int32_t) * (ex_fail_entries != SIZE_MAX ? std::max<size_t>(ex_fail_entries, 1)
                                                                               : SLn * std::max(E, 1)));
  o.tfail = blob.reserve_dev(sizeof(int32_t) * SLn * std::max(NT, 1));
  o.txlv = blob.reserve_dev(sizeof(int32_t) * std::max(NT, 1));  // -1: not computed
  o.slfail = blob.reserve_dev(sizeof(int32_t) * SLn);  // -1: no failure yet
  o.chk_dead_rows = o.chk_on ? (int)std::min<size_t>(SLn, ((size_t)64 << 20) / (4 * CHK_MAXC)) : 0;
  o.chkdead = blob.reserve_dev(std::max<size_t>(sizeof(int32_t) * o.chk_dead_rows * CHK_MAXC, 8));
  o.fail_end = blob.total();
  o.opt_stride = opt_stride;
  o.txl = blob.reserve_dev(sizeof(uint64_t) * (size_t)std::max(NT, 1) * TW);
  o.opts = blob.reserve_dev(sizeof(uint32_t) * (size_t)Pc * opt_stride);
  o.nrem = blob.reserve_dev(sizeof(uint32_t) * Pc);
  o.nopt = blob.reserve_dev(sizeof(uint32_t) * Pc);
  o.n_hcnc = (size_t)C.GH * Pc;
  o.hcnc = blob.reserve_dev(std::max<size_t>(o.n_hcnc, 1));
  o.nctc = blob.reserve_dev(std::max<size_t>((size_t)C.TK * Pc, 1));
  o.arena_end = blob.total();
}

// SolveArgs of one Solve over the shared region `sh` and the arena `ar` (offsets from `o`).
void BindSolve(SolveArgs& a, const Compiled& C, const SolveOffs& o, uint8_t* sh, uint8_t* ar, int n_pods, int Pc,
               uint32_t rmask, int res_mode) {
  uint8_t* cbase = (uint8_t*)C.B->dev.p;
  memset(&a, 0, sizeof a);
  a.dict = (const DevDict*)(cbase + C.B->o_dict);
  a.cats = (const DevCatalog*)(cbase + C.B->o_cats);
  a.n_catalogs = (int32_t)C.B->cats.size();
  a.vint = (const int64_t*)(cbase + C.B->o_vint);
  a.n_pods = n_pods;
  a.pod_shape = (const int32_t*)(ar + o.pod_shape);
  a.pod_level = (int32_t*)(ar + o.pod_level);
  a.queue = (int32_t*)(ar + o.queue);
  a.lastlen = (int32_t*)(ar + o.lastlen);
  a.lastlen_epoch = (int32_t*)(ar + o.lastlen_ep);
  a.shape_level_base = (const int32_t*)(sh + o.slb);
  a.shape_nlevels = (const int32_t*)(sh + o.snl);
  a.shape_reqs = sh + o.sreqs;
  a.shape_negop = (const uint64_t*)(sh + o.sneg);
  a.shape_requests = (const int64_t*)(sh + o.sreq);
  a.shape_tolerates = (const uint64_t*)(sh + o.stol);
  a.shape_pvp = (const uint64_t*)(sh + o.pvp);
  a.pvp_base = (const int32_t*)(sh + o.pvpb);
  a.pvp_slot = (const int32_t*)(sh + o.pvps);
  a.sl_pvp_n = (const int32_t*)(sh + o.pvpn);
  a.n_tmpl = (int32_t)C.B->tmpl_reqs.size();
  a.tmpl_reqs = cbase + C.B->o_treqs;
  a.tmpl_taintset = (const int32_t*)(cbase + C.B->o_tts);
  a.tmpl_catalog = (const int32_t*)(cbase + C.B->o_tcat);
  a.tmpl_X = (const uint64_t*)(cbase + C.B->o_tX);
  a.tmpl_daemon = (const int64_t*)(cbase + C.B->o_tdm);
  a.tmpl_limit_present = (const uint32_t*)(sh + o.tlp);
  a.tmpl_remaining = (int64_t*)(ar + o.trem);
  a.n_existing = (int32_t)C.ex_reqs.size();
  a.ex_reqs = ar + o.exr;
  a.ex_reqs_ro = nullptr;  // (batched simulations: GeneralBatchRun points it at the pristine block)
  a.ex_own = (uint64_t*)(ar + o.exown);
  a.ex_taintset = (const int32_t*)(sh + o.exts);
  a.ex_available = (const int64_t*)(sh + o.exav);
  a.ex_requests = (int64_t*)(ar + o.exrq);
  a.ex_room = (int64_t*)(ar + o.exroom);
  a.nc_reqs = ar + o.ncr;
  a.nc_X = (uint64_t*)(ar + o.ncX);
  a.nc_requests = (int64_t*)(ar + o.ncrq);
  a.nc_tmpl = (int32_t*)(ar + o.nct);
  a.g_npods = (int32_t*)(ar + o.npods);
  a.g_order = (int32_t*)(ar + o.order);
  a.sort_in_lds = 1;
  a.sort_cap = o.sort_cap;
  a.ncc = o.ncc;
  a.chk_blk = (ChkBlk*)(ar + o.chkblk);
  a.chk_dead = (int32_t*)(ar + o.chkdead);
  a.chk_dead_rows = o.chk_dead_rows;
  a.chk_maxc = o.chk_on ? CHK_MAXC : 0;
  if (C.ov.chunk_capacity) a.chk_maxc = o.chk_on ? std::max(0, std::min(CHK_MAXC, C.ov.chunk_capacity)) : 0;
  a.nc_head = (NcHead*)(((uintptr_t)(ar + o.nchead) + 63) & ~(uintptr_t)63);
  a.nc_fail = (int32_t*)(ar + o.ncfail);
  a.ex_ver = (int32_t*)(ar + o.exver);
  a.ex_fail = (int32_t*)(ar + o.exfail);
  a.tmpl_ver = (int32_t*)(ar + o.tver);
  a.tmpl_fail = (int32_t*)(ar + o.tfail);
  a.tmpl_xlim = (uint64_t*)(ar + o.txl);
  a.tmpl_xlim_ver = (int32_t*)(ar + o.txlv);
  a.sl_fail = (int32_t*)(ar + o.slfail);
  a.cur_nc = (int32_t*)(ar + o.curnc);
  a.cur_ex = (int32_t*)(ar + o.curex);
  a.nc_maxalloc = (int64_t*)(ar + o.maxalloc);
  a.nc_fitj = (int32_t*)(ar + o.fitj);
  a.nc_cat = (int32_t*)(ar + o.nccat);
  a.hp_any = C.hp_any ? 1 : 0;
  a.shape_hp_conf = (const uint64_t*)(sh + o.shpc);
  a.shape_hp_add = (const uint64_t*)(sh + o.shpa);
  a.shape_rclass = (const int32_t*)(sh + o.srcl);
  a.sl_rqc = (const int32_t*)(sh + o.rqcs);
  a.rqc_off = (const int32_t*)(sh + o.rqco);
  a.rqc_mem = (const int32_t*)(sh + o.rqcm);
  a.rqc_empty = C.rqc_empty;
  a.ex_hp = (uint64_t*)(ar + o.exhp);
  a.nc_hp = (uint64_t*)(ar + o.nchp);
  a.req_res_mask = rmask;
  a.n_req_res = __builtin_popcount(rmask);
  a.timing = C.ov.timing ? 1 : 0;
  // kp_overrides.fast_lane: 1 plain, 2 cont 1, 3 cont 2, 4 cont 3. solve_kernel's dispatch takes a forced value as it takes
  // the hint: cont 1 to 3 are instantiated for the LDS order without topology and without existing nodes only, and
  // every other Solve (topology, existing nodes, the chunked or flat order from the spill on) runs CONT 0
  a.cont = C.ov.fast_lane ? (C.ov.fast_lane == 2 ? 1 : C.ov.fast_lane == 3 ? 2 : C.ov.fast_lane == 4 ? 3 : 0) : C.cont_hint;
  a.n_groups = C.G;
  a.tg_key = (const int32_t*)(sh + o.tgk);
  a.tg_row = (const int32_t*)(sh + o.tgr);
  a.tg_maxskew = (const int32_t*)(sh + o.tgs);
  a.tg_mindom = (const int32_t*)(sh + o.tgm);
  a.tg_aff = (const int32_t*)(sh + o.tga);
  a.tg_term_base = (const int32_t*)(sh + o.tgtb);
  a.tg_filt_tol = (const uint64_t*)(sh + o.tgft);
  a.tg_terms = sh + o.tgt;
  a.tg_terms_negop = (const uint64_t*)(sh + o.tgtn);
  a.tg_cnt = (int32_t*)(ar + o.tgc);
  a.tg_live = (int32_t*)(ar + o.tglv);
  a.tg_nterm = (const int32_t*)(sh + o.tgnt);
  a.tg_reg = (uint64_t*)(ar + o.tgreg);
  a.hcnt_ex = ar + o.hcx;
  a.hcnt_nc = ar + o.hcnc;
  a.hnc_stride = Pc;
  a.shape_rec_base = (const int32_t*)(sh + o.srb);
  a.shape_rec_n = (const int32_t*)(sh + o.srn);
  a.rec_list = (const int32_t*)(sh + o.recl);
  a.rec_aux = (const int32_t*)(sh + o.recx);
  a.sl_fast_topo = (const int32_t*)(sh + o.slft);
  a.sl_own_base = (const int32_t*)(sh + o.slob);
  a.sl_own_n = (const int32_t*)(sh + o.slon);
  a.own_group = (const int32_t*)(sh + o.owng);
  a.own_self = (const int32_t*)(sh + o.owns);
  a.own_pd = (const uint64_t*)(sh + o.ownp);
  a.own_rec = (const int4*)(sh + o.ownr);
  a.sl_stage = (const int32_t*)(sh + o.slst);
  a.sl_topo_keys = (const uint64_t*)(sh + o.sltk);
  a.tkey_slot = (const int32_t*)(sh + o.tks);
  a.n_tk = C.TK;
  a.tk_keys = (const int32_t*)(sh + o.tkk);
  a.nc_tcode = ar + o.nctc;
  a.ex_static_ok = ar + o.exso;
  a.ex_tcode = sh + o.extc;
  a.placement = (int32_t*)(ar + o.place);
  a.events = (int32_t*)(ar + o.events);
  a.stats = (uint64_t*)(ar + o.stats);
  a.res_mode = res_mode;
  a.res_cls = C.B->res_cls;
  a.nc_held = (uint64_t*)(ar + o.held);
  for (int c = 0; c < KP_MAX_CLASSES; c++) a.res_cap0[c] = C.B->res_cap0.empty() ? 0 : C.B->res_cap0[c];
}

// The template-options table's launch over rows [row_lo, row_hi) (out: `words` u64 per (shape-level, template)).
TfeasArgs TfeasOf(const SolveArgs& a, const uint8_t* sh, const SolveOffs& o, int rows, int words) {
  TfeasArgs f;
  memset(&f, 0, sizeof f);
  f.dict = a.dict;
  f.cats = a.cats;
  f.n_catalogs = a.n_catalogs;
  f.vint = a.vint;
  f.n_tmpl = a.n_tmpl;
  f.tmpl_reqs = a.tmpl_reqs;
  f.tmpl_catalog = a.tmpl_catalog;
  f.tmpl_X = a.tmpl_X;
  f.tmpl_daemon = a.tmpl_daemon;
  f.shape_reqs = a.shape_reqs;
  f.shape_negop = a.shape_negop;
  f.sl_shape = (const int32_t*)(sh + o.slsh);
  f.shape_requests = a.shape_requests;
  f.shape_pvp = a.shape_pvp;
  f.pvp_base = a.pvp_base;
  f.pvp_slot = a.pvp_slot;
  f.sl_own_n = a.sl_own_n;
  f.req_res_mask = a.req_res_mask;
  f.row_lo = 0;
  f.row_hi = rows;
  f.words = words;
  f.out = (uint64_t*)(sh + o.tfeas);
  return f;
}

// the newNodeClaims order lives in LDS (64 KiB) up to this many NodeClaims, then spills
int SortCapacity(const kp_overrides& ov) { return ov.sort_capacity > 0 ? std::min(8192, ov.sort_capacity) : 8192; }

}  // namespace

extern "C" {

}  // extern "C"

// A communicator of n_ranks kp_ctx (one per GPU): RCCL (kp_comm_init / kp_comm_init_all), or a caller-supplied host
// all-gather (kp_comm_init_host). Its settings are read once here, so that every rank takes the same decisions.
struct kp_comm {
  CtxRef ctx;
  ncclComm_t comm = nullptr;        // RCCL transport (null: host transport)
  kp_allgather_fn host_fn = nullptr;
  void* host_user = nullptr;
  int n_ranks = 1, rank = 0;
  bool no_tfeas = false;            // kp_overrides.template_table at init: no template-options table
  uint64_t tfeas_shard_min = 0;     // shard the table over the ranks from this many (shape-level, template) pairs
  DevBuf buf;  // [0]: this rank's record, [1..n_ranks]: the gathered records
};

namespace {
// All-gather of `bytes` per rank over host buffers (recv: n_ranks * bytes in rank order), through the comm's
// transport. Every rank of a collective step calls this exactly once per step, whatever its local outcome: a rank
// that failed locally sends a record saying so (the callers' status / KP_CHOICE_FAILED records), so no peer is left
// waiting in the collective.
int32_t CommExchange(kp_comm* c, const void* send, void* recv, size_t bytes) {
  if (c->host_fn) {
    if (c->host_fn(c->host_user, c->rank, send, recv, bytes) != 0)
      return fail(KP_E_DEVICE, "host all-gather callback failed (rank %d)", c->rank);
    return KP_OK;
  }
  hipStream_t st = c->ctx->stream;
  if (c->buf.n < bytes * (size_t)(c->n_ranks + 1)) {
    c->buf.reset();
    HIPCHK(c->buf.alloc(bytes * (size_t)(c->n_ranks + 1)));
  }
  uint8_t* dev = (uint8_t*)c->buf.p;
  HIPCHK(hipMemcpyAsync(dev, send, bytes, hipMemcpyHostToDevice, st));
  ncclResult_t r = ncclAllGather(dev, dev + bytes, bytes, ncclUint8, c->comm, st);
  if (r != ncclSuccess) return fail(KP_E_DEVICE, "ncclAllGather: %s", ncclGetErrorString(r));
  HIPCHK(hipMemcpyAsync(recv, dev + bytes, bytes * (size_t)c->n_ranks, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return KP_OK;
}
// Device-to-device all-gather (the template-options table): RCCL directly, or staged through the host transport.
int32_t CommAllGatherDev(kp_comm* c, const void* send, void* recv, size_t bytes) {
  hipStream_t st = c->ctx->stream;
  if (!c->host_fn) {
    ncclResult_t r = ncclAllGather(send, recv, bytes, ncclUint8, c->comm, st);
    if (r != ncclSuccess) return fail(KP_E_DEVICE, "ncclAllGather: %s", ncclGetErrorString(r));
    HIPCHK(hipStreamSynchronize(st));
    return KP_OK;
  }
  vector<uint8_t> hs(bytes), hr(bytes * (size_t)c->n_ranks);
  const hipError_t e = hipMemcpyAsync(hs.data(), send, bytes, hipMemcpyDeviceToHost, st);
  const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(st) : e;
  int32_t rc = CommExchange(c, hs.data(), hr.data(), bytes);  // reached even when the copy failed
  if (e2 != hipSuccess) return fail(KP_E_DEVICE, "all-gather staging: %s", hipGetErrorString(e2));
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(recv, hr.data(), hr.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return KP_OK;
}
void CommReadSettings(kp_comm* c) {
  c->no_tfeas = c->ctx->ov.template_table != 0;
  // the table costs ~10 us per 1k pairs on one GPU and an all-gather tens of us: shard only tables worth it
  c->tfeas_shard_min = 1u << 20;
  if (c->ctx->ov.table_shard_min) c->tfeas_shard_min = c->ctx->ov.table_shard_min;
}

// Per (shape-level, template) whose taints the level does not tolerate (shape_tolerates): the index, in the NodePool's
// own taints order, of the first taint no toleration of the level matches (Taints.ToleratesPod reports the first);
// -1 where every taint is tolerated.
vector<int32_t> TaintFirst(const kp_solve_in* in, const Compiled& C) {
  const SolveBase& b = *C.B;
  const size_t NT = b.tmpl_nodepool.size(), SL = C.shape_reqs.size();
  vector<int32_t> out(std::max<size_t>(SL * NT, 1), -1);
  for (size_t s = 0; s < C.shape_level_base.size(); s++) {
    const kp_pod_shape& sh = in->shapes[s];
    for (int l = 0; l < C.shape_nlevels[s]; l++) {
      const size_t sl = (size_t)C.shape_level_base[s] + l;
      const bool pns = C.sl_pns[sl] != 0;
      for (size_t t = 0; t < NT; t++) {
        if ((C.shape_tolerates[sl] >> b.tmpl_taintset[t]) & 1) continue;
        const kp_nodepool& np = in->nodepools[b.tmpl_nodepool[t]];
        for (uint32_t i = 0; i < np.n_taints && out[sl * NT + t] < 0; i++) {
          const string xk = np.taints[i].key ? np.taints[i].key : "", xv = np.taints[i].value ? np.taints[i].value : "";
          bool ok = false;
          for (uint32_t j = 0; j < sh.n_tolerations + (pns ? 1 : 0) && !ok; j++) {
            const kp_toleration& tl = j < sh.n_tolerations ? sh.tolerations[j] : kPnsToleration;
            const string tk = tl.key ? tl.key : "", tv = tl.value ? tl.value : "";
            if (tl.effect != KP_EFFECT_ANY && tl.effect != np.taints[i].effect) continue;
            if (!tk.empty() && tk != xk) continue;
            if (tl.op == KP_TOL_EQUAL) ok = tv == xv;
            else if (tl.op == KP_TOL_EXISTS) ok = true;
          }
          if (!ok) out[sl * NT + t] = (int32_t)i;
        }
      }
    }
  }
  return out;
}
}  // namespace

struct kp_solve_plan {
  CtxRef ctx;
  std::unique_ptr<Compiled> cp;
  DevBuf buf;  // per-Solve arena (the catalogue / template part lives in cp->B->dev, shared through the ctx cache)
  SolveArgs a;
  double catalog_ms = 0;  // SolveBase build time when this prepare missed the cache, else 0
  double compile_ms = 0;  // host CompileSolve time of this prepare (KP_HOST_TIMING)
  size_t o_mut = 0, n_mut = 0, o_pristine = 0, o_ver = 0, n_ver = 0, o_fail = 0, n_fail = 0;
  size_t o_stats = 0, o_npods = 0, o_place = 0, o_events = 0, o_nct = 0, o_ncrq = 0, o_opts = 0, o_nrem = 0,
         o_nopt = 0, o_ncr = 0, o_hcnc = 0, n_hcnc = 0, o_held = 0;
  int opt_stride = 0, P = 0, Pc = 1;
  uint32_t max_types = 0;
  bool any_min = false;
  double prepare_ms = 0;
  uint64_t base_version = 0;  // SolveBase::version the plan's derived data (template-options table) reflects
  TfeasArgs tf;               // the table's launch over every row (kp_solve_refresh recomputes it locally)
  bool tfeas_on = false;
  // the explanation step (kp_solve_run_explained): its launch, the arena block it writes (records, then the per-pod row
  // index: one download) and the mark table behind it; per (shape-level, template) the index in the NodePool's taints
  // of the first taint the level does not tolerate (-1: all tolerated)
  ExplainArgs ex;
  size_t o_why = 0, n_why = 0, o_mark = 0, n_mark = 0;
  vector<int32_t> taint_first;
};

extern "C" {

// Compile the batch (dictionary, bitsets, catalogue SoA, templates, shapes, queue order) and upload it:
// after this the whole Solve input is resident in HBM.
// Upload a SolveBase once (dict, parsed integers, catalogue SoA + descriptors, templates); later Solves on the same
// catalogues and NodePools point their kernels at this copy.
static int32_t EnsureBaseOnDevice(kp_ctx* ctx, SolveBase& B) {
  if (B.on_device) return KP_OK;
  Compiled view;
  view.B = std::shared_ptr<SolveBase>(&B, [](SolveBase*) {});  // non-owning: PutCatalogs / DevCats read B
  Blob blob;
  B.o_dict = blob.put(&B.d.dd, 1);
  B.o_vint = blob.put(B.d.vint);
  vector<CatOffsets> coffs;
  PutCatalogs(blob, view, coffs);
  B.coffs = coffs;
  B.o_cats = blob.reserve(sizeof(DevCatalog) * coffs.size());
  B.o_treqs = blob.put(B.tmpl_reqs);
  B.o_tts = blob.put(B.tmpl_taintset);
  B.o_tcat = blob.put(B.tmpl_catalog);
  B.o_tX = blob.put(B.tmpl_X);
  B.o_tdm = blob.put(B.tmpl_daemon);
  HIPCHK(B.dev.alloc(blob.total()));
  uint8_t* base = (uint8_t*)B.dev.p;
  vector<DevCatalog> dc = DevCats(base, view, coffs);
  memcpy(blob.host.data() + B.o_cats, dc.data(), sizeof(DevCatalog) * dc.size());
  HIPCHK(hipMemcpyAsync(base, blob.host.data(), blob.host.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  B.on_device = true;
  return KP_OK;
}

// Compile the batch and upload it. The catalogue half (SolveBase: dictionary, catalogue SoA, templates) is taken
// from the ctx cache when the catalogues (identity + seqnum) and NodePools match and the dictionary covers the
// batch; only the per-Solve half (shapes, existing nodes, topology, queue order) is compiled and uploaded.
static int32_t SolvePrepare(kp_ctx* ctx, const kp_solve_in* in, kp_comm* comm, kp_solve_plan** out);
int32_t kp_solve_prepare(kp_ctx* ctx, const kp_solve_in* in, kp_solve_plan** out) {
  return SolvePrepare(ctx, in, nullptr, out);
}
int32_t kp_solve_prepare_comm(kp_ctx* ctx, const kp_solve_in* in, kp_comm* comm, kp_solve_plan** out) {
  if (comm && comm->ctx != ctx) return fail(KP_E_INVAL, "communicator belongs to another context");
  return SolvePrepare(ctx, in, comm, out);
}
static int32_t SolvePrepareLocal(kp_ctx* ctx, const kp_solve_in* in, kp_comm* comm,
                                 std::unique_ptr<kp_solve_plan>& plan, size_t& gather_chunk, size_t& gather_off);
static int32_t SolvePrepare(kp_ctx* ctx, const kp_solve_in* in, kp_comm* comm, kp_solve_plan** out) {
  auto t0 = std::chrono::steady_clock::now();
  if (!ctx || !in || !out) return fail(KP_E_INVAL, "null argument");
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  std::unique_ptr<kp_solve_plan> plan;
  size_t chunk = 0, off = 0;
  int32_t rc = SolvePrepareLocal(ctx, in, comm, plan, chunk, off);
  if (comm && comm->n_ranks > 1) {
    // every rank reaches this exchange, failed or not: (status, table chunk bytes) of each rank; the all-gather of
    // the table follows only when every rank prepared and all agree on its size
    const string err = g_err;
    int64_t mine[2] = {rc, (int64_t)chunk};
    vector<int64_t> all(2 * (size_t)comm->n_ranks);
    int32_t xrc = CommExchange(comm, mine, all.data(), sizeof mine);
    if (xrc) return xrc;
    if (rc) {
      g_err = err;
      return rc;
    }
    for (int i = 0; i < comm->n_ranks; i++) {
      if (all[2 * i]) return fail(KP_E_DEVICE, "rank %d failed to prepare the Solve (error %lld)", i, (long long)all[2 * i]);
      if (all[2 * i + 1] != (int64_t)chunk)
        return fail(KP_E_INVAL, "ranks disagree on the template-options table (%lld vs %zu bytes): every rank must "
                    "pass the same batch", (long long)all[2 * i + 1], chunk);
    }
    if (chunk) {
      uint8_t* tab = (uint8_t*)plan->buf.p + off;
      rc = CommAllGatherDev(comm, tab + chunk * comm->rank, tab, chunk);
      if (rc) return rc;
    }
  } else if (rc) {
    return rc;
  }
  plan->prepare_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = plan.release();
  return KP_OK;
}
// Everything of a prepare that involves only this rank: compile, upload, this rank's rows of the template table.
// gather_chunk > 0: the table rows [rank * chunk, (rank + 1) * chunk) bytes at gather_off still need the all-gather.
static int32_t SolvePrepareLocal(kp_ctx* ctx, const kp_solve_in* in, kp_comm* comm,
                                 std::unique_ptr<kp_solve_plan>& plan, size_t& gather_chunk, size_t& gather_off) {
  gather_chunk = gather_off = 0;
  HIPCHK(hipSetDevice(ctx->device));
  plan = std::make_unique<kp_solve_plan>();
  plan->ctx = ctx;
  plan->cp = std::make_unique<Compiled>();
  Compiled& C = *plan->cp;
  const auto tc0 = std::chrono::steady_clock::now();
  int32_t rc = CompileSolve(in, C, ctx);
  if (rc) return rc;
  plan->compile_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc0).count();
  plan->catalog_ms = C.base_hit ? 0 : C.B->build_ms;
  rc = EnsureBaseOnDevice(ctx, *C.B);
  if (rc) return rc;
  const Dict& d = C.B->d;
  const int TW = C.B->TW, P = (int)in->n_pods, NT = (int)C.B->tmpl_reqs.size();
  const int Pc = std::max(P, 1);
  plan->P = P;
  plan->Pc = Pc;
  plan->max_types = in->max_instance_types;
  for (auto& q : C.B->tmpl_reqs) plan->any_min |= q.hmin != 0;
  for (auto& q : C.shape_reqs) plan->any_min |= q.hmin != 0;

  const uint32_t rmask = RequestedResources(C);
  Blob blob;
  SolveOffs o;
  PutShared(blob, C, o);
  PutArena(blob, C, C.pod_shape, C.queue, Pc, ExStatic(C, rmask), rmask, o);
  const size_t host_bytes = blob.host.size();
  const int opt_stride = in->max_instance_types ? (int)in->max_instance_types : std::max(1, d.dd.T);
  ReserveArenaDev(blob, C, Pc, opt_stride, SortCapacity(C.ov), true, o);
  // template options per (shape-level, template): rows split evenly over the communicator's ranks (padded so that
  // every rank contributes the same byte count to the all-gather)
  const int SLi = (int)C.shape_reqs.size();
  const bool tfeas_on = NT > 0 && SLi > 0 && !(comm ? comm->no_tfeas : ctx->ov.template_table != 0);
  // shard the rows over the ranks only when the table is large enough to repay the all-gather (kp_comm settings)
  const bool shard = tfeas_on && comm && comm->n_ranks > 1 && (uint64_t)SLi * NT >= comm->tfeas_shard_min;
  const int n_ranks = shard ? comm->n_ranks : 1, my_rank = shard ? comm->rank : 0;
  const int tf_words = TW + KP_NRES / 2 + 1;
  const int rows_per_rank = (SLi + n_ranks - 1) / n_ranks;
  const size_t tf_bytes = tfeas_on ? (size_t)rows_per_rank * n_ranks * NT * tf_words * sizeof(uint64_t) : 0;
  o.tfeas = blob.reserve_dev(std::max<size_t>(tf_bytes, 8));
  // the explanation step's outputs: records [SL][NT] and the per-pod row index in one block, then the mark table
  const size_t SLx = std::max(SLi, 1), NTx = std::max(NT, 1);
  const size_t why_rec_bytes = sizeof(ExplainRec) * SLx * NTx;
  plan->n_why = why_rec_bytes + sizeof(int32_t) * (size_t)Pc;
  plan->o_why = blob.reserve_dev(plan->n_why);
  plan->n_mark = SLx;
  plan->o_mark = blob.reserve_dev(plan->n_mark);
  const size_t total_bytes = blob.total();

  // the per-Solve arena: reuse the ctx's spare allocation when it is large enough
  if (ctx->spare && ctx->spare_bytes >= total_bytes) {
    plan->buf.p = ctx->spare;
    plan->buf.n = ctx->spare_bytes;
    ctx->spare = nullptr;
    ctx->spare_bytes = 0;
  } else {
    if (ctx->spare) HIPCHK(hipFree(ctx->spare));
    ctx->spare = nullptr;
    ctx->spare_bytes = 0;
    HIPCHK(plan->buf.alloc(total_bytes));
  }
  uint8_t* base = (uint8_t*)plan->buf.p;
  const size_t n_mut = o.mut_end - o.mut;
  HIPCHK(hipMemcpyAsync(base, blob.host.data(), host_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(base + o.pristine, base + o.mut, n_mut, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));

  SolveArgs& a = plan->a;
  const int res_mode = !C.B->res_cls ? 0 : in->reserved_offering_mode == KP_RESERVED_STRICT ? 2 : 1;
  BindSolve(a, C, o, base, base, P, Pc, rmask, res_mode);
  plan->o_hcnc = o.hcnc;
  plan->n_hcnc = o.n_hcnc;
  plan->o_held = o.held;
  if (tfeas_on) {  // this rank's rows of the template-options table, then one all-gather (RCCL) of every rank's rows
    plan->tf = TfeasOf(a, base, o, SLi, tf_words);
    plan->tfeas_on = true;
    TfeasArgs f = plan->tf;
    f.row_lo = std::min(SLi, my_rank * rows_per_rank);
    f.row_hi = std::min(SLi, (my_rank + 1) * rows_per_rank);
    HIPCHK(launch_tmpl_feas(f, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (shard) {  // the all-gather of every rank's rows follows in SolvePrepare, after the ranks' status exchange
      gather_chunk = (size_t)rows_per_rank * NT * tf_words * sizeof(uint64_t);
      gather_off = o.tfeas;
    }
    a.tfeas = (const uint64_t*)(base + o.tfeas);
    a.tfeas_words = tf_words;
  }

  {
    ExplainArgs& x = plan->ex;
    memset(&x, 0, sizeof x);
    x.dict = a.dict, x.cats = a.cats, x.n_catalogs = a.n_catalogs, x.vint = a.vint;
    x.n_pods = P, x.pod_shape = a.pod_shape, x.pod_level = a.pod_level, x.placement = a.placement;
    x.tmpl_remaining = a.tmpl_remaining, x.tg_cnt = a.tg_cnt, x.tg_reg = a.tg_reg;
    x.n_sl = SLi, x.n_tmpl = NT;
    x.shape_level_base = a.shape_level_base, x.sl_shape = (const int32_t*)(base + o.slsh);
    x.shape_reqs = a.shape_reqs, x.shape_negop = a.shape_negop, x.shape_tolerates = a.shape_tolerates;
    x.shape_requests = a.shape_requests, x.shape_pvp = a.shape_pvp, x.pvp_base = a.pvp_base, x.pvp_slot = a.pvp_slot;
    x.tmpl_reqs = a.tmpl_reqs, x.tmpl_taintset = a.tmpl_taintset, x.tmpl_catalog = a.tmpl_catalog, x.tmpl_X = a.tmpl_X;
    x.tmpl_daemon = a.tmpl_daemon, x.tmpl_limit_present = a.tmpl_limit_present;
    x.sl_own_base = a.sl_own_base, x.sl_own_n = a.sl_own_n, x.own_rec = a.own_rec, x.own_pd = a.own_pd;
    x.sl_topo_keys = a.sl_topo_keys, x.req_res_mask = a.req_res_mask;
    x.rec = (ExplainRec*)(base + plan->o_why);
    x.pod_row = (int32_t*)(base + plan->o_why + why_rec_bytes);
    x.mark = base + plan->o_mark;
    plan->taint_first = TaintFirst(in, C);
  }
  plan->o_ver = o.ver0;
  plan->n_ver = o.ver_end - o.ver0;
  plan->o_fail = o.fail0;
  plan->n_fail = o.fail_end - o.fail0;
  plan->o_mut = o.mut;
  plan->n_mut = n_mut;
  plan->o_pristine = o.pristine;
  plan->o_stats = o.stats;
  plan->o_npods = o.npods;
  plan->o_place = o.place;
  plan->o_events = o.events;
  plan->o_nct = o.nct;
  plan->o_ncrq = o.ncrq;
  plan->o_opts = o.opts;
  plan->o_nrem = o.nrem;
  plan->o_nopt = o.nopt;
  plan->o_ncr = o.ncr;
  plan->opt_stride = opt_stride;
  plan->base_version = C.B->version;
  return KP_OK;
}

// kp_solve_run on a plan whose catalogues changed since its data was derived would place pods on stale offerings
static int32_t SolvePlanStale(const kp_solve_plan* plan) {
  const SolveBase& B = *plan->cp->B;
  if (int32_t rc = CatalogsAlive(B.alive)) return rc;
  if (plan->base_version != B.version || SeqnumsOf(B.catalogs) != B.seqnums)
    return fail(KP_E_INVAL, "stale plan: a catalogue's seqnum changed since it was prepared (kp_solve_refresh)");
  return KP_OK;
}

int32_t kp_solve_refresh(kp_solve_plan* plan) {
  if (!plan) return fail(KP_E_INVAL, "null argument");
  kp_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  SolveBase& B = *plan->cp->B;
  if (int32_t rc = CatalogsAlive(B.alive)) return rc;
  if (SeqnumsOf(B.catalogs) != B.seqnums) {
    int32_t rc = RefreshOfferings(ctx, B);
    if (rc < 0) return rc;
    if (rc > 0)
      return fail(KP_E_INVAL, "the offering update changed which NodePools keep instance types: prepare the Solve again");
  }
  if (plan->base_version != B.version && plan->tfeas_on) {  // the table derives from the templates' options
    HIPCHK(launch_tmpl_feas(plan->tf, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  for (int c = 0; c < KP_MAX_CLASSES; c++) plan->a.res_cap0[c] = B.res_cap0.empty() ? 0 : B.res_cap0[c];
  plan->base_version = B.version;
  return KP_OK;
}

void kp_solve_plan_destroy(kp_solve_plan* p) {
  if (!p) return;
  kp_ctx* ctx = p->ctx;
  {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    if (p->buf.p && p->buf.n >= ctx->spare_bytes) {  // keep the larger arena for the next prepare
      if (ctx->spare) (void)hipFree(ctx->spare);
      ctx->spare = p->buf.p;
      ctx->spare_bytes = p->buf.n;
      p->buf.p = nullptr;
      p->buf.n = 0;
    }
  }
  delete p;  // (after the lock: it may drop the context's last reference)
}

// kp_cancel: one int32 flag in pinned, host-mapped memory (written by the host, polled by solve_kernel)
struct kp_cancel {
  CtxRef ctx;
  int32_t* flag = nullptr;  // hipHostMalloc: coherent, mapped; the same address on the device (unified addressing)
};

int32_t kp_cancel_create(kp_ctx* ctx, kp_cancel** out) {
  if (!ctx || !out) return fail(KP_E_INVAL, "null argument");
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  auto c = std::make_unique<kp_cancel>();
  c->ctx = ctx;
  void* p = nullptr;
  HIPCHK(hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocCoherent));
  c->flag = (int32_t*)p;
  __atomic_store_n(c->flag, 0, __ATOMIC_SEQ_CST);
  *out = c.release();
  return KP_OK;
}
// lock-free: called from another thread while a run holds the context's lock
int32_t kp_cancel_set(kp_cancel* c) {
  if (!c) return fail(KP_E_INVAL, "null argument");
  __atomic_store_n(c->flag, 1, __ATOMIC_SEQ_CST);
  return KP_OK;
}
int32_t kp_cancel_reset(kp_cancel* c) {
  if (!c) return fail(KP_E_INVAL, "null argument");
  __atomic_store_n(c->flag, 0, __ATOMIC_SEQ_CST);
  return KP_OK;
}
void kp_cancel_destroy(kp_cancel* c) {
  if (!c) return;
  {
    std::lock_guard<std::recursive_mutex> lock(c->ctx->mu);  // (no run is reading it once the lock is ours)
    (void)hipSetDevice(c->ctx->device);
    if (c->flag) (void)hipHostFree(c->flag);
  }
  delete c;
}

// FinalizeScheduling: a NodeClaim holding reservations launches only into them (reservation-id In {held ids}; the held
// classes are compatible with its requirements, so the intersection is exactly that set)
static void ApplyHeld(const SolveBase& B, uint64_t held, KReqs& q) {
  if (!held) return;
  const Dict& d = B.d;
  const int k = d.key(kResID);
  for (int wi = 0; wi < nwords(d, k); wi++) q.vals[kw(d, k, wi)] = 0;
  for (uint64_t m = held; m; m &= m - 1) {
    const int bit = B.classes[__builtin_ctzll(m)].rid_bit;
    q.vals[bit / 64] |= 1ull << (bit % 64);
  }
  q.present |= 1ull << k;
  q.compl_ &= ~(1ull << k);
}

// A finished Solve's result sections within its arena (kp_solve_run: the plan's buffer; kp_cluster_drift: the winner's
// arena of a batched launch), their host copies, and the kp_solve_result built from them.
struct ResultOffs {
  size_t place, events, nct, ncrq, opts, nrem, nopt, ncr, held;
};
struct ArenaResult {
  vector<int32_t> place, events, nct;
  vector<int64_t> ncrq;
  vector<uint32_t> opts, nrem, nopt;
  vector<KReqs> fin;
  vector<uint64_t> held;
};
static int32_t FetchArenaResult(hipStream_t st, const uint8_t* base, const ResultOffs& o, int Pc, int opt_stride, bool res_mode,
                                int n_nc, ArenaResult& r) {
  if (n_nc < 0 || n_nc > Pc) return fail(KP_E_DEVICE, "Solve result: %d NodeClaims for %d pods", n_nc, Pc);
  const int nn = std::max(n_nc, 1);
  r.place.resize(Pc), r.events.resize(Pc), r.nct.resize(nn);
  r.ncrq.resize((size_t)nn * KP_NRES);
  r.opts.resize((size_t)nn * opt_stride), r.nrem.resize(nn), r.nopt.resize(nn);
  r.fin.resize(n_nc);
  r.held.assign(res_mode ? n_nc : 0, 0);
  HIPCHK(hipMemcpyAsync(r.place.data(), base + o.place, sizeof(int32_t) * Pc, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(r.events.data(), base + o.events, sizeof(int32_t) * Pc, hipMemcpyDeviceToHost, st));
  if (n_nc) {
    HIPCHK(hipMemcpyAsync(r.nct.data(), base + o.nct, sizeof(int32_t) * n_nc, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(r.ncrq.data(), base + o.ncrq, sizeof(int64_t) * n_nc * KP_NRES, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(r.opts.data(), base + o.opts, sizeof(uint32_t) * (size_t)n_nc * opt_stride, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(r.nrem.data(), base + o.nrem, sizeof(uint32_t) * n_nc, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(r.nopt.data(), base + o.nopt, sizeof(uint32_t) * n_nc, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(r.fin.data(), base + o.ncr, sizeof(KReqs) * n_nc, hipMemcpyDeviceToHost, st));
    if (res_mode) HIPCHK(hipMemcpyAsync(r.held.data(), base + o.held, sizeof(uint64_t) * n_nc, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return KP_OK;
}
// stats: the Solve's stats words ([3] NodeClaims, [4] events); P pods. pod_of(p): the result's index of the Solve's pod
// p; existing_of(pos): the result's index of the existing node at position pos (-1: none). Applies the held
// reservations and Truncate's minValues check (a NodeClaim whose truncated options break minValues fails its pods).
extern "C++" template <class PodOf, class ExistingOf>
static int32_t AssembleResult(const SolveBase& B, const uint64_t* stats, ArenaResult& a, int P, int opt_stride, PodOf pod_of,
                              ExistingOf existing_of, kp_solve_result& res) {
  const Dict& d = B.d;
  const int n_nc = (int)a.fin.size(), n_ev = (int)stats[4];
  if (n_ev < 0 || n_ev > (int)a.events.size()) return fail(KP_E_DEVICE, "Solve result: %d events", n_ev);
  for (int i = 0; i < (int)a.held.size(); i++) ApplyHeld(B, a.held[i], a.fin[i]);
  res.placement.assign(P, -1);
  res.ncs.resize(n_nc);
  for (int i = 0; i < n_ev; i++) {
    const int p = a.events[i];
    if (p < 0 || p >= P) return fail(KP_E_DEVICE, "Solve result: event %d names pod %d of %d", i, p, P);
    const int t = a.place[p];
    if (t >= 0) {
      if (t >= n_nc) return fail(KP_E_DEVICE, "Solve result: pod %d on NodeClaim %d of %d", p, t, n_nc);
      res.ncs[t].pods.push_back((uint32_t)pod_of(p));
      res.placement[pod_of(p)] = t;
    } else if (t <= -2) {
      const int e = existing_of(-2 - t);
      if (e < 0) return fail(KP_E_DEVICE, "Solve result: pod %d on existing position %d", p, -2 - t);
      res.placement[pod_of(p)] = -2 - e;
    }
  }
  res.nc_cat.resize(n_nc);
  for (int i = 0; i < n_nc; i++) {
    if (a.nct[i] < 0 || a.nct[i] >= (int)B.tmpl_catalog.size() || a.nopt[i] > (uint32_t)opt_stride)
      return fail(KP_E_DEVICE, "Solve result: NodeClaim %d template %d, %u options", i, a.nct[i], a.nopt[i]);
    auto& nc = res.ncs[i];
    res.nc_cat[i] = B.tmpl_catalog[a.nct[i]];
    nc.nodepool = (uint32_t)B.tmpl_nodepool[a.nct[i]];
    nc.n_remaining = a.nrem[i];
    memset(&nc.requests, 0, sizeof nc.requests);
    for (int r = 0; r < KP_NRES; r++) {
      nc.requests.milli[r] = a.ncrq[(size_t)i * KP_NRES + r];
      if (nc.requests.milli[r]) nc.requests.present |= 1u << r;
    }
    nc.options.assign(a.opts.begin() + (size_t)i * opt_stride, a.opts.begin() + (size_t)i * opt_stride + a.nopt[i]);
    nc.reqs = DecodeReqs(d, a.fin[i]);
    // Truncate(reqs, max): minValues must still hold on the truncated options, else the pods fail
    if (a.fin[i].hmin & a.fin[i].present) {
      const HostCat& hc = B.cats[B.tmpl_catalog[a.nct[i]]];
      vector<int> ts(nc.options.begin(), nc.options.end());
      if (!HostMinValuesOK(d, hc, a.fin[i], ts)) {
        for (uint32_t p : nc.pods) res.placement[p] = -1;
        nc.options.clear();
      }
    }
  }
  res.fin = a.fin;
  return KP_OK;
}

// One Solve over resident inputs: restore mutable state, solve_kernel, finalize_kernel, copy results.
static int32_t SolveRun(kp_solve_plan* plan, kp_cancel* cancel, bool explain, kp_solve_result** out);
int32_t kp_solve_run(kp_solve_plan* plan, kp_solve_result** out) { return SolveRun(plan, nullptr, false, out); }
int32_t kp_solve_run_cancellable(kp_solve_plan* plan, kp_cancel* cancel, kp_solve_result** out) {
  return SolveRun(plan, cancel, false, out);
}
// The Solve, then the explanation step on the same stream before the copy-back: explain_mark_kernel + explain_kernel read
// the state solve_kernel left (placements, levels, remaining limits, topology counts) and write their own block only
int32_t kp_solve_run_explained(kp_solve_plan* plan, kp_cancel* cancel, kp_solve_result** out) {
  return SolveRun(plan, cancel, true, out);
}

// The explained result's host half: the records and the per-pod rows in one download; the key masks of
// KP_WHY_REQUIREMENTS records resolved to the dictionary's strings (byte order), the taint index from the plan's table
static int32_t FetchReasons(kp_solve_plan* plan, hipStream_t st, kp_solve_result& res) {
  const SolveBase& B = *plan->cp->B;
  const Dict& d = B.d;
  const size_t NT = B.tmpl_nodepool.size(), SL = plan->cp->shape_reqs.size();
  const size_t n_rec = std::max<size_t>(SL, 1) * std::max<size_t>(NT, 1);
  vector<uint8_t> blockv(plan->n_why);
  HIPCHK(hipMemcpyAsync(blockv.data(), (uint8_t*)plan->buf.p + plan->o_why, plan->n_why, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  res.explained = true;
  res.n_tmpl = (int)NT;
  res.why.resize(n_rec);
  memcpy(res.why.data(), blockv.data(), sizeof(ExplainRec) * n_rec);
  res.pod_row.assign(plan->P, -1);
  if (plan->P) memcpy(res.pod_row.data(), blockv.data() + sizeof(ExplainRec) * n_rec, sizeof(int32_t) * plan->P);
  res.why_taint = plan->taint_first;
  for (int np : B.tmpl_nodepool) res.why_nodepool.push_back((uint32_t)np);
  res.key_names = d.keys;
  vector<char> seen(std::max<size_t>(SL, 1), 0);
  for (int p = 0; p < plan->P; p++) {
    const int32_t row = res.pod_row[p];
    if (row < 0) continue;
    if ((size_t)row >= SL) return fail(KP_E_DEVICE, "explanation: pod %d names shape-level %d of %zu", p, row, SL);
    if (seen[row]) continue;
    seen[row] = 1;
    for (size_t t = 0; t < NT; t++) {
      const ExplainRec& r = res.why[(size_t)row * NT + t];
      if (r.code < KP_WHY_NONE || r.code > KP_WHY_MIN_VALUES)
        return fail(KP_E_DEVICE, "explanation: record (%d, %zu) holds code %d", row, t, r.code);
      if (r.code != KP_WHY_REQUIREMENTS) continue;
      vector<int> ks;
      for (uint64_t m = r.keys; m; m &= m - 1) {
        const int k = __builtin_ctzll(m);
        if (k >= (int)res.key_names.size()) return fail(KP_E_DEVICE, "explanation: key %d of %zu", k, res.key_names.size());
        ks.push_back(k);
      }
      std::sort(ks.begin(), ks.end(), [&](int x, int y) { return res.key_names[x] < res.key_names[y]; });
      auto& v = res.why_keys[(size_t)row * NT + t];
      for (int k : ks) v.push_back(res.key_names[k].c_str());
    }
  }
  return KP_OK;
}

static int32_t SolveRun(kp_solve_plan* plan, kp_cancel* cancel, bool explain, kp_solve_result** out) {
  auto t0 = std::chrono::steady_clock::now();
  if (!plan || !out) return fail(KP_E_INVAL, "null argument");
  if (explain && plan->a.res_mode)
    return fail(KP_E_UNSUPPORTED, "explained Solves over capacity reservations are not implemented");
  if (cancel && cancel->ctx.p != plan->ctx.p) return fail(KP_E_INVAL, "the cancel token belongs to another context");
  kp_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  if (int32_t rc = SolvePlanStale(plan)) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  // (a token already set: nothing is queued on the stream)
  if (cancel && __atomic_load_n(cancel->flag, __ATOMIC_SEQ_CST)) return fail(KP_E_CANCELED, "cancelled before the run");
  const Compiled& C = *plan->cp;
  uint8_t* base = (uint8_t*)plan->buf.p;
  const int P = plan->P, Pc = plan->Pc, opt_stride = plan->opt_stride;
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(base + plan->o_mut, base + plan->o_pristine, plan->n_mut, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemsetAsync(base + plan->o_stats, 0, sizeof(uint64_t) * KP_SOLVE_STATS, st));
  HIPCHK(hipMemsetAsync(base + plan->o_npods, 0, sizeof(int32_t) * Pc, st));
  HIPCHK(hipMemsetAsync(base + plan->o_place, 0xFF, sizeof(int32_t) * Pc, st));
  HIPCHK(hipMemsetAsync(base + plan->o_ver, 0, plan->n_ver, st));
  HIPCHK(hipMemsetAsync(base + plan->o_fail, 0xFF, plan->n_fail, st));
  if (plan->n_hcnc) HIPCHK(hipMemsetAsync(base + plan->o_hcnc, 0, plan->n_hcnc, st));
  SolveArgs a = plan->a;
  if (cancel) {
    void* dp = nullptr;
    HIPCHK(hipHostGetDevicePointer(&dp, cancel->flag, 0));
    a.cancel = (const int32_t*)dp;
  }
  const size_t dyn = std::max<size_t>((size_t)2 * a.sort_cap * sizeof(int32_t), a.chk_maxc ? CHK_LDS_BYTES : 0);
  HIPCHK(hipEventRecord(ctx->ev0, st));
  HIPCHK(launch_solve(a, 8, dyn, st));
  HIPCHK(hipEventRecord(ctx->ev1, st));
  uint64_t stats[KP_SOLVE_STATS];
  HIPCHK(hipMemcpyAsync(stats, base + plan->o_stats, sizeof stats, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (stats[7]) return fail(KP_E_DEVICE, "solve_kernel exceeded its Queue.Pop bound (%llu pops): aborted",
                            (unsigned long long)stats[2]);
  if (stats[46]) return fail(KP_E_CANCELED, "Solve cancelled after %llu pops (kp_cancel_set)", (unsigned long long)stats[2]);
  const int n_nc = (int)stats[3];
  FinalizeArgs f;
  f.solve_stats = nullptr;
  f.dict = a.dict;
  f.cats = a.cats;
  f.vint = a.vint;
  f.n_nc = n_nc;
  f.nc_tmpl = a.nc_tmpl;
  f.tmpl_catalog = a.tmpl_catalog;
  f.nc_reqs = a.nc_reqs;
  f.nc_X = a.nc_X;
  f.max_types = (int32_t)plan->max_types;
  f.opt_stride = opt_stride;
  f.out_options = (uint32_t*)(base + plan->o_opts);
  f.out_n_remaining = (uint32_t*)(base + plan->o_nrem);
  f.out_n_options = (uint32_t*)(base + plan->o_nopt);
  f.nc_held = a.res_mode ? a.nc_held : nullptr;
  HIPCHK(hipEventRecord(ctx->ev2, st));
  HIPCHK(launch_finalize(f, st));
  HIPCHK(hipEventRecord(ctx->ev3, st));
  if (explain) {
    HIPCHK(hipMemsetAsync(base + plan->o_mark, 0, plan->n_mark, st));
    HIPCHK(launch_explain(plan->ex, st));
  }

  auto res = std::make_unique<kp_solve_result>();
  ArenaResult ar;
  const ResultOffs ro{plan->o_place, plan->o_events, plan->o_nct, plan->o_ncrq, plan->o_opts, plan->o_nrem, plan->o_nopt,
                      plan->o_ncr, plan->o_held};
  if (int32_t rc = FetchArenaResult(st, base, ro, Pc, opt_stride, a.res_mode != 0, n_nc, ar)) return rc;
  float ms_solve = 0, ms_fin = 0;
  HIPCHK(hipEventElapsedTime(&ms_solve, ctx->ev0, ctx->ev1));
  HIPCHK(hipEventElapsedTime(&ms_fin, ctx->ev2, ctx->ev3));
  // pods are the batch's own indices; an existing position is the input index of its node
  if (int32_t rc = AssembleResult(*C.B, stats, ar, P, opt_stride, [](int p) { return p; },
                                  [&](int pos) { return pos < (int)C.ex_input.size() ? C.ex_input[pos] : -1; }, *res))
    return rc;
  if (explain)
    if (int32_t rc = FetchReasons(plan, st, *res)) return rc;
  memset(&res->stats, 0, sizeof res->stats);
  res->stats.device_ms = ms_solve + ms_fin;
  res->stats.solve_kernel_ms = ms_solve;
  res->stats.finalize_kernel_ms = ms_fin;
  res->stats.attempts = stats[0];
  res->stats.bytes_algorithmic = stats[1];
  res->stats.pops = stats[2];
  res->stats.prepare_ms = plan->prepare_ms;
  res->stats.catalog_ms = plan->catalog_ms;
  res->stats.catalog_cached = plan->cp->base_hit ? 1 : 0;
  res->stats.catalog_refreshed = plan->cp->base_refreshed ? 1 : 0;
  for (int i = 0; i < 8; i++) res->stats.phase_cycles[i] = stats[8 + i];
  res->stats.scanned = stats[5];
  res->stats.cursor_starts = stats[6];
  for (int i = 0; i < 8; i++) res->stats.attempt_cycles[i] = stats[16 + i];
  res->stats.fast_pods = stats[24];
  res->stats.slow_sorts = stats[31];
  for (int i = 0; i < 6; i++) res->stats.fast_cycles[i] = stats[25 + i];
  for (int i = 0; i < 8; i++) res->stats.fast_bails[i] = stats[32 + i];
  res->stats.reserved_offering_errors = stats[40];
  for (int i = 0; i < 5; i++) res->stats.order_chunks[i] = stats[41 + i];
  res->stats.run_length_pods = stats[47];
  res->stats.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = res.release();
  return KP_OK;
}

// Host half of kp_solve_prepare without a device: the Go shim's "can the device path take this batch" probe.
int32_t kp_solve_validate(const kp_solve_in* in) {
  if (!in) return fail(KP_E_INVAL, "null argument");
  Compiled C;
  return CompileSolve(in, C);
}

int32_t kp_solve(kp_ctx* ctx, const kp_solve_in* in, kp_solve_result** out) { return kp_solve_cancellable(ctx, in, nullptr, out); }

int32_t kp_solve_cancellable(kp_ctx* ctx, const kp_solve_in* in, kp_cancel* cancel, kp_solve_result** out) {
  kp_solve_plan* plan = nullptr;
  int32_t rc = kp_solve_prepare(ctx, in, &plan);
  if (rc) return rc;
  rc = kp_solve_run_cancellable(plan, cancel, out);
  kp_solve_plan_destroy(plan);
  return rc;
}
int32_t kp_solve_explained(kp_ctx* ctx, const kp_solve_in* in, kp_cancel* cancel, kp_solve_result** out) {
  kp_solve_plan* plan = nullptr;
  int32_t rc = kp_solve_prepare(ctx, in, &plan);
  if (rc) return rc;
  rc = kp_solve_run_explained(plan, cancel, out);
  kp_solve_plan_destroy(plan);
  return rc;
}
int32_t kp_result_explained(const kp_solve_result* r) { return r && r->explained ? 1 : 0; }
uint32_t kp_result_reason_count(const kp_solve_result* r, uint32_t pod) {
  if (!r || !r->explained || pod >= r->pod_row.size() || r->pod_row[pod] < 0) return 0;
  return (uint32_t)r->n_tmpl;
}
int32_t kp_result_pod_reasons(const kp_solve_result* r, uint32_t pod, kp_pool_reason* out, uint32_t n) {
  if (!r || (!out && n)) return fail(KP_E_INVAL, "null argument");
  if (!r->explained) return fail(KP_E_INVAL, "the result was not explained (kp_solve_run_explained)");
  if (pod >= r->pod_row.size()) return fail(KP_E_INVAL, "pod %u of %zu", pod, r->pod_row.size());
  const int row = r->pod_row[pod];
  const uint32_t cnt = row < 0 ? 0 : std::min<uint32_t>(n, (uint32_t)r->n_tmpl);
  for (uint32_t t = 0; t < cnt; t++) {
    const size_t i = (size_t)row * r->n_tmpl + t;
    const ExplainRec& x = r->why[i];
    kp_pool_reason& o = out[t];
    memset(&o, 0, sizeof o);
    o.nodepool = r->why_nodepool[t];
    o.code = x.code;
    o.taint = x.code == KP_WHY_TAINT ? r->why_taint[i] : -1;
    o.n_types = (uint32_t)x.n_types;
    o.n_requirements = (uint32_t)x.n_req, o.n_fits = (uint32_t)x.n_fits, o.n_offering = (uint32_t)x.n_off;
    o.n_requirements_fits = (uint32_t)x.n_rf, o.n_requirements_offering = (uint32_t)x.n_ro;
    o.n_fits_offering = (uint32_t)x.n_fo, o.n_remaining = (uint32_t)x.n_remaining;
    auto it = r->why_keys.find(i);
    if (it != r->why_keys.end()) {
      o.n_keys = (uint32_t)it->second.size();
      o.keys = it->second.data();
    }
  }
  return KP_OK;
}

uint32_t kp_result_nodeclaim_count(const kp_solve_result* r) { return r ? (uint32_t)r->ncs.size() : 0; }
int32_t kp_result_pod_placements(const kp_solve_result* r, int32_t* out, uint32_t n) {
  if (!r || !out || n != r->placement.size()) return fail(KP_E_INVAL, "bad placement buffer");
  memcpy(out, r->placement.data(), sizeof(int32_t) * n);
  return KP_OK;
}
int32_t kp_result_nodeclaim(const kp_solve_result* r, uint32_t i, kp_nodeclaim_info* out) {
  if (!r || !out || i >= r->ncs.size()) return fail(KP_E_INVAL, "bad nodeclaim index");
  const auto& n = r->ncs[i];
  out->nodepool = n.nodepool;
  out->n_pods = (uint32_t)n.pods.size();
  out->n_remaining = n.n_remaining;
  out->n_options = (uint32_t)n.options.size();
  out->pods = n.pods.data();
  out->options = n.options.data();
  out->requests = n.requests;
  out->requirements.items = n.reqs ? n.reqs->items.data() : nullptr;
  out->requirements.n = n.reqs ? (uint32_t)n.reqs->items.size() : 0;
  out->requirements.reserved_ = 0;
  return KP_OK;
}
int32_t kp_result_stats(const kp_solve_result* r, kp_solve_stats* out) {
  if (!r || !out) return fail(KP_E_INVAL, "null");
  *out = r->stats;
  return KP_OK;
}
void kp_result_destroy(kp_solve_result* r) { delete r; }

// CompatibleAvailableFilter batched on the GPU.
}  // extern "C"

namespace {
// Dictionary + catalogue SoA for a batch of query rows against ONE catalogue (CompatibleAvailableFilter rows,
// launch requests): the catalogue's labels and offerings plus the rows' requirements, compiled rows in qreqs.
int32_t CompileQueries(const kp_catalog* cat, const vector<RawReqs>& qs, Compiled& cp, vector<KReqs>& qreqs) {
  DictBuilder db;
  for (auto& t : cat->types) {
    db.addReqs(t.reqs);
    for (auto& o : t.offs) {
      db.addLabel(kCapType, o.ct);
      db.addLabel(kZone, o.zone);
      if (o.has_zid) db.addLabel(kZoneID, o.zid);
      if (o.has_rid) db.addLabel(kResID, o.rid);
      if (o.has_rt) db.addLabel(kResType, o.rt);
    }
  }
  db.bounded[kResID];
  db.bounded[kResType];
  for (auto& q : qs) db.addReqs(q);
  int32_t rc = db.build(cp.B->d);
  if (rc) return rc;
  const int T = (int)cat->types.size(), TW = std::max(1, (T + 63) / 64);
  cp.B->d.dd.T = T;
  cp.B->d.dd.TW = TW;
  cp.B->TW = TW;  // FillOfferings (kp_*_refresh) lays the offering masks out with it
  map<ClassKey, int> classes;
  const Dict& d = cp.B->d;
  for (auto& t : cat->types)
    for (auto& o : t.offs) {
      const ClassKey ck = ClassOf(d, o);
      if (!classes.count(ck)) {
        int id = (int)classes.size();
        classes[ck] = id;
      }
    }
  if (classes.size() > KP_MAX_CLASSES) return fail(KP_E_UNSUPPORTED, "%zu offering classes", classes.size());
  cp.B->C = (int)classes.size();
  cp.B->d.dd.C = cp.B->C;
  cp.B->classes.resize(cp.B->C);
  for (auto& kv : classes) cp.B->classes[kv.second] = ClassOfKey(kv.first);
  cp.B->cats.resize(1);
  rc = CompileCatalog(d, cat->types, TW, classes, cp.B->cats[0]);
  if (rc) return rc;
  uint64_t catalog_keys = 0;
  for (int k = 0; k < d.dd.K; k++)
    for (int t = 0; t < T; t++)
      if (!((cp.B->cats[0].NOKEY[(size_t)k * TW + t / 64] >> (t % 64)) & 1)) catalog_keys |= 1ull << k;
  cp.B->d.dd.catalog_keys = catalog_keys;
  cp.B->d.dd.single_valued = catalog_keys & ~cp.B->cats[0].multi_valued;
  qreqs.assign(std::max<size_t>(qs.size(), 1), KReqs{});
  for (size_t i = 0; i < qs.size(); i++) qreqs[i] = Compile(d, qs[i]);
  return KP_OK;
}

}  // namespace

// Shared by kp_filter_refresh / kp_launch_refresh: rebuild the offering section of a plan's compiled catalogue
// from the catalogue's current offerings (class ids as compiled) and copy it over the resident arrays.
static int32_t RefreshOfferings(kp_ctx* ctx, const kp_catalog* cat, Compiled& cp, const CatOffsets& coff, uint8_t* base) {
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  map<ClassKey, int> classes;
  for (int c = 0; c < cp.B->C; c++) classes[KeyOfClass(cp.B->classes[c])] = c;
  HostCat hc;  // filled aside: the plan's host copy changes only once the device copy did
  hc.T = cp.B->cats[0].T;
  hc.S = cp.B->cats[0].S;
  try {
    FillOfferings(cp.B->d, cat->types, cp.B->TW, classes, hc);
  } catch (const std::out_of_range&) {
    return fail(KP_E_INVAL, "refresh: an offering outside the plan's offering classes");
  }
  HIPCHK(hipMemcpyAsync(base + coff.offer, hc.offer_avail.data(), hc.offer_avail.size() * sizeof(uint64_t),
                        hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(base + coff.price, hc.price.data(), hc.price.size() * sizeof(double),
                        hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(base + coff.price_cm, hc.price_cm.data(), hc.price_cm.size() * sizeof(double),
                        hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(base + coff.price_sub, hc.price_sub.data(), hc.price_sub.size() * sizeof(double),
                        hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HostCat& dst = cp.B->cats[0];
  dst.offer_avail.swap(hc.offer_avail);
  dst.price.swap(hc.price);
  dst.price_cm.swap(hc.price_cm);
  dst.price_sub.swap(hc.price_sub);
  return KP_OK;
}

struct kp_filter_plan {
  CtxRef ctx;
  DevBuf buf;
  FeasArgs fa;
  uint32_t n_queries = 0;
  int T = 0;
  size_t tiles = 0, o_mask = 0, o_ch = 0, o_cls = 0;
  bool compact = false;  // KP_FILTER_COMPACT: classes per row instead of the cheapest-price rows
  int ch_stride = 0;  // doubles per device cheapest-price row (whole 128-byte lines; the caller's rows are T long)
  bool cheapest = false;
  double prepare_ms = 0;
  const kp_catalog* cat = nullptr;  // kp_filter_refresh: catalogue, compiled form and its offering offsets
  std::shared_ptr<bool> alive;      // cat's alive token: run / refresh after kp_catalog_destroy return KP_E_INVAL
  uint64_t seqnum = 0;              // catalogue seqnum the resident offerings reflect
  Compiled cp;
  CatOffsets coff{};
};

extern "C" {

// Compile the query rows against the catalogue dictionary and upload rows + catalogue SoA (resident).
int32_t kp_filter_prepare(kp_ctx* ctx, const kp_catalog* cat, const kp_feasibility_query* queries, uint32_t n_queries,
                          int32_t with_cheapest, kp_filter_plan** out) {
  auto t0 = std::chrono::steady_clock::now();
  if (!ctx || !cat || (!queries && n_queries) || !out) return fail(KP_E_INVAL, "null argument");
  if (with_cheapest < KP_FILTER_MASK_ONLY || with_cheapest > KP_FILTER_COMPACT)
    return fail(KP_E_INVAL, "with_cheapest %d", with_cheapest);
  const bool compact = with_cheapest == KP_FILTER_COMPACT;
  if (compact) with_cheapest = 0;  // (no price rows: the classes and the resident class prices instead)
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  auto plan = std::make_unique<kp_filter_plan>();
  plan->ctx = ctx;
  plan->compact = compact;
  Compiled cp;
  vector<RawReqs> qs(n_queries);
  for (uint32_t i = 0; i < n_queries; i++) qs[i] = ParseReqs(queries[i].requirements);
  vector<KReqs> qreqs;
  int32_t rc = CompileQueries(cat, qs, cp, qreqs);
  if (rc) return rc;
  const int T = (int)cat->types.size();
  vector<int64_t> qrq((size_t)std::max<uint32_t>(n_queries, 1) * KP_NRES, 0);
  for (uint32_t i = 0; i < n_queries; i++)
    for (int r = 0; r < KP_NRES; r++)
      qrq[(size_t)i * KP_NRES + r] = (queries[i].requests.present >> r) & 1 ? queries[i].requests.milli[r] : 0;
  Blob blob;
  const size_t o_dict = blob.put(&cp.B->d.dd, 1);
  const size_t o_vint = blob.put(cp.B->d.vint);
  vector<CatOffsets> coffs;
  PutCatalogs(blob, cp, coffs);
  const size_t o_cats = blob.reserve(sizeof(DevCatalog));
  const size_t o_q = blob.put(qreqs);
  const size_t o_qr = blob.put(qrq);
  const size_t host_bytes = blob.host.size();
  const size_t tiles = (size_t)(T + 63) / 64;
  plan->o_mask = blob.reserve(sizeof(uint64_t) * std::max<size_t>(1, n_queries * tiles));
  plan->ch_stride = (T + 15) & ~15;
  plan->o_ch = with_cheapest ? blob.reserve(sizeof(double) * std::max<size_t>(1, (size_t)n_queries * plan->ch_stride)) : 0;
  plan->o_cls = compact ? blob.reserve(sizeof(uint64_t) * std::max<size_t>(1, n_queries)) : 0;
  HIPCHK(hipMalloc(&plan->buf.p, blob.host.size()));
  uint8_t* base = (uint8_t*)plan->buf.p;
  vector<DevCatalog> dc = DevCats(base, cp, coffs);
  memcpy(blob.host.data() + o_cats, dc.data(), sizeof(DevCatalog));
  HIPCHK(hipMemcpyAsync(base, blob.host.data(), host_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  FeasArgs& fa = plan->fa;
  fa.dict = (const DevDict*)(base + o_dict);
  fa.cat = (const DevCatalog*)(base + o_cats);
  fa.vint = (const int64_t*)(base + o_vint);
  fa.T = T;
  fa.n_queries = (int32_t)n_queries;
  fa.mode_compatible = 1;
  fa.pad_ = 0;
  fa.q_reqs = base + o_q;
  fa.q_requests = (const int64_t*)(base + o_qr);
  fa.out_mask = (uint64_t*)(base + plan->o_mask);
  fa.out_cheapest = with_cheapest ? (double*)(base + plan->o_ch) : nullptr;
  fa.out_classes = compact ? (uint64_t*)(base + plan->o_cls) : nullptr;
  fa.ch_stride = plan->ch_stride;
  // the bitset kernel (KP_FEAS_GLOBAL: the per-type global-gather kernel, kept as its cross-check)
  const kp_overrides& ov = plan->ctx->ov;
  fa.bits = ov.feasibility_kernel == 1 ? 0 : 1;
  fa.blocks = (int32_t)std::min<uint32_t>(std::max<uint32_t>((n_queries + 7) / 8, 1), 8192);
  if (ov.feasibility_blocks > 0) fa.blocks = std::min(65535, ov.feasibility_blocks);  // measurement knob
  fa.pad_ = ov.feasibility_temporal ? 0 : 1;  // bit 0: the cheapest-price stream as non-temporal stores
  fa.one_row = ov.feasibility_kernel == 2 ? 1 : 0;  // cross-check: the one-row-per-wave kernel at any catalogue size
  plan->n_queries = n_queries;
  plan->T = T;
  plan->tiles = tiles;
  plan->cheapest = with_cheapest != 0;
  plan->cat = cat;
  plan->alive = cat->alive;
  plan->seqnum = cat->seqnum;
  plan->coff = coffs[0];
  plan->cp = std::move(cp);
  plan->prepare_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = plan.release();
  return KP_OK;
}

// One launch over the resident rows. Results are copied out only into the non-NULL buffers.
int32_t kp_filter_run(kp_filter_plan* plan, uint64_t* out_mask, double* out_cheapest, kp_solve_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  if (!plan) return fail(KP_E_INVAL, "null argument");
  if (out_cheapest && !plan->cheapest) return fail(KP_E_INVAL, "plan was prepared without cheapest prices");
  kp_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  if (int32_t rc = CatalogsAlive({plan->alive})) return rc;
  if (plan->cat->seqnum != plan->seqnum)  // R:instancetype.go:225-237: a changed seqnum invalidates the offerings
    return fail(KP_E_INVAL, "stale plan: catalogue seqnum %llu, plan built at %llu (kp_filter_refresh)",
                (unsigned long long)plan->cat->seqnum, (unsigned long long)plan->seqnum);
  HIPCHK(hipSetDevice(ctx->device));
  uint8_t* base = (uint8_t*)plan->buf.p;
  const uint32_t n = plan->n_queries;
  HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
  if (n) HIPCHK(launch_feasibility(plan->fa, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
  if (n && out_mask)
    HIPCHK(hipMemcpyAsync(out_mask, base + plan->o_mask, sizeof(uint64_t) * n * plan->tiles, hipMemcpyDeviceToHost, ctx->stream));
  if (n && out_cheapest)
    HIPCHK(hipMemcpy2DAsync(out_cheapest, sizeof(double) * plan->T, base + plan->o_ch, sizeof(double) * plan->ch_stride,
                            sizeof(double) * plan->T, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->device_ms = ms;
    stats->attempts = (uint64_t)n * plan->T;  // (row, type) pairs evaluated
    // the kernel launch_feasibility chose (kp_abi.h): 1 per-type, 2 bits, 3 quad with copy wave, 4 quad all-eval
    const FeasArgs& fa = plan->fa;
    stats->phase_cycles[0] = !n ? 0 : !fa.bits ? 1 : (fa.T > 1024 || fa.one_row) ? 2 : fa.out_cheapest ? 3 : 4;
    stats->prepare_ms = plan->prepare_ms;
    stats->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return KP_OK;
}

// The compact result: the same launch, the rows' class sets copied out instead of the price rows.
int32_t kp_filter_run_compact(kp_filter_plan* plan, uint64_t* out_mask, uint64_t* out_classes, kp_solve_stats* stats) {
  if (!plan) return fail(KP_E_INVAL, "null argument");
  if (out_classes && !plan->compact) return fail(KP_E_INVAL, "plan was not prepared with KP_FILTER_COMPACT");
  int32_t rc = kp_filter_run(plan, out_mask, nullptr, stats);
  if (rc || !out_classes || !plan->n_queries) return rc;
  kp_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(out_classes, (uint8_t*)plan->buf.p + plan->o_cls, sizeof(uint64_t) * plan->n_queries,
                        hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KP_OK;
}

// The per-(class, type) cheapest available offering prices the compact result indexes (class-major, +inf: none),
// as the plan's resident catalogue holds them (kp_filter_refresh keeps them current).
int32_t kp_filter_class_prices(kp_filter_plan* plan, double* out, uint32_t capacity, uint32_t* n_classes) {
  if (!plan || !n_classes) return fail(KP_E_INVAL, "null argument");
  std::lock_guard<std::recursive_mutex> lock(plan->ctx->mu);
  if (int32_t rc = CatalogsAlive({plan->alive})) return rc;
  if (plan->cat->seqnum != plan->seqnum)  // (a consumer caches the table per seqnum: never hand out the old prices)
    return fail(KP_E_INVAL, "stale plan: catalogue seqnum %llu, plan built at %llu (kp_filter_refresh)",
                (unsigned long long)plan->cat->seqnum, (unsigned long long)plan->seqnum);
  const HostCat& hc = plan->cp.B->cats[0];
  const int C = plan->cp.B->C, T = plan->T;
  *n_classes = (uint32_t)C;
  if (!out) return KP_OK;
  if ((size_t)capacity < (size_t)C * T) return fail(KP_E_INVAL, "capacity %u < %d classes x %d types", capacity, C, T);
  for (int c = 0; c < C; c++)
    for (int t = 0; t < T; t++) out[(size_t)c * T + t] = hc.price_cm[(size_t)c * hc.S + t];
  return KP_OK;
}

// ICE refresh of a prepared plan: FillOfferings over the catalogue's current offerings with the plan's own class
// ids, then only the offering arrays are copied over their resident copies.
int32_t kp_filter_refresh(kp_filter_plan* plan, const kp_catalog* cat) {
  if (!plan || !cat) return fail(KP_E_INVAL, "null argument");
  if (int32_t rc = CatalogsAlive({plan->alive})) return rc;
  if (cat != plan->cat || (int)cat->types.size() != plan->T)
    return fail(KP_E_INVAL, "kp_filter_refresh: the plan was prepared on another catalogue");
  const int32_t rc = RefreshOfferings(plan->ctx, cat, plan->cp, plan->coff, (uint8_t*)plan->buf.p);
  if (rc == KP_OK) plan->seqnum = cat->seqnum;
  return rc;
}

void kp_filter_plan_destroy(kp_filter_plan* p) {
  if (!p) return;
  (void)hipSetDevice(p->ctx->device);
  delete p;
}

int32_t kp_filter_compatible_available(kp_ctx* ctx, const kp_catalog* cat, const kp_feasibility_query* queries,
                                       uint32_t n_queries, uint64_t* out_mask, double* out_cheapest,
                                       kp_solve_stats* stats) {
  if (!out_mask) return fail(KP_E_INVAL, "null argument");
  kp_filter_plan* plan = nullptr;
  int32_t rc = kp_filter_prepare(ctx, cat, queries, n_queries, out_cheapest != nullptr, &plan);
  if (rc) return rc;
  rc = kp_filter_run(plan, out_mask, out_cheapest, stats);
  kp_filter_plan_destroy(plan);
  return rc;
}

// ---- launch-side selection (instance.DefaultProvider.Create), batched over NodeClaims -----------------
}  // extern "C"

// Launch-side reservation tables per (type, class): the cheapest offering at any availability (CapacityBlockFilter
// reads unavailable offerings too, R:filter.go:177-189) and the greatest ReservationCapacity over the available
// offerings (ReservedOfferingFilter, R:filter.go:247-251).
static void FillReservationTables(const Dict& d, const vector<HostType>& types, const map<ClassKey, int>& cls_id, int C,
                                  vector<double>& price_all, vector<int32_t>& rcap) {
  const size_t T = types.size();
  price_all.assign(std::max<size_t>(T * C, 1), std::numeric_limits<double>::infinity());
  rcap.assign(std::max<size_t>(T * C, 1), INT32_MIN);
  for (size_t t = 0; t < T; t++)
    for (auto& o : types[t].offs) {
      const int c = cls_id.at(ClassOf(d, o));
      double& p = price_all[t * C + c];
      if (o.price < p) p = o.price;
      if (o.available) rcap[t * C + c] = std::max(rcap[t * C + c], o.rcap);
    }
}

struct LtState;  // kp_launch_templates (below)
struct kp_launch_plan {
  CtxRef ctx;
  DevBuf buf;
  LaunchArgs la;
  uint32_t n = 0, max_types = 0, ovr_stride = 0;
  size_t o_out = 0, o_types = 0, o_ovr = 0, o_stats = 0, o_pall = 0, o_rcap = 0;
  double prepare_ms = 0;
  const kp_catalog* cat = nullptr;  // kp_launch_refresh
  std::shared_ptr<bool> alive;      // cat's alive token (as kp_filter_plan)
  uint64_t seqnum = 0;              // catalogue seqnum the resident offerings reflect
  int T = 0;
  Compiled cp;
  CatOffsets coff{};
  // kp_launch_run_templates: which requests list vpc.amazonaws.com/efa, the distinct types the requests list, and the
  // state its first call builds
  vector<uint8_t> req_efa;
  vector<uint32_t> used;
  std::shared_ptr<LtState> lt;
};
static_assert(sizeof(LaunchOut) == sizeof(kp_launch_result), "LaunchOut mirrors kp_launch_result");

extern "C" {

int32_t kp_launch_prepare(kp_ctx* ctx, const kp_catalog* cat, const kp_launch_request* reqs, uint32_t n,
                          const char* const* subnet_zones, uint32_t n_subnet_zones, uint32_t max_types,
                          kp_launch_plan** out) {
  auto t0 = std::chrono::steady_clock::now();
  if (!ctx || !cat || (!reqs && n) || !out || (!subnet_zones && n_subnet_zones)) return fail(KP_E_INVAL, "null argument");
  if (max_types == 0 || max_types > LAUNCH_CAP) return fail(KP_E_INVAL, "max_types %u not in [1, %d]", max_types, LAUNCH_CAP);
  if (n_subnet_zones > 255) return fail(KP_E_UNSUPPORTED, "%u subnet zones", n_subnet_zones);
  const int T = (int)cat->types.size();
  for (auto& t : cat->types) {
    // overrides per type <= subnet zones: one offering per (capacity type, zone), except reserved ones, which the
    // ReservedOfferingFilter narrows to one per zone (then one per (zone, reservation) keeps classes single)
    std::set<std::tuple<string, string, string, string>> seen;
    for (auto& o : t.offs) {
      const bool res = o.ct == "reserved";
      if (o.has_zone && !seen.insert({o.ct, o.zone, res ? o.rid : "", res ? o.rt : ""}).second)
        return fail(KP_E_UNSUPPORTED, "%s: two %s offerings in zone %s", t.name.c_str(), o.ct.c_str(), o.zone.c_str());
    }
  }
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  auto plan = std::make_unique<kp_launch_plan>();
  plan->ctx = ctx;
  Compiled cp;
  vector<RawReqs> qs(n);
  vector<uint32_t> off(n + 1, 0), list;
  for (uint32_t i = 0; i < n; i++) {
    qs[i] = ParseReqs(reqs[i].requirements);
    if (reqs[i].n_instance_types > LAUNCH_CAP)
      return fail(KP_E_UNSUPPORTED, "request %u: %u instance types", i, reqs[i].n_instance_types);
    if (reqs[i].n_instance_types && !reqs[i].instance_types) return fail(KP_E_INVAL, "request %u: null list", i);
    for (uint32_t j = 0; j < reqs[i].n_instance_types; j++) {
      if (reqs[i].instance_types[j] >= (uint32_t)T) return fail(KP_E_INVAL, "request %u: type %u", i, reqs[i].instance_types[j]);
      list.push_back(reqs[i].instance_types[j]);
    }
    off[i + 1] = (uint32_t)list.size();
  }
  if (T > 4096) return fail(KP_E_UNSUPPORTED, "%d instance types", T);
  vector<KReqs> qreqs;
  int32_t rc = CompileQueries(cat, qs, cp, qreqs);
  if (rc) return rc;
  const Dict& d = cp.B->d;
  const int TW = cp.B->d.dd.TW, C = cp.B->C;
  vector<int64_t> qrq((size_t)std::max<uint32_t>(n, 1) * KP_NRES, 0);
  for (uint32_t i = 0; i < n; i++)
    for (int r = 0; r < KP_NRES; r++)
      qrq[(size_t)i * KP_NRES + r] = (reqs[i].requests.present >> r) & 1 ? reqs[i].requests.milli[r] : 0;
  // ExoticInstanceTypeFilter's predicate (R:filter.go:295-310): a metal size or accelerator capacity
  vector<uint64_t> exotic(TW, 0);
  const string kSize = "karpenter.k8s.aws/instance-size";
  for (int t = 0; t < T; t++) {
    const HostType& ht = cat->types[t];
    bool exo = false;
    for (auto& r : ht.reqs)
      if (r.key == kSize && r.op == KP_OP_IN)
        for (auto& v : r.values)
          if (v.find("metal") != string::npos) exo = true;
    for (int r : {KP_RES_NEURON, KP_RES_NEURONCORE, KP_RES_AMD_GPU, KP_RES_NVIDIA_GPU, KP_RES_GAUDI})
      if (((ht.cap_present >> r) & 1) && ht.cap[r] != 0) exo = true;
    if (exo) exotic[t / 64] |= 1ull << (t % 64);
  }
  // offering classes in each type's offering order; class -> subnet zone; capacity-type class masks
  int MO = 1;
  for (auto& t : cat->types) MO = std::max(MO, (int)t.offs.size() + 1);
  vector<uint8_t> ofs_cls((size_t)T * MO, 0xFF);
  const int kct = d.key(kCapType), kz = d.key(kZone);
  std::map<ClassKey, int> cls_id;
  for (int c = 0; c < C; c++) cls_id[KeyOfClass(cp.B->classes[c])] = c;
  for (int t = 0; t < T; t++) {
    int j = 0;
    for (auto& o : cat->types[t].offs) ofs_cls[(size_t)t * MO + j++] = (uint8_t)cls_id.at(ClassOf(d, o));
  }
  const int spot_bit = kct >= 0 ? d.bit(kct, "spot") : -1, od_bit = kct >= 0 ? d.bit(kct, "on-demand") : -1;
  const int res_bit = kct >= 0 ? d.bit(kct, "reserved") : -1, krt = d.key(kResType);
  const int rt0_bit = krt >= 0 ? d.bit(krt, "default") : -1, rt1_bit = krt >= 0 ? d.bit(krt, "capacity-block") : -1;
  uint64_t cls_res = 0, cls_rt0 = 0, cls_rt1 = 0;
  for (int c = 0; c < C; c++) {
    const OfferClass& oc = cp.B->classes[c];
    if (res_bit >= 0 && oc.ct_bit == res_bit) cls_res |= 1ull << c;
    if (rt0_bit >= 0 && oc.rt_bit == rt0_bit) cls_rt0 |= 1ull << c;
    if (rt1_bit >= 0 && oc.rt_bit == rt1_bit) cls_rt1 |= 1ull << c;
  }
  vector<double> price_all;
  vector<int32_t> rcap;
  FillReservationTables(d, cat->types, cls_id, C, price_all, rcap);
  uint64_t cls_spot = 0, cls_od = 0;
  vector<int8_t> cls_zone(std::max(C, 1), -1);
  for (int c = 0; c < C; c++) {
    if (spot_bit >= 0 && cp.B->classes[c].ct_bit == spot_bit) cls_spot |= 1ull << c;
    if (od_bit >= 0 && cp.B->classes[c].ct_bit == od_bit) cls_od |= 1ull << c;
    for (uint32_t z = 0; z < n_subnet_zones; z++)
      if (kz >= 0 && cp.B->classes[c].zone_bit >= 0 && subnet_zones[z] && d.bit(kz, subnet_zones[z]) == cp.B->classes[c].zone_bit) {
        cls_zone[c] = (int8_t)z;
        break;
      }
  }
  Blob blob;
  const size_t o_dict = blob.put(&cp.B->d.dd, 1);
  const size_t o_vint = blob.put(cp.B->d.vint);
  vector<CatOffsets> coffs;
  PutCatalogs(blob, cp, coffs);
  const size_t o_cats = blob.reserve(sizeof(DevCatalog));
  const size_t o_q = blob.put(qreqs);
  const size_t o_qr = blob.put(qrq);
  const size_t o_off = blob.put(off);
  if (list.empty()) list.push_back(0);
  const size_t o_list = blob.put(list);
  const size_t o_exo = blob.put(exotic);
  const size_t o_cz = blob.put(cls_zone);
  const size_t o_oc = blob.put(ofs_cls);
  plan->o_pall = blob.put(price_all);
  plan->o_rcap = blob.put(rcap);
  const size_t host_bytes = blob.host.size();
  const uint32_t ovr_stride = std::max<uint32_t>(1, max_types * std::max<uint32_t>(1, n_subnet_zones));
  plan->o_out = blob.reserve(sizeof(kp_launch_result) * std::max<uint32_t>(n, 1));
  plan->o_types = blob.reserve(sizeof(uint32_t) * (size_t)std::max<uint32_t>(n, 1) * max_types);
  plan->o_ovr = blob.reserve(sizeof(uint32_t) * (size_t)std::max<uint32_t>(n, 1) * ovr_stride);
  plan->o_stats = blob.reserve(sizeof(uint64_t) * 2);
  HIPCHK(hipMalloc(&plan->buf.p, blob.host.size()));
  uint8_t* base = (uint8_t*)plan->buf.p;
  vector<DevCatalog> dc = DevCats(base, cp, coffs);
  memcpy(blob.host.data() + o_cats, dc.data(), sizeof(DevCatalog));
  HIPCHK(hipMemcpyAsync(base, blob.host.data(), host_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  LaunchArgs& la = plan->la;
  memset(&la, 0, sizeof la);
  la.dict = (const DevDict*)(base + o_dict);
  la.cat = (const DevCatalog*)(base + o_cats);
  la.vint = (const int64_t*)(base + o_vint);
  la.n = (int32_t)n;
  la.max_types = (int32_t)max_types;
  la.spot_bit = spot_bit;
  la.od_bit = od_bit;
  la.ct_key = kct;
  la.MO = MO;
  la.cls_spot = cls_spot;
  la.cls_od = cls_od;
  la.res_bit = res_bit;
  la.cls_res = cls_res;
  la.cls_rt0 = cls_rt0;
  la.cls_rt1 = cls_rt1;
  la.price_all = (const double*)(base + plan->o_pall);
  la.rcap = (const int32_t*)(base + plan->o_rcap);
  la.q_reqs = base + o_q;
  la.q_requests = (const int64_t*)(base + o_qr);
  la.list_off = (const uint32_t*)(base + o_off);
  la.list = (const uint32_t*)(base + o_list);
  la.exotic = (const uint64_t*)(base + o_exo);
  la.cls_zone = (const int8_t*)(base + o_cz);
  la.ofs_cls = base + o_oc;
  la.ovr_stride = ovr_stride;
  la.out = (LaunchOut*)(base + plan->o_out);
  la.out_types = (uint32_t*)(base + plan->o_types);
  la.out_overrides = (uint32_t*)(base + plan->o_ovr);
  la.stats = (uint64_t*)(base + plan->o_stats);
  plan->n = n;
  plan->max_types = max_types;
  plan->ovr_stride = ovr_stride;
  plan->req_efa.resize(n);
  for (uint32_t i = 0; i < n; i++) plan->req_efa[i] = (reqs[i].requests.present >> KP_RES_EFA) & 1;
  {
    vector<uint8_t> listed(std::max(T, 1), 0);
    for (uint32_t j = 0; j < off[n]; j++) listed[list[j]] = 1;
    for (int t = 0; t < T; t++)
      if (listed[t]) plan->used.push_back((uint32_t)t);
  }
  plan->cat = cat;
  plan->alive = cat->alive;
  plan->seqnum = cat->seqnum;
  plan->T = T;
  plan->coff = coffs[0];
  plan->cp = std::move(cp);
  plan->prepare_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = plan.release();
  return KP_OK;
}

// One launch over the resident requests; results copied only into the non-NULL buffers (out_types:
// [n][max_types], out_overrides: [n][max_types * n_subnet_zones]).
int32_t kp_launch_run(kp_launch_plan* plan, kp_launch_result* out, uint32_t* out_types, uint32_t* out_overrides,
                      kp_solve_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  if (!plan) return fail(KP_E_INVAL, "null argument");
  kp_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  if (int32_t rc = CatalogsAlive({plan->alive})) return rc;
  if (plan->cat->seqnum != plan->seqnum)
    return fail(KP_E_INVAL, "stale plan: catalogue seqnum %llu, plan built at %llu (kp_launch_refresh)",
                (unsigned long long)plan->cat->seqnum, (unsigned long long)plan->seqnum);
  HIPCHK(hipSetDevice(ctx->device));
  uint8_t* base = (uint8_t*)plan->buf.p;
  const uint32_t n = plan->n;
  HIPCHK(hipMemsetAsync(base + plan->o_stats, 0, sizeof(uint64_t) * 2, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
  if (n) HIPCHK(launch_launch(plan->la, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
  uint64_t st[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(st, base + plan->o_stats, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
  if (n && out) HIPCHK(hipMemcpyAsync(out, base + plan->o_out, sizeof(kp_launch_result) * n, hipMemcpyDeviceToHost, ctx->stream));
  if (n && out_types)
    HIPCHK(hipMemcpyAsync(out_types, base + plan->o_types, sizeof(uint32_t) * (size_t)n * plan->max_types,
                          hipMemcpyDeviceToHost, ctx->stream));
  if (n && out_overrides)
    HIPCHK(hipMemcpyAsync(out_overrides, base + plan->o_ovr, sizeof(uint32_t) * (size_t)n * plan->ovr_stride,
                          hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->device_ms = ms;
    stats->attempts = st[0];           // (request, listed type) pairs evaluated
    stats->bytes_algorithmic = st[1];
    stats->prepare_ms = plan->prepare_ms;
    stats->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return KP_OK;
}

// ICE refresh of a prepared launch plan (same offering section as kp_filter_refresh; the offering -> class map and
// the subnet-zone classes do not change with availability or price).
int32_t kp_launch_refresh(kp_launch_plan* plan, const kp_catalog* cat) {
  if (!plan || !cat) return fail(KP_E_INVAL, "null argument");
  if (int32_t rc = CatalogsAlive({plan->alive})) return rc;
  if (cat != plan->cat || (int)cat->types.size() != plan->T)
    return fail(KP_E_INVAL, "kp_launch_refresh: the plan was prepared on another catalogue");
  int32_t rc = RefreshOfferings(plan->ctx, cat, plan->cp, plan->coff, (uint8_t*)plan->buf.p);
  if (rc != KP_OK) return rc;
  {  // the reservation tables follow availability and price too
    std::lock_guard<std::recursive_mutex> lock(plan->ctx->mu);
    map<ClassKey, int> cls_id;
    for (int c = 0; c < plan->cp.B->C; c++) cls_id[KeyOfClass(plan->cp.B->classes[c])] = c;
    vector<double> price_all;
    vector<int32_t> rcap;
    FillReservationTables(plan->cp.B->d, cat->types, cls_id, plan->cp.B->C, price_all, rcap);
    uint8_t* base = (uint8_t*)plan->buf.p;
    HIPCHK(hipMemcpyAsync(base + plan->o_pall, price_all.data(), price_all.size() * sizeof(double),
                          hipMemcpyHostToDevice, plan->ctx->stream));
    HIPCHK(hipMemcpyAsync(base + plan->o_rcap, rcap.data(), rcap.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                          plan->ctx->stream));
    HIPCHK(hipStreamSynchronize(plan->ctx->stream));
  }
  plan->seqnum = cat->seqnum;
  return KP_OK;
}

void kp_launch_plan_destroy(kp_launch_plan* p) {
  if (!p) return;
  (void)hipSetDevice(p->ctx->device);
  delete p;
}

int32_t kp_launch_select(kp_ctx* ctx, const kp_catalog* cat, const kp_launch_request* reqs, uint32_t n,
                         const char* const* subnet_zones, uint32_t n_subnet_zones, uint32_t max_types,
                         kp_launch_result* out, uint32_t* out_types, uint32_t* out_overrides, kp_solve_stats* stats) {
  if (!out) return fail(KP_E_INVAL, "null argument");
  kp_launch_plan* plan = nullptr;
  int32_t rc = kp_launch_prepare(ctx, cat, reqs, n, subnet_zones, n_subnet_zones, max_types, &plan);
  if (rc) return rc;
  rc = kp_launch_run(plan, out, out_types, out_overrides, stats);
  kp_launch_plan_destroy(plan);
  return rc;
}

// ---- consolidation: cluster snapshot + batched simulations -----------------------------------------
}  // extern "C"

// Owned deep copy of a kp_cluster (strings and nested arrays), kept by a cluster plan whose simulations run as
// whole Solves (the general path): the caller's buffers are not retained past kp_cluster_prepare.
struct OwnedCluster {
  std::deque<string> strs;
  vector<std::unique_ptr<uint8_t[]>> blocks;
  kp_cluster cl;
  vector<const kp_catalog*> cats;
  vector<std::shared_ptr<bool>> alive;
  const char* S(const char* x) {
    if (!x) return nullptr;
    strs.emplace_back(x);
    return strs.back().c_str();
  }
  template <class T>
  T* A(const T* src, size_t n) {
    if (!src || !n) return nullptr;
    blocks.emplace_back(new uint8_t[sizeof(T) * n]);
    T* d = reinterpret_cast<T*>(blocks.back().get());
    memcpy((void*)d, (const void*)src, sizeof(T) * n);
    return d;
  }
  void Reqs(kp_requirements& r) {
    kp_requirement* it = A(r.items, r.n);
    for (uint32_t i = 0; it && i < r.n; i++) {
      it[i].key = S(it[i].key);
      const char** v = (const char**)A(it[i].values, it[i].n_values);
      for (uint32_t j = 0; v && j < it[i].n_values; j++) v[j] = S(v[j]);
      it[i].values = v;
    }
    r.items = it;
  }
  const kp_label* Labels(const kp_label* l, uint32_t n) {
    kp_label* o = A(l, n);
    for (uint32_t i = 0; o && i < n; i++) o[i].key = S(o[i].key), o[i].value = S(o[i].value);
    return o;
  }
  const kp_taint* Taints(const kp_taint* t, uint32_t n) {
    kp_taint* o = A(t, n);
    for (uint32_t i = 0; o && i < n; i++) o[i].key = S(o[i].key), o[i].value = S(o[i].value);
    return o;
  }
  const kp_host_port* Ports(const kp_host_port* h, uint32_t n) {
    kp_host_port* o = A(h, n);
    for (uint32_t i = 0; o && i < n; i++) o[i].ip = S(o[i].ip);
    return o;
  }
  void Selector(kp_label_selector& s) {
    s.match_labels = Labels(s.match_labels, s.n_match_labels);
    kp_selector_requirement* e = A(s.match_expressions, s.n_match_expressions);
    for (uint32_t i = 0; e && i < s.n_match_expressions; i++) {
      e[i].key = S(e[i].key);
      const char** v = (const char**)A(e[i].values, e[i].n_values);
      for (uint32_t j = 0; v && j < e[i].n_values; j++) v[j] = S(v[j]);
      e[i].values = v;
    }
    s.match_expressions = e;
  }
  const kp_pod_affinity_term* Terms(const kp_pod_affinity_term* t, uint32_t n) {
    kp_pod_affinity_term* o = A(t, n);
    for (uint32_t i = 0; o && i < n; i++) {
      o[i].topology_key = S(o[i].topology_key);
      Selector(o[i].selector);
      Selector(o[i].namespace_selector);
      const char** v = (const char**)A(o[i].namespaces, o[i].n_namespaces);
      for (uint32_t j = 0; v && j < o[i].n_namespaces; j++) v[j] = S(v[j]);
      o[i].namespaces = v;
    }
    return o;
  }
  void Node(kp_existing_node& n) {
    n.name = S(n.name);
    n.labels = Labels(n.labels, n.n_labels);
    n.taints = Taints(n.taints, n.n_taints);
    n.host_ports = Ports(n.host_ports, n.n_host_ports);
  }
  explicit OwnedCluster(const kp_cluster* in) {
    cl = *in;
    cats.assign(in->catalogs, in->catalogs + in->n_catalogs);
    for (auto* c : cats) alive.push_back(c->alive);
    cl.catalogs = cats.data();
    cl.catalog_descs = nullptr;
    kp_nodepool* np = A(in->nodepools, in->n_nodepools);
    for (uint32_t i = 0; np && i < in->n_nodepools; i++) {
      np[i].name = S(np[i].name);
      Reqs(np[i].requirements);
      np[i].labels = Labels(np[i].labels, np[i].n_labels);
      np[i].taints = Taints(np[i].taints, np[i].n_taints);
    }
    cl.nodepools = np;
    kp_cluster_node* nd = A(in->nodes, in->n_nodes);
    for (uint32_t i = 0; nd && i < in->n_nodes; i++) {
      Node(nd[i].node);
      nd[i].pods = A(nd[i].pods, nd[i].n_pods);
    }
    cl.nodes = nd;
    kp_pod_shape* sh = A(in->shapes, in->n_shapes);
    for (uint32_t i = 0; sh && i < in->n_shapes; i++) {
      kp_pod_shape& x = sh[i];
      x.node_selector = Labels(x.node_selector, x.n_node_selector);
      kp_requirements* rt = A(x.required_terms, x.n_required_terms);
      for (uint32_t j = 0; rt && j < x.n_required_terms; j++) Reqs(rt[j]);
      x.required_terms = rt;
      kp_preferred_term* pt = A(x.preferred_terms, x.n_preferred_terms);
      for (uint32_t j = 0; pt && j < x.n_preferred_terms; j++) Reqs(pt[j].preference);
      x.preferred_terms = pt;
      kp_toleration* tl = A(x.tolerations, x.n_tolerations);
      for (uint32_t j = 0; tl && j < x.n_tolerations; j++) tl[j].key = S(tl[j].key), tl[j].value = S(tl[j].value);
      x.tolerations = tl;
      kp_topology_spread* ts = A(x.topology_spread, x.n_topology_spread);
      for (uint32_t j = 0; ts && j < x.n_topology_spread; j++) {
        ts[j].topology_key = S(ts[j].topology_key);
        Selector(ts[j].selector);
      }
      x.topology_spread = ts;
      x.namespace_ = S(x.namespace_);
      x.labels = Labels(x.labels, x.n_labels);
      x.host_ports = Ports(x.host_ports, x.n_host_ports);
      kp_requirements vr{x.volume_requirements, x.n_volume_requirements, 0};
      Reqs(vr);
      x.volume_requirements = vr.items;
      x.required_anti_affinity = Terms(x.required_anti_affinity, x.n_required_anti_affinity);
      x.preferred_anti_affinity = Terms(x.preferred_anti_affinity, x.n_preferred_anti_affinity);
      x.required_affinity = Terms(x.required_affinity, x.n_required_affinity);
      x.preferred_affinity = Terms(x.preferred_affinity, x.n_preferred_affinity);
    }
    cl.shapes = sh;
    kp_pod* pods = A(in->pods, in->n_pods);
    if (in->pod_uids && pods) {  // each subset's Solve sees the pods' exact UID ranks as their keys
      vector<uint64_t> k;
      if (ExactUidKeys(in->pod_uids, in->n_pods, k))
        for (uint32_t i = 0; i < in->n_pods; i++) pods[i].uid_key = k[i];
    }
    cl.pods = pods;
    cl.pod_uids = nullptr;
    cl.pending_pods = A(in->pending_pods, in->n_pending);
    kp_namespace* ns = A(in->namespaces, in->n_namespaces);
    for (uint32_t i = 0; ns && i < in->n_namespaces; i++) ns[i].name = S(ns[i].name), ns[i].labels = Labels(ns[i].labels, ns[i].n_labels);
    cl.namespaces = ns;
  }
};

// kp_cluster_candidates: what the call compiles from the snapshot on its first use and keeps resident (the nodes' pod
// CSR, the pods' shapes, the nodes' name ranks and static reason bits, the shapes' label bitsets and namespace ids), the
// dictionaries a call's PDB selectors are compiled against, and the buffer its per-call arrays and results live in.
struct CandState {
  DevBuf buf;
  CandArgs a{};                                   // the resident half of the kernel arguments
  std::unordered_map<string, uint32_t> atom_id;   // "P" key NUL value: a label pair of some shape; "K" key: a label key
  std::unordered_map<string, uint32_t> ns_id;     // the shapes' namespaces
  DevBuf call;
  size_t call_bytes = 0;
};

struct DriftState;
struct InterruptState;
struct GeneralBatch;
struct kp_cluster_plan {
  CtxRef ctx;
  std::unique_ptr<OwnedCluster> general;  // set: simulations run as whole Solves (kp_solve on this device)
  // a plan of the batched simulation kernel keeps the cluster too: kp_cluster_drift runs whole Solves on any plan (its
  // superset Solve `gb` is built on the first drift call); kp_cluster_simulate never reads it
  std::unique_ptr<OwnedCluster> owned;
  const OwnedCluster* cluster() const { return general ? general.get() : owned.get(); }
  double general_ms = 0;                 // device time of the last general batch (solve + finalize kernels)
  uint64_t general_phase[8] = {};         // kp_overrides.timing: the batch's solve_kernel phase cycles, summed
  std::shared_ptr<GeneralBatch> gb;       // the general path's superset Solve (batched simulations), once built
  vector<std::map<string, string>> general_labels;
  bool gb_tried = false;
  uint32_t general_batched = 0;           // simulations of the last general batch that ran batched
  uint64_t sim_waves[2] = {0, 0};         // the last batched sweep: wave slots launched, most subsets any wave ran
  vector<uint32_t> cmd_live;              // kp_cluster_command without budgets: the identity list its launch walks
  std::unique_ptr<Compiled> cp;
  DevBuf buf;                       // resident snapshot
  DevBuf scratch;                   // per-wave state, grown on demand
  size_t scratch_bytes = 0;
  DevBuf batch;                     // subsets + results, grown on demand
  size_t batch_bytes = 0;
  SimArgs a;
  int N = 0, T2 = 1, n_cu = 256;
  vector<uint32_t> node_npods;
  vector<uint8_t> deleting;         // [N] MarkedForDeletion
  int n_base = 0;                   // pending + deleting-node pods in every simulation
  double prepare_ms = 0;
  // kp_cluster_refresh: where the offering-dependent parts live in the snapshot, and what they derive from
  vector<CatOffsets> coffs;
  size_t o_tX = 0, o_nprice = 0, o_nflags = 0;
  struct NodeOffer {
    uint32_t cat, type;
    std::map<string, string> labels;  // the capacity-type / zone / zone-id labels (NodeCandidatePrice)
  };
  vector<NodeOffer> node_offer;
  vector<uint8_t> node_flags;
  // disruption budgets: the NodePool each node's karpenter.sh/nodepool label names (0xFFFF: none), derived at prepare
  vector<uint16_t> node_pool;
  const uint16_t* d_node_pool = nullptr;  // its resident copy (batched path)
  uint32_t n_pools = 0;
  std::unique_ptr<CandState> cand;        // kp_cluster_candidates, built on its first call
  std::shared_ptr<DriftState> drift;      // kp_cluster_detect_drift, built on its first call
  std::shared_ptr<InterruptState> interrupt;  // kp_cluster_interruptions, built on its first call
};

// kp_*_budgeted: the caller's allowed[] and the count of subsets it blocked
struct BudgetGate {
  const uint32_t* allowed;
  uint32_t n_allowed;
  uint64_t blocked = 0;
};

namespace {
static_assert(sizeof(SimOut) == sizeof(kp_sim_result), "SimOut mirrors kp_sim_result");

// Offerings.Compatible(NewLabelRequirements(node labels)).Cheapest().Price: an offering's capacity-type /
// zone / zone-id requirement (all well-known) is compatible unless the node carries that label with a
// different value.
bool NodeCandidatePrice(const HostType& t, const std::map<string, string>& labels, double* price) {
  bool any = false;
  double p = 0;
  auto clash = [&](const char* key, bool has, const string& v) {
    if (!has) return false;
    auto f = labels.find(key);
    return f != labels.end() && f->second != v;
  };
  // the reservation keys: an offering without one requires DoesNotExist (R:offering.go:136-137), so a node labelled
  // with a reservation id / type is compatible only with the offerings of that reservation
  auto clash_res = [&](const char* key, bool has, const string& v) {
    auto f = labels.find(key);
    if (f == labels.end()) return false;
    return !has || f->second != v;
  };
  for (auto& o : t.offs) {
    if (clash(kCapType, true, o.ct) || clash(kZone, o.has_zone, o.zone) || clash(kZoneID, o.has_zid, o.zid)) continue;
    if (clash_res(kResID, o.has_rid, o.rid) || clash_res(kResType, o.has_rt, o.rt)) continue;
    if (!any || o.price < p) p = o.price;
    any = true;
  }
  *price = p;
  return any;
}

// The per-node NodePool table of a cluster plan (disruption budgets count a subset's members per owning NodePool)
void FillNodePools(const kp_cluster* cl, kp_cluster_plan* plan) {
  std::unordered_map<string, uint32_t> idx;
  for (uint32_t i = 0; i < cl->n_nodepools; i++) idx.emplace(cl->nodepools[i].name ? cl->nodepools[i].name : "", i);
  plan->n_pools = cl->n_nodepools;
  plan->node_pool.assign(std::max<uint32_t>(cl->n_nodes, 1), 0xFFFF);
  for (uint32_t i = 0; i < cl->n_nodes; i++) {
    const kp_existing_node& n = cl->nodes[i].node;
    for (uint32_t j = 0; j < n.n_labels; j++) {
      if (!n.labels[j].key || Normalize(n.labels[j].key) != kNodePool) continue;
      auto f = idx.find(n.labels[j].value ? n.labels[j].value : "");
      if (f != idx.end() && f->second < 0xFFFF) plan->node_pool[i] = (uint16_t)f->second;
    }
  }
}
// Budget arguments against the plan (kp_*_budgeted)
int32_t CheckBudget(const kp_cluster_plan* plan, const BudgetGate* bg) {
  if (!bg->allowed) return fail(KP_E_INVAL, "null allowed");
  if (bg->n_allowed != plan->n_pools)
    return fail(KP_E_INVAL, "n_allowed %u, the cluster has %u NodePools", bg->n_allowed, plan->n_pools);
  if (plan->n_pools > GATE_MAX_POOLS)
    return fail(KP_E_UNSUPPORTED, "disruption budgets over %u NodePools (max %d)", plan->n_pools, GATE_MAX_POOLS);
  return KP_OK;
}
}  // namespace

extern "C" {

static int32_t GeneralBatchBuild(kp_cluster_plan* plan, std::shared_ptr<GeneralBatch>& out);
// A cluster plan for the general path: the cluster is kept as an owned copy and compiled as the batched simulations'
// superset Solve (or, where that does not apply, validated by a host compile: every node existing, every pod pending).
static int32_t PrepareGeneral(kp_ctx* ctx, const kp_cluster* cl, kp_cluster_plan** out,
                              std::chrono::steady_clock::time_point t0) {
  for (uint32_t i = 0; i < cl->n_catalogs; i++)
    if (!cl->catalogs || !cl->catalogs[i]) return fail(KP_E_INVAL, "catalogue %u is null", i);
  vector<kp_existing_node> ex(cl->n_nodes);
  for (uint32_t i = 0; i < cl->n_nodes; i++) ex[i] = cl->nodes[i].node;
  kp_solve_in in;
  memset(&in, 0, sizeof in);
  in.catalogs = cl->catalogs;
  in.n_catalogs = cl->n_catalogs;
  in.n_nodepools = cl->n_nodepools;
  in.nodepools = cl->nodepools;
  in.existing = ex.data();
  in.n_existing = cl->n_nodes;
  in.n_shapes = cl->n_shapes;
  in.shapes = cl->shapes;
  in.pods = cl->pods;
  in.n_pods = cl->n_pods;
  in.max_instance_types = 100;
  in.namespaces = cl->namespaces;
  in.n_namespaces = cl->n_namespaces;
  in.pod_uids = cl->pod_uids;
  PhaseTimer pt;
  auto plan = std::make_unique<kp_cluster_plan>();
  plan->ctx = ctx;
  plan->N = (int)cl->n_nodes;
  FillNodePools(cl, plan.get());
  plan->general = std::make_unique<OwnedCluster>(cl);
  pt.lap("general: owned copy");
  // the superset Solve of the batched simulations, built now (it validates every node and pod as well); a cluster
  // it does not take keeps the per-subset compile, validated here by the whole-cluster compile
  int32_t rc = KP_E_UNSUPPORTED;
  if (ctx->ov.general_batch == 0) {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    plan->gb_tried = true;
    rc = GeneralBatchBuild(plan.get(), plan->gb);
    // the batched layout is an optimisation: a device that cannot hold it leaves the per-subset compile
    if (rc == KP_E_NOMEM || rc == KP_E_DEVICE) (void)hipGetLastError(), rc = KP_E_UNSUPPORTED;
    if (rc && rc != KP_E_UNSUPPORTED) return rc;
    if (rc) plan->gb.reset();
  }
  if (rc) {
    Compiled C;
    rc = CompileSolve(&in, C);
    if (rc) return rc;
  }
  plan->prepare_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = plan.release();
  return KP_OK;
}

int32_t kp_cluster_prepare(kp_ctx* ctx, const kp_cluster* cl, kp_cluster_plan** out) {
  auto t0 = std::chrono::steady_clock::now();
  if (!ctx || !cl || !out) return fail(KP_E_INVAL, "null argument");
  if (cl->n_nodes && !cl->nodes) return fail(KP_E_INVAL, "null nodes");
  if (cl->pod_uids)  // one rule on every path (batched kernels, general batch, per-subset compile): as kp_solve
    for (uint32_t i = 0; i < cl->n_pods; i++)
      if (!cl->pod_uids[i]) return fail(KP_E_INVAL, "null pod uid");
  // capacity reservations: SimulateScheduling's Solve reserves offerings strictly (DisableReservedCapacityFallback),
  // which the batched kernels do not model: such clusters take the general path (whole device Solves)
  bool topo = false;
  for (uint32_t i = 0; i < cl->n_catalogs; i++)
    topo |= cl->catalogs && cl->catalogs[i] && cl->catalogs[i]->reservations;
  for (uint32_t i = 0; i < cl->n_shapes; i++)
    topo |= cl->shapes[i].n_topology_spread > 0 || PodTermCount(cl->shapes[i]) > 0;
  {  // a pod requirement on kubernetes.io/hostname (the batched kernels' node compatibility drops the hostname)
    std::set<string> named;
    for (uint32_t i = 0; i < cl->n_shapes && !topo; i++) {
      const kp_pod_shape& sh = cl->shapes[i];
      for (uint32_t j = 0; j < sh.n_node_selector; j++)
        topo |= sh.node_selector[j].key && string(sh.node_selector[j].key) == kHostname;
      for (uint32_t j = 0; j < sh.n_required_terms; j++) HostnameNames(sh.required_terms[j], &topo, &named);
      for (uint32_t j = 0; j < sh.n_preferred_terms; j++) HostnameNames(sh.preferred_terms[j].preference, &topo, &named);
      HostnameNames(kp_requirements{sh.volume_requirements, sh.n_volume_requirements, 0}, &topo, &named);
    }
  }
  if (topo) return PrepareGeneral(ctx, cl, out, t0);
  for (uint32_t i = 0; i < cl->n_catalogs; i++)
    if (!cl->catalogs || !cl->catalogs[i]) return fail(KP_E_INVAL, "catalogue %u is null", i);
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  // the owned copy kp_cluster_drift compiles its Solves from: it reads the caller's buffers only (null-tolerant, as on
  // the general path, where it is made before any validation), so it is made on a thread of its own while the snapshot
  // is compiled, built and uploaded; every return below joins it
  struct OwnedCopy {
    std::unique_ptr<OwnedCluster> oc;
    bool failed = false;  // the copy threw (out of memory): reported after the join, nothing crosses the thread
    std::thread th;
    ~OwnedCopy() {
      if (th.joinable()) th.join();
    }
  } owned_copy;
  owned_copy.th = std::thread([&owned_copy, cl] {
    try {
      owned_copy.oc = std::make_unique<OwnedCluster>(cl);
    } catch (...) {
      owned_copy.failed = true;
    }
  });
  auto plan = std::make_unique<kp_cluster_plan>();
  plan->ctx = ctx;
  plan->cp = std::make_unique<Compiled>();
  Compiled& C = *plan->cp;
  const int N = (int)cl->n_nodes;
  plan->N = N;
  FillNodePools(cl, plan.get());
  vector<kp_existing_node> ex(N);
  for (int i = 0; i < N; i++) ex[i] = cl->nodes[i].node;
  kp_solve_in in;
  memset(&in, 0, sizeof in);
  in.catalogs = cl->catalogs;
  in.n_catalogs = cl->n_catalogs;
  in.n_nodepools = cl->n_nodepools;
  in.nodepools = cl->nodepools;
  in.existing = ex.data();
  in.n_existing = (uint32_t)N;
  in.n_shapes = cl->n_shapes;
  in.shapes = cl->shapes;
  in.pods = cl->pods;
  in.n_pods = cl->n_pods;
  in.max_instance_types = 100;
  in.namespaces = cl->namespaces;
  in.n_namespaces = cl->n_namespaces;
  in.pod_uids = cl->pod_uids;
  int32_t rc = CompileSolve(&in, C);
  if (rc) return rc;
  const Dict& d = C.B->d;
  const int TW = C.B->TW, E = N, EW = (E + 63) / 64, SL = (int)C.shape_reqs.size(), NT = (int)C.B->tmpl_reqs.size();
  const int T = d.dd.T, K = d.dd.K;
  // a pod NotIn/DoesNotExist on a key some node lacks would add that key to the node's requirements
  uint64_t all_nodes_keys = ~0ull;
  for (auto& q : C.ex_reqs) all_nodes_keys &= q.present;
  for (int sl = 0; sl < SL; sl++)
    if (C.shape_negop[sl] & ~all_nodes_keys)  // CanAdd is then not a function of the snapshot: whole Solves
      return PrepareGeneral(ctx, cl, out, t0);
  // existing nodes: label value bit per key (node labels are single-valued In requirements)
  vector<uint16_t> ex_code((size_t)std::max(K, 1) * std::max(E, 1), 0xFFFF);
  vector<uint8_t> ex_init(std::max(E, 1), 0);
  vector<int32_t> node_pos(std::max(N, 1), 0);
  for (int e = 0; e < E; e++) {
    const KReqs& q = C.ex_reqs[e];
    node_pos[C.ex_input[e]] = e;
    ex_init[e] = cl->nodes[C.ex_input[e]].node.initialized ? 1 : 0;
    for (int k = 0; k < K; k++) {
      if (!((q.present >> k) & 1)) continue;
      for (int wi = 0; wi < nwords(d, k); wi++) {
        const int w = kw(d, k, wi);
        if (q.vals[w]) {
          ex_code[(size_t)k * E + e] = (uint16_t)(w * 64 + __builtin_ctzll(q.vals[w]));
          break;
        }
      }
    }
  }
  // pods: global queue rank
  const uint32_t P = cl->n_pods;
  vector<uint32_t> rank(std::max<uint32_t>(P, 1)), rank_pod(std::max<uint32_t>(P, 1));
  for (uint32_t i = 0; i < P; i++) {
    rank[C.queue[i]] = i;
    rank_pod[i] = (uint32_t)C.queue[i];
  }
  // cluster nodes: pods (CSR), candidate price, flags, type-name ids
  std::unordered_map<string, uint32_t> names;
  auto name_id = [&](const string& s) {
    auto it = names.find(s);
    if (it != names.end()) return it->second;
    const uint32_t id = (uint32_t)names.size();
    names[s] = id;
    return id;
  };
  vector<uint32_t> node_off(N + 1, 0), node_pods;
  vector<double> node_price(std::max(N, 1), 0);
  vector<uint8_t> node_flags(std::max(N, 1), 0);
  vector<uint32_t> node_name(std::max(N, 1), 0);
  plan->node_npods.resize(N);
  for (int i = 0; i < N; i++) {
    const kp_cluster_node& n = cl->nodes[i];
    if (n.catalog >= cl->n_catalogs || !cl->catalogs[n.catalog]) return fail(KP_E_INVAL, "node %d: catalogue %u", i, n.catalog);
    const kp_catalog* cat = cl->catalogs[n.catalog];
    if (n.instance_type >= cat->types.size()) return fail(KP_E_INVAL, "node %d: instance type %u", i, n.instance_type);
    if (n.n_pods && !n.pods) return fail(KP_E_INVAL, "node %d: null pods", i);
    for (uint32_t j = 0; j < n.n_pods; j++) {
      if (n.pods[j] >= P) return fail(KP_E_INVAL, "node %d: pod %u", i, n.pods[j]);
      node_pods.push_back(n.pods[j]);
    }
    node_off[i + 1] = (uint32_t)node_pods.size();
    plan->node_npods[i] = n.n_pods;
    std::map<string, string> labels;
    for (uint32_t j = 0; j < n.node.n_labels; j++)
      labels[Normalize(n.node.labels[j].key ? n.node.labels[j].key : "")] = n.node.labels[j].value ? n.node.labels[j].value : "";
    const HostType& ht = cat->types[n.instance_type];
    double pr = 0;
    const bool priced = NodeCandidatePrice(ht, labels, &pr);
    node_price[i] = pr;
    auto ct = labels.find(kCapType);
    node_flags[i] = (priced ? 1 : 0) | (ct != labels.end() && ct->second == "spot" ? 2 : 0);
    node_name[i] = name_id(ht.name);
    kp_cluster_plan::NodeOffer no{n.catalog, n.instance_type, {}};
    for (const char* k : {kCapType, kZone, kZoneID}) {
      auto f = labels.find(k);
      if (f != labels.end()) no.labels[k] = f->second;
    }
    plan->node_offer.push_back(std::move(no));
  }
  if (node_pods.empty()) node_pods.push_back(0);
  // pods every simulation schedules besides those of S (SimulateScheduling: pending pods and the pods of nodes
  // already being deleted), and the deleting nodes, which are never destinations
  if (cl->n_pending && !cl->pending_pods) return fail(KP_E_INVAL, "null pending_pods");
  vector<uint8_t> pod_kind(std::max<uint32_t>(P, 1), 0);
  vector<uint32_t> base_keys;
  vector<uint64_t> base_excl(std::max(EW, 1), 0);
  plan->deleting.assign(N, 0);
  for (uint32_t j = 0; j < cl->n_pending; j++) {
    const uint32_t p = cl->pending_pods[j];
    if (p >= P) return fail(KP_E_INVAL, "pending pod %u", p);
    if (pod_kind[p]) return fail(KP_E_INVAL, "pod %u listed twice", p);
    pod_kind[p] = 2;
    base_keys.push_back(rank[p]);
  }
  for (int i = 0; i < N; i++) {
    if (!cl->nodes[i].deleting) continue;
    plan->deleting[i] = 1;
    const int e = node_pos[i];
    base_excl[e >> 6] |= 1ull << (e & 63);
    for (uint32_t j = node_off[i]; j < node_off[i + 1]; j++) {
      if (pod_kind[node_pods[j]]) return fail(KP_E_INVAL, "pod %u listed twice", node_pods[j]);
      pod_kind[node_pods[j]] = 1;
      base_keys.push_back(rank[node_pods[j]]);
    }
  }
  plan->n_base = (int)base_keys.size();
  if (base_keys.empty()) base_keys.push_back(0);
  vector<uint32_t> type_name((size_t)cl->n_catalogs * std::max(T, 1), 0xFFFFFFFFu);
  for (uint32_t c = 0; c < cl->n_catalogs; c++)
    for (size_t t = 0; t < cl->catalogs[c]->types.size(); t++)
      type_name[(size_t)c * T + t] = name_id(cl->catalogs[c]->types[t].name);
  vector<int32_t> sl_shape(std::max(SL, 1), 0);
  for (uint32_t s = 0; s < cl->n_shapes; s++)
    for (int l = 0; l < C.shape_nlevels[s]; l++) sl_shape[C.shape_level_base[s] + l] = (int32_t)s;
  const int ctk = d.key(kCapType);

  Blob blob;
  const size_t o_dict = blob.put(&C.B->d.dd, 1);
  const size_t o_vint = blob.put(C.B->d.vint);
  vector<CatOffsets> coffs;
  PutCatalogs(blob, C, coffs);
  const size_t o_cats = blob.reserve(sizeof(DevCatalog) * coffs.size());
  const size_t o_slb = blob.put(C.shape_level_base);
  const size_t o_snl = blob.put(C.shape_nlevels);
  const size_t o_sls = blob.put(sl_shape);
  const size_t o_sreqs = blob.put(C.shape_reqs);
  const size_t o_sneg = blob.put(C.shape_negop);
  const size_t o_sreq = blob.put(C.shape_requests);
  const size_t o_stol = blob.put(C.shape_tolerates);
  const size_t o_pvp = blob.put(C.pvp);
  const size_t o_pvpb = blob.put(C.pvp_base);
  const size_t o_pvps = blob.put(C.pvp_slot);
  vector<int32_t> tmpl_np(C.B->tmpl_nodepool.begin(), C.B->tmpl_nodepool.end());
  if (tmpl_np.empty()) tmpl_np.push_back(0);
  const size_t o_treqs = blob.put(C.B->tmpl_reqs);
  const size_t o_tts = blob.put(C.B->tmpl_taintset);
  const size_t o_tcat = blob.put(C.B->tmpl_catalog);
  const size_t o_tnp = blob.put(tmpl_np);
  const size_t o_tX = blob.put(C.B->tmpl_X);
  const size_t o_tdm = blob.put(C.B->tmpl_daemon);
  const size_t o_excode = blob.put(ex_code);
  const size_t o_exts = blob.put(C.ex_taintset);
  const size_t o_exav = blob.put(C.ex_available);
  const size_t o_exrq = blob.put(C.ex_requests);
  const size_t o_exin = blob.put(ex_init);
  const size_t o_pshape = blob.put(C.pod_shape);
  const size_t o_prank = blob.put(rank);
  const size_t o_rpod = blob.put(rank_pod);
  const size_t o_npos = blob.put(node_pos);
  const size_t o_noff = blob.put(node_off);
  const size_t o_npods = blob.put(node_pods);
  const size_t o_nprice = blob.put(node_price);
  const size_t o_nflags = blob.put(node_flags);
  const size_t o_nname = blob.put(node_name);
  const size_t o_tname = blob.put(type_name);
  const size_t o_pkind = blob.put(pod_kind);
  const size_t o_bkeys = blob.put(base_keys);
  const size_t o_bexcl = blob.put(base_excl);
  const size_t o_tlp = blob.put(C.tmpl_limit_present);
  const size_t o_trem = blob.put(C.tmpl_remaining);
  const size_t o_shpc = blob.put(C.shape_hp_conf), o_shpa = blob.put(C.shape_hp_add), o_exhp = blob.put(C.ex_hp);
  const size_t o_npool = blob.put(plan->node_pool);
  const size_t host_bytes = blob.host.size();
  const size_t o_usable = blob.reserve(sizeof(uint64_t) * (size_t)std::max(SL, 1) * std::max(EW, 1));
  const size_t o_tres = blob.reserve(sizeof(SimNC) * (size_t)std::max(SL, 1));
  HIPCHK(hipMalloc(&plan->buf.p, blob.host.size()));
  uint8_t* base = (uint8_t*)plan->buf.p;
  {
    vector<DevCatalog> dc = DevCats(base, C, coffs);
    memcpy(blob.host.data() + o_cats, dc.data(), sizeof(DevCatalog) * dc.size());
  }
  HIPCHK(hipMemcpyAsync(base, blob.host.data(), host_bytes, hipMemcpyHostToDevice, ctx->stream));

  SimArgs& a = plan->a;
  memset(&a, 0, sizeof a);
  a.dict = (const DevDict*)(base + o_dict);
  a.cats = (const DevCatalog*)(base + o_cats);
  a.n_catalogs = (int32_t)coffs.size();
  a.SL = SL;
  a.vint = (const int64_t*)(base + o_vint);
  a.shape_level_base = (const int32_t*)(base + o_slb);
  a.shape_nlevels = (const int32_t*)(base + o_snl);
  a.sl_shape = (const int32_t*)(base + o_sls);
  a.shape_reqs = base + o_sreqs;
  a.shape_negop = (const uint64_t*)(base + o_sneg);
  a.shape_requests = (const int64_t*)(base + o_sreq);
  a.shape_tolerates = (const uint64_t*)(base + o_stol);
  a.shape_pvp = (const uint64_t*)(base + o_pvp);
  a.pvp_base = (const int32_t*)(base + o_pvpb);
  a.pvp_slot = (const int32_t*)(base + o_pvps);
  a.n_tmpl = NT;
  a.tmpl_reqs = base + o_treqs;
  a.tmpl_taintset = (const int32_t*)(base + o_tts);
  a.tmpl_catalog = (const int32_t*)(base + o_tcat);
  a.tmpl_nodepool = (const int32_t*)(base + o_tnp);
  a.tmpl_X = (const uint64_t*)(base + o_tX);
  a.tmpl_daemon = (const int64_t*)(base + o_tdm);
  a.tmpl_limit_present = (const uint32_t*)(base + o_tlp);
  a.tmpl_remaining = (const int64_t*)(base + o_trem);
  a.pod_kind = base + o_pkind;
  a.base_keys = (const uint32_t*)(base + o_bkeys);
  a.base_excl = (const uint64_t*)(base + o_bexcl);
  a.n_base = plan->n_base;
  a.E = E;
  a.EW = EW;
  a.ex_code = (const uint16_t*)(base + o_excode);
  a.ex_taintset = (const int32_t*)(base + o_exts);
  a.ex_available = (const int64_t*)(base + o_exav);
  a.ex_requests = (const int64_t*)(base + o_exrq);
  a.ex_init = base + o_exin;
  a.hp_any = C.hp_any ? 1 : 0;
  a.shape_hp_conf = (const uint64_t*)(base + o_shpc);
  a.shape_hp_add = (const uint64_t*)(base + o_shpa);
  a.ex_hp = (const uint64_t*)(base + o_exhp);
  a.usable = (uint64_t*)(base + o_usable);
  a.tres = (SimNC*)(base + o_tres);
  a.pod_shape = (const int32_t*)(base + o_pshape);
  a.pod_rank = (const uint32_t*)(base + o_prank);
  a.rank_pod = (const uint32_t*)(base + o_rpod);
  a.node_pos = (const int32_t*)(base + o_npos);
  a.node_pod_off = (const uint32_t*)(base + o_noff);
  a.node_pods = (const uint32_t*)(base + o_npods);
  a.node_price = (const double*)(base + o_nprice);
  a.node_flags = base + o_nflags;
  a.node_name = (const uint32_t*)(base + o_nname);
  a.type_name = (const uint32_t*)(base + o_tname);
  plan->d_node_pool = (const uint16_t*)(base + o_npool);
  a.ct_key = ctk;
  a.spot_bit = ctk >= 0 ? d.bit(ctk, "spot") : -1;
  a.od_bit = ctk >= 0 ? d.bit(ctk, "on-demand") : -1;
  a.req_res_mask = 0;
  for (size_t i = 0; i < C.shape_requests.size(); i++)
    if (C.shape_requests[i] > 0) a.req_res_mask |= 1u << (i % KP_NRES);
  for (size_t i = 0; i < C.B->tmpl_daemon.size(); i++)
    if (C.B->tmpl_daemon[i] > 0) a.req_res_mask |= 1u << (i % KP_NRES);
  a.RU = 0;
  for (int r = 0; r < KP_NRES; r++)
    if ((a.req_res_mask >> r) & 1) a.ru_res[a.RU++] = (int8_t)r;
  a.max_types = 100;
  a.spot_to_spot = cl->spot_to_spot ? 1 : 0;
  (void)TW;
  plan->T2 = 1;
  while (plan->T2 < std::max(T, 1)) plan->T2 <<= 1;
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device) == hipSuccess && ncu > 0)
    plan->n_cu = ncu;
  plan->coffs = coffs;
  plan->o_tX = o_tX;
  plan->o_nprice = o_nprice;
  plan->o_nflags = o_nflags;
  plan->node_flags = node_flags;
  HIPCHK(launch_sim_prep(a, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  owned_copy.th.join();
  if (owned_copy.failed || !owned_copy.oc) return fail(KP_E_NOMEM, "out of host memory copying the cluster");
  plan->owned = std::move(owned_copy.oc);
  plan->prepare_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = plan.release();
  return KP_OK;
}

// ICE refresh of a resident snapshot (kp_cluster_refresh, see kp_solve_refresh): the catalogues' offering arrays,
// the templates' options, the candidates' prices, then sim_prep_kernel again (its per shape-level template
// outcomes read the options and prices). A general-path plan compiles every simulation from the live catalogues.
int32_t kp_cluster_refresh(kp_cluster_plan* plan) {
  if (!plan) return fail(KP_E_INVAL, "null argument");
  if (plan->general) return KP_OK;
  kp_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  SolveBase& B = *plan->cp->B;
  if (int32_t rc = CatalogsAlive(B.alive)) return rc;
  if (SeqnumsOf(B.catalogs) == B.seqnums) return KP_OK;
  // host side; the snapshot's own device copy is written below, and the new seqnums are committed only once it is
  int32_t rc = RefreshOfferings(nullptr, B, false);
  if (rc < 0) return rc;
  if (rc > 0) return fail(KP_E_INVAL, "the offering update changed which NodePools keep instance types: prepare again");
  uint8_t* base = (uint8_t*)plan->buf.p;
  hipStream_t st = ctx->stream;
  for (size_t i = 0; i < B.cats.size(); i++) {
    const HostCat& hc = B.cats[i];
    const CatOffsets& o = plan->coffs[i];
    HIPCHK(hipMemcpyAsync(base + o.offer, hc.offer_avail.data(), hc.offer_avail.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(base + o.price, hc.price.data(), hc.price.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(base + o.price_cm, hc.price_cm.data(), hc.price_cm.size() * 8, hipMemcpyHostToDevice, st));
    if (!hc.price_sub.empty())
      HIPCHK(hipMemcpyAsync(base + o.price_sub, hc.price_sub.data(), hc.price_sub.size() * 8, hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipMemcpyAsync(base + plan->o_tX, B.tmpl_X.data(), B.tmpl_X.size() * 8, hipMemcpyHostToDevice, st));
  vector<double> price(std::max<size_t>(plan->node_offer.size(), 1), 0);
  for (size_t i = 0; i < plan->node_offer.size(); i++) {
    const auto& no = plan->node_offer[i];
    const bool priced = NodeCandidatePrice(B.catalogs[no.cat]->types[no.type], no.labels, &price[i]);
    plan->node_flags[i] = (uint8_t)((plan->node_flags[i] & ~1) | (priced ? 1 : 0));
  }
  HIPCHK(hipMemcpyAsync(base + plan->o_nprice, price.data(), price.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(base + plan->o_nflags, plan->node_flags.data(), plan->node_flags.size(), hipMemcpyHostToDevice, st));
  HIPCHK(launch_sim_prep(plan->a, st));
  HIPCHK(hipStreamSynchronize(st));
  CommitRefresh(B);
  return KP_OK;
}

void kp_cluster_plan_destroy(kp_cluster_plan* p) {
  if (!p) return;
  (void)hipSetDevice(p->ctx->device);
  delete p;
}

// One batch on the resident snapshot, results left on the device (a_out.out); the caller holds ctx->mu.
// ---- general simulations: each subset's SimulateScheduling as a whole Solve on the device -----------------------
// Used for clusters the batched sim kernels do not model (topology spread; pod NotIn/DoesNotExist on a label key
// some node lacks). Per subset: the pending pods, the deleting nodes' pods and the subset's pods are scheduled onto
// every other node (existing), with every pod still bound to one of those nodes as a bound pod (Topology.countDomains
// skips the pods being scheduled), then computeConsolidation's decision is taken on the Solve result exactly as the
// batched kernel takes it (sim_kernel's decision; disruption.md:89-128).
namespace {
bool OfferAdmits(const Dict& d, const KReqs& R, const HostOffering& o) {
  auto admits = [&](const char* key, bool has, const string& v) {
    if (!has) return true;
    const int k = d.key(key);
    if (k < 0 || !((R.present >> k) & 1)) return true;  // undefined well-known key: allowed
    const int b = d.bit(k, v);
    if (b < 0) return ((R.compl_ >> k) & 1) != 0;
    return Has(d, R, k, b);
  };
  // reservation keys: an offering without one is DoesNotExist on it, compatible with NotIn / DoesNotExist only
  auto admits_res = [&](const char* key, bool has, const string& v) {
    if (has) return admits(key, true, v);
    const int k = d.key(key);
    if (k < 0 || !((R.present >> k) & 1)) return true;
    const bool c = ((R.compl_ >> k) & 1) != 0, nz = KeyNonEmptyVals(d, R, k);
    return (c && nz) || (!c && !nz);
  };
  return admits(kCapType, true, o.ct) && admits(kZone, o.has_zone, o.zone) && admits(kZoneID, o.has_zid, o.zid) &&
         admits_res(kResID, o.has_rid, o.rid) && admits_res(kResType, o.has_rt, o.rt);
}
// Offerings.Available().Compatible(reqs).WorstLaunchPrice: capacity types in precedence reserved, spot, on-demand
double WorstLaunch(const Dict& d, const KReqs& R, const HostType& t, bool spot_only) {
  for (const char* ct : {"reserved", "spot", "on-demand"}) {
    if (spot_only && strcmp(ct, "spot") != 0) continue;
    bool any = false;
    double mx = 0;
    for (auto& o : t.offs) {
      if (!o.available || o.ct != ct || !OfferAdmits(d, R, o)) continue;
      if (!any || o.price > mx) mx = o.price;
      any = true;
    }
    if (any) return mx;
  }
  return std::numeric_limits<double>::max();
}
}  // namespace

// The offerings as OfferAdmits reads them, resolved against one dictionary once (the batched decisions run
// WorstLaunch over up to 100 options per simulation): per offering its capacity-type class and the dictionary bits
// of its five offering keys (-1: a value the dictionary lacks, -2: the offering has no such requirement).
struct OffBits {
  int16_t ct_class;  // 0 reserved, 1 spot, 2 on-demand, 3 other
  int16_t b[5];      // capacity type, zone, zone id, reservation id, reservation type
};
struct OfferTab {
  int k[5];                                  // the five keys' dictionary ids (-1: absent)
  vector<vector<vector<OffBits>>> off;       // [catalogue][type][offering]
  void Build(const Dict& d, const kp_cluster& cl) {
    const char* keys[5] = {kCapType, kZone, kZoneID, kResID, kResType};
    for (int i = 0; i < 5; i++) k[i] = d.key(keys[i]);
    off.assign(cl.n_catalogs, {});
    for (uint32_t c = 0; c < cl.n_catalogs; c++) {
      const vector<HostType>& types = cl.catalogs[c]->types;
      off[c].resize(types.size());
      for (size_t t = 0; t < types.size(); t++)
        for (const HostOffering& o : types[t].offs) {
          OffBits x;
          x.ct_class = o.ct == "reserved" ? 0 : o.ct == "spot" ? 1 : o.ct == "on-demand" ? 2 : 3;
          const string* v[5] = {&o.ct, &o.zone, &o.zid, &o.rid, &o.rt};
          const bool has[5] = {true, o.has_zone, o.has_zid, o.has_rid, o.has_rt};
          for (int i = 0; i < 5; i++) x.b[i] = !has[i] ? -2 : k[i] < 0 ? -1 : (int16_t)std::max(-1, d.bit(k[i], *v[i]));
          off[c][t].push_back(x);
        }
    }
  }
  // OfferAdmits on the resolved bits
  bool Admits(const Dict& d, const KReqs& R, const OffBits& x) const {
    for (int i = 0; i < 5; i++) {
      const int kk = k[i];
      if (kk < 0 || !((R.present >> kk) & 1)) continue;  // undefined well-known key: allowed
      if (x.b[i] == -2) {
        if (i < 3) continue;  // no zone / zone-id requirement on the offering
        const bool c = ((R.compl_ >> kk) & 1) != 0, nz = KeyNonEmptyVals(d, R, kk);  // DoesNotExist on it
        if (!((c && nz) || (!c && !nz))) return false;
      } else if (x.b[i] == -1) {
        if (!((R.compl_ >> kk) & 1)) return false;
      } else if (!Has(d, R, kk, x.b[i])) {
        return false;
      }
    }
    return true;
  }
  // WorstLaunch on the resolved bits
  double Worst(const Dict& d, const KReqs& R, const HostType& t, const vector<OffBits>& ob, bool spot_only) const {
    for (int cls = 0; cls < 3; cls++) {
      if (spot_only && cls != 1) continue;
      bool any = false;
      double mx = 0;
      for (size_t i = 0; i < t.offs.size(); i++) {
        const HostOffering& o = t.offs[i];
        if (!o.available || ob[i].ct_class != cls || !Admits(d, R, ob[i])) continue;
        if (!any || o.price > mx) mx = o.price;
        any = true;
      }
      if (any) return mx;
    }
    return std::numeric_limits<double>::max();
  }
};

// getCandidatePrices' per-node terms, once per cluster plan (the nodes' labels and offerings do not change between
// batches; a catalogue refresh rebuilds the batch and with it this cache)
struct CandCache {
  vector<double> price;        // cheapest label-compatible offering price
  vector<char> priced, spot;   // some offering is compatible; the node is labelled spot
  void Build(const kp_cluster& cl, const vector<std::map<string, string>>& labels) {
    const int N = (int)cl.n_nodes;
    price.assign(N, 0);
    priced.assign(N, 0);
    spot.assign(N, 0);
    for (int c = 0; c < N; c++) {
      const kp_cluster_node& n = cl.nodes[c];
      double p = 0;
      priced[c] = NodeCandidatePrice(cl.catalogs[n.catalog]->types[n.instance_type], labels[c], &p) ? 1 : 0;
      price[c] = p;
      auto f = labels[c].find(kCapType);
      spot[c] = f != labels[c].end() && f->second == "spot";
    }
  }
};

// computeConsolidation's decision on one simulation's Solve (sim_kernel's decision; disruption.md:89-128). all: every
// non-pending pod was scheduled (and no candidate pod onto an uninitialized node). The Solve made n_nc NodeClaims;
// R / ci / nodepool / opts: the first one's final requirements (held reservation ids applied), catalogue, NodePool and
// price-ordered options (after Truncate), minValues not yet checked on them.
// why (kp_cluster_simulate_explained, or null): the record of the exit taken, in kp_abi.h's order. The caller has
// filled the Solve's fields (WhySolve); Truncate's minValues check is judged before the candidates' prices and the
// spot-to-spot gate, which changes no decision (every one of those exits is a no-op).
struct WhySolve {
  kp_sim_why* why = nullptr;
  uint32_t nc_np = 0;          // non-pending pods on NodeClaim 0 (they fail when its truncated options break minValues)
  int64_t bad_pos = INT64_MAX; // queue position of first_unscheduled as filled
  int64_t nc_pos = INT64_MAX;  // queue position and cluster pod of the first non-pending pod on NodeClaim 0
  int32_t nc_pod = -1;
};
static void WhyClear(kp_sim_why* w) {
  memset(w, 0, sizeof *w);
  w->first_unscheduled = w->unpriced = -1;
}
static void GeneralDecide(const kp_cluster& cl, const vector<std::map<string, string>>& labels,
                          const vector<uint32_t>& cand, const SolveBase& B, bool all, int n_nc, const KReqs* R,
                          int ci, uint32_t nodepool, const uint32_t* opts, uint32_t n_opts, int32_t multi_node,
                          SimOut& r, const OfferTab* tab = nullptr, const CandCache* cc = nullptr,
                          vector<int>* kept_out = nullptr, bool* s2s_out = nullptr, const WhySolve* ws = nullptr) {
  kp_sim_why* why = ws ? ws->why : nullptr;
  double candPrice = 0;
  bool priced = true, allSpot = true;
  int32_t unpriced = -1;
  for (size_t k = 0; k < cand.size(); k++) {
    const uint32_t c = cand[k];
    if (cc) {
      priced = priced && cc->priced[c];
      if (unpriced < 0 && !cc->priced[c]) unpriced = (int32_t)k;
      candPrice += cc->price[c];
      allSpot = allSpot && cc->spot[c];
      continue;
    }
    const kp_cluster_node& n = cl.nodes[c];
    double p = 0;
    if (!NodeCandidatePrice(cl.catalogs[n.catalog]->types[n.instance_type], labels[c], &p)) {
      priced = false;
      if (unpriced < 0) unpriced = (int32_t)k;
    }
    candPrice += p;
    auto f = labels[c].find(kCapType);
    if (f == labels[c].end() || f->second != "spot") allSpot = false;
  }
  r.candidate_price = priced ? candPrice : 0;
  auto exit_as = [&](int32_t reason, int32_t stage = 0) {
    if (why) why->reason = reason, why->stage = stage;
  };
  if (why && n_nc > 1) {  // stopped at (or made) a second NodeClaim: nothing of the unfinished Solve is reported
    WhyClear(why);
    why->n_nodeclaims = 2;
    return exit_as(KP_UNCONS_MULTIPLE_NODECLAIMS);
  }
  // (with `why`, a Solve that left pods unscheduled still takes Truncate's minValues check on its one NodeClaim first:
  // that NodeClaim's pods fail too and are counted, as sim_kernel and a subset's own whole Solve count them)
  if (!all && (!why || n_nc != 1)) return exit_as(KP_UNCONS_UNSCHEDULABLE);  // no-op
  if (n_nc == 0) {
    r.decision = KP_DECISION_DELETE;
    r.savings = r.candidate_price;
    return;
  }
  if (n_nc != 1) return;
  const Dict& d = B.d;
  const vector<HostType>& types = cl.catalogs[ci]->types;
  const HostCat& hc = B.cats[ci];
  const bool hasMin = (R->hmin & R->present) != 0;
  if (hasMin) {  // Truncate(reqs, max): minValues must hold on the truncated options, else its pods fail (no-op)
    vector<int> ts(opts, opts + n_opts);
    if (!HostMinValuesOK(d, hc, *R, ts)) {
      if (why) {
        why->n_unscheduled += ws->nc_np;
        if (ws->nc_pos < ws->bad_pos) why->first_unscheduled = ws->nc_pod;
      }
      return exit_as(KP_UNCONS_UNSCHEDULABLE);
    }
  }
  if (!all) return exit_as(KP_UNCONS_UNSCHEDULABLE);
  const int kct = d.key(kCapType), bspot = kct >= 0 ? d.bit(kct, "spot") : -1;
  const bool ncSpot = kct < 0 || !((R->present >> kct) & 1) || (bspot >= 0 ? Has(d, *R, kct, bspot) : ((R->compl_ >> kct) & 1));
  const bool s2s = allSpot && ncSpot;  // spot-to-spot: only behind the feature gate
  auto worst = [&](int t) {
    return tab ? tab->Worst(d, *R, types[t], tab->off[ci][t], s2s) : WorstLaunch(d, *R, types[t], s2s);
  };
  if (why) {
    why->n_truncated = n_opts;
    double lo = std::numeric_limits<double>::max();
    for (uint32_t i = 0; i < n_opts; i++) lo = std::min(lo, worst((int)opts[i]));
    why->cheapest_launch = n_opts ? lo : 0;
  }
  if (!priced) {
    if (why) why->unpriced = unpriced;
    return exit_as(KP_UNCONS_UNPRICED);
  }
  if (s2s && !cl.spot_to_spot) return exit_as(KP_UNCONS_SPOT_TO_SPOT_DISABLED);
  vector<int> kept;
  for (uint32_t i = 0; i < n_opts; i++)
    if (worst((int)opts[i]) < candPrice) kept.push_back((int)opts[i]);
  if (why) why->n_cheaper = (uint32_t)kept.size();
  if (kept.empty()) return exit_as(KP_UNCONS_NOT_CHEAPER);
  if (hasMin && !HostMinValuesOK(d, hc, *R, kept)) return exit_as(KP_UNCONS_MIN_VALUES, 1);
  if (why && !multi_node) why->n_same_type = (uint32_t)kept.size();
  if (multi_node) {  // filterOutSameType: the candidates' cheapest price per type name
    vector<std::pair<const string*, double>> prices;
    for (uint32_t c : cand) {
      const kp_cluster_node& n = cl.nodes[c];
      const HostType& it = cl.catalogs[n.catalog]->types[n.instance_type];
      double p = 0;
      if (cc ? !cc->priced[c] : !NodeCandidatePrice(it, labels[c], &p)) continue;
      if (cc) p = cc->price[c];
      bool found = false;
      for (auto& e : prices)
        if (*e.first == it.name) {
          e.second = std::min(e.second, p);
          found = true;
        }
      if (!found) prices.push_back({&it.name, p});
    }
    double maxPrice = std::numeric_limits<double>::max();
    for (int t : kept)
      for (auto& e : prices)
        if (*e.first == types[t].name && e.second < maxPrice) maxPrice = e.second;
    vector<int> k2;
    for (int t : kept)
      if (worst(t) < maxPrice) k2.push_back(t);
    if (why) why->n_same_type = (uint32_t)k2.size();
    if (k2.empty()) return exit_as(KP_UNCONS_SAME_TYPE);
    if (hasMin && !HostMinValuesOK(d, hc, *R, k2)) return exit_as(KP_UNCONS_MIN_VALUES, 2);
    kept.swap(k2);
  }
  if (s2s && cand.size() == 1) {
    if (kept.size() < 15) return exit_as(KP_UNCONS_SPOT_FLEXIBILITY);
    kept.resize(std::min<size_t>(kept.size(), hasMin ? 100 : 15));
  }
  double best = std::numeric_limits<double>::max();
  for (int t : kept) best = std::min(best, worst(t));
  r.decision = KP_DECISION_REPLACE;
  r.nodepool = nodepool;
  r.replacement_price = best;
  r.savings = candPrice - best;
  r.n_options = (uint32_t)kept.size();
  if (kept_out) kept_out->assign(kept.begin(), kept.end());  // the command's InstanceTypeOptions, price order
  if (s2s_out) *s2s_out = s2s;
}

// One subset's SimulateScheduling as its own Solve: compiled on the host from the subset's inputs (the path for
// subsets the batch cannot take, and the whole path with KP_GENERAL_BATCH=0).
struct SimOneSolve {
  vector<kp_existing_node> ex;  // the Solve's existing nodes: neither in the subset nor being deleted, cluster order
  vector<int> kind;             // per queued pod (input order): 0 candidate pod, 1 deleting-node pod, 2 pending
  vector<uint32_t> cluster_pod; // per queued pod: its cluster pod index
  std::unique_ptr<kp_solve_plan, void (*)(kp_solve_plan*)> sp{nullptr, kp_solve_plan_destroy};
  std::unique_ptr<kp_solve_result, void (*)(kp_solve_result*)> res{nullptr, kp_result_destroy};
};
// What a general-path call adds up over its launches and its subsets compiled alone
struct GenTotals {
  uint64_t counters[3] = {0, 0, 0};  // attempts, bytes, pops
  uint64_t batched = 0, single = 0, n_launches = 0;  // simulations batched / compiled per subset, batched launches
  double dev_ms = 0;
  double host_ms[2] = {0, 0};  // the batch's host work: overlays + arguments, decisions
};
// The same from the eight counter words a cluster call leaves on the device (sim_kernel's stats, and GeneralSimLocked's
// in their place: attempts, bytes, pops, batched, single, -, launches) and its device time
static GenTotals TotalsOf(const uint64_t* kst, double dev_ms) {
  GenTotals T;
  for (int k = 0; k < 3; k++) T.counters[k] = kst[k];
  T.batched = kst[3], T.single = kst[4], T.n_launches = kst[6];
  T.dev_ms = dev_ms;
  return T;
}
// kp_solve_stats of a cluster call (t0: when the call began). Plans of the batched kernel overwrite phase_cycles[1..2].
static void FillStats(kp_solve_stats* stats, const kp_cluster_plan* plan, const GenTotals& T,
                      std::chrono::steady_clock::time_point t0) {
  stats->device_ms = T.dev_ms;
  stats->solve_kernel_ms = T.dev_ms;
  stats->attempts = T.counters[0];
  stats->bytes_algorithmic = T.counters[1];
  stats->pops = T.counters[2];
  stats->phase_cycles[0] = T.batched;
  stats->phase_cycles[1] = T.single;
  stats->phase_cycles[2] = T.n_launches;
  stats->prepare_ms = plan->prepare_ms;
  stats->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
// AllNonPendingPodsScheduled's rule for one queued pod (the host's copy; the device's is scan_unscheduled). kind: 0 a
// candidate pod, 1 a deleting node's, 2 pending (never counted). The pod fails unplaced (-1), and a candidate pod also
// on an existing node (<= -2) that is not initialized (deleting-node pods exempt); initialized(pos) answers for the
// Solve's existing position pos.
extern "C++" template <class F>
static inline bool PodUnscheduled(int kind, int32_t pl, F initialized) {
  if (kind == 2) return false;
  return pl == -1 || (kind == 0 && pl <= -2 && !initialized(-2 - pl));
}
// SimulateScheduling's Solve over a cluster: its inputs for these existing nodes, queued pods and bound pods
static kp_solve_in SimulationIn(const kp_cluster& cl, const vector<kp_existing_node>& ex, const vector<kp_pod>& pods,
                                const vector<kp_bound_pod>& bound) {
  kp_solve_in in;
  memset(&in, 0, sizeof in);
  in.catalogs = cl.catalogs;
  in.n_catalogs = cl.n_catalogs;
  in.n_nodepools = cl.n_nodepools;
  in.nodepools = cl.nodepools;
  in.existing = ex.data();
  in.n_existing = (uint32_t)ex.size();
  in.n_shapes = cl.n_shapes;
  in.shapes = cl.shapes;
  in.pods = pods.data();
  in.n_pods = (uint32_t)pods.size();
  in.max_instance_types = 100;
  in.bound_pods = bound.data();
  in.n_bound_pods = (uint32_t)bound.size();
  in.namespaces = cl.namespaces;
  in.n_namespaces = cl.n_namespaces;
  in.reserved_offering_mode = KP_RESERVED_STRICT;  // SimulateScheduling: NewScheduler(..., DisableReservedCapacityFallback)
  return in;
}
static int32_t GeneralSolveOne(kp_cluster_plan* plan, const vector<uint32_t>& cand, SimOneSolve& so, GenTotals& T,
                               kp_cancel* cancel) {
  kp_ctx* ctx = plan->ctx;
  const kp_cluster& cl = plan->cluster()->cl;
  const int N = (int)cl.n_nodes;
  vector<char> inS(N, 0);
  for (uint32_t c : cand) inS[c] = 1;
  vector<kp_existing_node>& ex = so.ex;
  vector<int>& kind = so.kind;
  vector<int> exNode;
  for (int i = 0; i < N; i++)
    if (!inS[i] && !cl.nodes[i].deleting) {
      ex.push_back(cl.nodes[i].node);
      exNode.push_back(i);
    }
  vector<kp_pod> pods;
  auto add = [&](uint32_t p, int k) {
    pods.push_back(cl.pods[p]);
    kind.push_back(k);
    so.cluster_pod.push_back(p);
  };
  for (uint32_t j = 0; j < cl.n_pending; j++) {
    if (cl.pending_pods[j] >= cl.n_pods) return fail(KP_E_INVAL, "pending pod %u", cl.pending_pods[j]);
    add(cl.pending_pods[j], 2);
  }
  for (int i = 0; i < N; i++)
    if (cl.nodes[i].deleting)
      for (uint32_t j = 0; j < cl.nodes[i].n_pods; j++) add(cl.nodes[i].pods[j], 1);
  for (uint32_t c : cand)
    for (uint32_t j = 0; j < cl.nodes[c].n_pods; j++) add(cl.nodes[c].pods[j], 0);
  vector<kp_bound_pod> bound;
  for (size_t e = 0; e < exNode.size(); e++) {
    const kp_cluster_node& n = cl.nodes[exNode[e]];
    for (uint32_t j = 0; j < n.n_pods; j++) {
      const uint32_t p = n.pods[j];
      if (p >= cl.n_pods || cl.pods[p].shape >= cl.n_shapes) return fail(KP_E_INVAL, "node %d: pod %u", exNode[e], p);
      const kp_pod_shape& sh = cl.shapes[cl.pods[p].shape];
      bound.push_back({sh.namespace_, sh.labels, sh.n_labels, (uint32_t)e, sh.required_anti_affinity,
                       sh.n_required_anti_affinity, 0});
    }
  }
  const kp_solve_in in = SimulationIn(cl, ex, pods, bound);
  kp_solve_plan* sp = nullptr;
  int32_t rc = SolvePrepare(ctx, &in, nullptr, &sp);
  if (rc) return rc;
  so.sp.reset(sp);
  kp_solve_result* res = nullptr;
  rc = kp_solve_run_cancellable(sp, cancel, &res);
  if (rc) return rc;
  so.res.reset(res);
  T.counters[0] += res->stats.attempts;
  T.counters[1] += res->stats.bytes_algorithmic;
  T.counters[2] += res->stats.pops;
  T.dev_ms += res->stats.device_ms;
  return KP_OK;
}
// The spot-to-spot branch of computeConsolidation: the replacement launches spot only, so
// karpenter.sh/capacity-type In [spot] replaces whatever the NodeClaim required of the capacity type.
static void NarrowToSpot(const Dict& d, KReqs& q) {
  const int k = d.key(kCapType);
  const int bit = k >= 0 ? d.bit(k, "spot") : -1;
  if (bit < 0) return;
  for (int wi = 0; wi < nwords(d, k); wi++) q.vals[kw(d, k, wi)] = 0;
  q.vals[bit / 64] |= 1ull << (bit % 64);
  q.present |= 1ull << k;
  q.compl_ &= ~(1ull << k);
  q.hgt &= ~(1ull << k), q.hlt &= ~(1ull << k), q.hmin &= ~(1ull << k);
}
// A command (kp_cluster_command) is the Solve's own result cut to the options the decision kept, spot-to-spot narrowed
static void CutToCommand(const Dict& d, kp_solve_result& res, const vector<int>& kept, bool s2s) {
  res.ncs[0].options.assign(kept.begin(), kept.end());
  if (s2s) {
    NarrowToSpot(d, res.fin[0]);
    res.ncs[0].reqs = DecodeReqs(d, res.fin[0]);
  }
}
// command (kp_cluster_command): where to leave the decision's command; its placements are already in the simulation's
// input order and name the Solve's existing nodes
static int32_t GeneralSimOne(kp_cluster_plan* plan, const vector<uint32_t>& cand, const vector<std::map<string, string>>& labels,
                             int32_t multi_node, SimOut& r, GenTotals& T, kp_cancel* cancel, kp_solve_result** command,
                             kp_sim_why* why = nullptr) {
  SimOneSolve so;
  if (int32_t rc = GeneralSolveOne(plan, cand, so, T, cancel)) return rc;
  const kp_cluster& cl = plan->cluster()->cl;
  const kp_solve_result* res = so.res.get();
  r.n_pods = (uint32_t)so.kind.size();
  bool all = true;  // (a no-op at the first failure)
  for (size_t p = 0; p < so.kind.size() && all; p++)
    all = !PodUnscheduled(so.kind[p], res->placement[p], [&](int pos) { return so.ex[(size_t)pos].initialized != 0; });
  const int n_nc = (int)res->ncs.size();
  vector<int> kept;
  bool s2s = false;
  WhySolve ws;
  if (why) {  // the Solve's fields, from its own result in its own queue order (kp_drift_result's rule)
    WhyClear(why);
    ws.why = why;
    why->n_nodeclaims = (uint32_t)std::min(n_nc, 2);
    for (int32_t p : so.sp->cp->queue)
      if (PodUnscheduled(so.kind[p], res->placement[p], [&](int pos) { return so.ex[(size_t)pos].initialized != 0; }))
        if (why->n_unscheduled++ == 0) why->first_unscheduled = (int32_t)so.cluster_pod[p];
    // (kp_solve_run has applied Truncate's minValues check: the pods of a NodeClaim that broke it are unplaced already)
  }
  // (kp_solve_run already applied the held reservations and the minValues truncation check to NodeClaim 0)
  GeneralDecide(cl, labels, cand, *so.sp->cp->B, all, n_nc, n_nc ? &res->fin[0] : nullptr, n_nc ? res->nc_cat[0] : 0,
                n_nc ? res->ncs[0].nodepool : 0, n_nc ? res->ncs[0].options.data() : nullptr,
                n_nc ? (uint32_t)res->ncs[0].options.size() : 0, multi_node, r, nullptr, nullptr, &kept, &s2s,
                why ? &ws : nullptr);
  if (command && r.decision != KP_DECISION_NOOP) {
    if (r.decision == KP_DECISION_REPLACE) CutToCommand(so.sp->cp->B->d, *so.res, kept, s2s);
    *command = so.res.release();
  }
  return KP_OK;
}

// ---- batched general simulations ------------------------------------------------------------------------------
// Compiling each subset's Solve on the host walks every node and every bound pod (~18 ms per subset at 2000 nodes).
// Instead the cluster is compiled once as the superset Solve - every node not being deleted is an existing node,
// every pod a simulation can queue (pending, deleting nodes', every node's) is in its pod list - with each node's
// contribution to the topology state recorded (Compiled::track_nodes). A subset's Solve is that Solve with:
//   * the subset's nodes excluded from placement (ex_static_ok 0) - the other nodes keep their relative order;
//   * its queue: the pending and deleting-node pods plus the subset's pods, in the superset's queue order (the same
//     keys: shape rank, creation, UID);
//   * the bound pods on its nodes removed from the topology counts and registered domains (Topology.countDomains
//     over the remaining nodes), hostname rows' "some domain has a count" recomputed;
//   * the spread groups' liveness recomputed from the shapes it queues (NewTopology creates the groups of queued
//     pods), and hostname groups that stop being live at creation get their unregistered nodes (255) back.
// Subsets whose removal would make an inverse anti-affinity group vanish take the per-subset compile. Every
// simulation of a batch is one workgroup of one solve_kernel launch (its own arena: mutable state + scratch).
// Host memory the device copies read from / write into while the host prepares the next launch (pinned: an async
// copy from pageable memory would stage synchronously), grown geometrically.
struct PinnedBuf {
  void* p = nullptr;
  size_t n = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
  hipError_t reserve(size_t bytes) {
    if (bytes <= n) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
    const size_t want = std::max(bytes, (size_t)(1.5 * (double)bytes));
    const hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) n = want;
    else p = nullptr;
    return e;
  }
  uint8_t* at(size_t off) const { return (uint8_t*)p + off; }
};

// One launch slot of the general batch: device arenas + argument blocks, the pinned host copies its launch reads
// (overlays, arguments) and writes (results), and the event that marks its results landed.
struct GenSlot {
  DevBuf arenas, args;
  size_t arenas_bytes = 0, args_bytes = 0;
  DevBuf rec;  // record-mode launches: the simulations' queue pods, lengths and caller indices, and the launch's record
  size_t rec_bytes = 0;
  PinnedBuf up, down;
  hipEvent_t done = nullptr, t0 = nullptr, t1 = nullptr;  // results landed; the launch's kernels (timing)
  hipEvent_t uploaded = nullptr;                            // the launch's overlays and arguments on the device
  hipStream_t ks = nullptr;               // the slot's kernel stream (CopyStreams::k)
  const FinalizeArgs* dfargs = nullptr;   // the launch's finalize arguments in `args`
  int n = 0;
  size_t b0 = 0;
  vector<vector<int32_t>> queues;
  ~GenSlot() {
    for (hipEvent_t e : {done, t0, t1, uploaded})
      if (e) (void)hipEventDestroy(e);
  }
};
// the batch's copy streams: uploads (the next launch's overlays) and downloads (the last launch's results) overlap the
// kernels instead of queueing between them; and one kernel stream per launch slot, so that a launch's batch_init and
// first workgroups fill the CUs the previous launch's last simulations leave idle (the slots share only read-only data)
struct CopyStreams {
  hipStream_t up = nullptr, down = nullptr, k[2] = {nullptr, nullptr};
  ~CopyStreams() {
    for (hipStream_t x : {up, down, k[0], k[1]})
      if (x) (void)hipStreamDestroy(x);
  }
};

struct GeneralBatch {
  std::unique_ptr<Compiled> C;
  size_t ulist_total = 0;  // entries of the per-shape-level usable lists (the batched existing-node memo's size)
  uint64_t base_version = 0;
  vector<int32_t> node_input;   // cluster node -> existing input index of the superset (-1: being deleted)
  vector<int32_t> node_sorted;  // cluster node -> position in the Solve's existing order (-1)
  vector<int32_t> pos_node;     // existing position -> cluster node
  vector<int32_t> pod_qpos;     // superset pod -> queue position
  vector<int32_t> pod_shape;    // superset pod -> shape
  vector<int32_t> base_pods;    // superset pods every simulation queues (pending, deleting nodes'), queue order
  vector<uint8_t> pod_kind;     // superset pod -> 2 pending, 1 deleting node's, 0 a node's
  vector<vector<int32_t>> node_pods;  // cluster node -> its superset pods
  vector<uint8_t> ex_static;
  vector<int32_t> regcnt;       // [G * 64] existing nodes registering each (group, ordinal)
  vector<int32_t> live0;        // [G] liveness with only the base pods queued
  OfferTab offers;              // the decisions' offering bits (the superset's dictionary)
  CandCache cands;              // the candidates' prices
  uint32_t rmask = 0;
  int res_mode = 0, opt_stride = 100, tf_words = 0;
  bool tfeas_on = false;
  SolveOffs so;                 // shared-region offsets
  DevBuf shared;
  // per arena size (Pc): the layout, the host template of [0, mut_end) and the device copy of [common, mut_end)
  int Pc = 0;
  SolveOffs o;
  size_t stride = 0;
  vector<uint8_t> tmpl;
  DevBuf pristine;
  GenSlot slot[2];  // two launch slots (GeneralBatchRun)
  CopyStreams cs;
  // what the verdict kernels gather, uploaded once per plan (RecordTables), and kp_cluster_drift's verdicts
  vector<int32_t> pod_cluster;  // superset pod -> cluster pod index
  bool min_values = false;      // some template or shape-level carries minValues (drift: the per-subset path)
  DevBuf rec_tab, drift_out;
  size_t drift_out_n = 0;
  const uint8_t* d_pod_kind = nullptr;
  const int32_t* d_pod_cluster = nullptr;
  const uint8_t* d_pos_uninit = nullptr;
};

// The superset Solve of a cluster (kp_cluster_plan: general). KP_E_UNSUPPORTED: the batch cannot take this cluster
// (the caller keeps the per-subset compile).
static int32_t GeneralBatchBuild(kp_cluster_plan* plan, std::shared_ptr<GeneralBatch>& out) {
  kp_ctx* ctx = plan->ctx;
  const kp_cluster& cl = plan->cluster()->cl;
  const int N = (int)cl.n_nodes;
  PhaseTimer pt;
  auto gb = std::make_shared<GeneralBatch>();
  vector<kp_existing_node> ex;
  vector<kp_pod> pods;
  vector<kp_bound_pod> bound;
  gb->node_input.assign(N, -1);
  gb->node_pods.assign(N, {});
  for (uint32_t j = 0; j < cl.n_pending; j++) {
    if (cl.pending_pods[j] >= cl.n_pods) return fail(KP_E_INVAL, "pending pod %u", cl.pending_pods[j]);
    pods.push_back(cl.pods[cl.pending_pods[j]]);
    gb->pod_kind.push_back(2);
    gb->pod_cluster.push_back((int32_t)cl.pending_pods[j]);
  }
  for (int i = 0; i < N; i++)
    if (cl.nodes[i].deleting)
      for (uint32_t j = 0; j < cl.nodes[i].n_pods; j++) {
        pods.push_back(cl.pods[cl.nodes[i].pods[j]]);
        gb->pod_kind.push_back(1);
        gb->pod_cluster.push_back((int32_t)cl.nodes[i].pods[j]);
      }
  const int n_base = (int)pods.size();
  for (int i = 0; i < N; i++) {
    if (cl.nodes[i].deleting) continue;
    const uint32_t e = (uint32_t)ex.size();
    gb->node_input[i] = (int32_t)e;
    ex.push_back(cl.nodes[i].node);
    for (uint32_t j = 0; j < cl.nodes[i].n_pods; j++) {
      const uint32_t p = cl.nodes[i].pods[j];
      if (p >= cl.n_pods || cl.pods[p].shape >= cl.n_shapes) return fail(KP_E_INVAL, "node %d: pod %u", i, p);
      const kp_pod_shape& sh = cl.shapes[cl.pods[p].shape];
      bound.push_back({sh.namespace_, sh.labels, sh.n_labels, e, sh.required_anti_affinity, sh.n_required_anti_affinity, 0});
      gb->node_pods[i].push_back((int32_t)pods.size());
      pods.push_back(cl.pods[p]);
      gb->pod_kind.push_back(0);
      gb->pod_cluster.push_back((int32_t)p);
    }
  }
  {  // queue ties broken by pod index would order differently per subset: only distinct (creation, UID) keys
    vector<std::pair<int64_t, uint64_t>> keys;
    for (auto& p : pods) keys.push_back({p.creation_unix, p.uid_key});
    std::sort(keys.begin(), keys.end());
    if (std::adjacent_find(keys.begin(), keys.end()) != keys.end())
      return fail(KP_E_UNSUPPORTED, "pods with equal (creation, UID) keys");
  }
  const kp_solve_in in = SimulationIn(cl, ex, pods, bound);
  pt.lap("general: inputs");
  gb->C = std::make_unique<Compiled>();
  Compiled& C = *gb->C;
  C.track_nodes = true;
  int32_t rc = CompileSolve(&in, C, ctx);
  if (rc) return rc;
  pt.lap("general: superset compile");
  if (!C.track_nodes) return fail(KP_E_INVAL, "superset compile lost its node tracking");
  rc = EnsureBaseOnDevice(ctx, *C.B);
  if (rc) return rc;
  gb->base_version = C.B->version;
  const int E = (int)C.ex_input.size(), G = C.G, P = (int)pods.size();
  gb->node_sorted.assign(N, -1);
  gb->pos_node.assign(E, -1);
  vector<int32_t> input_node(E, -1);
  for (int i = 0; i < N; i++)
    if (gb->node_input[i] >= 0) input_node[gb->node_input[i]] = i;
  for (int e = 0; e < E; e++) {
    gb->pos_node[e] = input_node[C.ex_input[e]];
    gb->node_sorted[gb->pos_node[e]] = e;
  }
  gb->pod_qpos.assign(P, 0);
  gb->pod_shape = C.pod_shape;
  for (int q = 0; q < P; q++) gb->pod_qpos[C.queue[q]] = q;
  for (int q = 0; q < P; q++)
    if (C.queue[q] < n_base) gb->base_pods.push_back(C.queue[q]);
  if (G) {
    if (C.node_cnt.size() != (size_t)E || C.tg_spread.size() != (size_t)G || C.shape_l0.size() != cl.n_shapes)
      return fail(KP_E_INVAL, "superset topology tracking incomplete");
    gb->regcnt.assign((size_t)G * 64, 0);
    for (auto& v : C.node_reg)
      for (int32_t x : v) gb->regcnt[x]++;
    gb->live0.assign(G, 0);
    for (int g = 0; g < G; g++) gb->live0[g] = C.tg_live[g] && !C.tg_spread[g];
    vector<char> seen(cl.n_shapes, 0);
    for (int p : gb->base_pods) {
      const int s = C.pod_shape[p];
      if (seen[s]) continue;
      seen[s] = 1;
      for (int32_t g : C.shape_l0[s]) gb->live0[g] = 1;
    }
  }
  pt.lap("general: tracking");
  for (const KReqs& q : C.B->tmpl_reqs) gb->min_values |= (q.hmin & q.present) != 0;
  for (const KReqs& q : C.shape_reqs) gb->min_values |= (q.hmin & q.present) != 0;
  gb->rmask = RequestedResources(C);
  gb->ex_static = ExStatic(C, gb->rmask);
  gb->offers.Build(C.B->d, cl);
  pt.lap("general: offers");
  {  // (the candidate prices read the capacity-type, zone, zone-id and reservation labels only)
    vector<std::map<string, string>> labels(N);
    for (int i = 0; i < N; i++)
      for (uint32_t j = 0; j < cl.nodes[i].node.n_labels; j++) {
        const kp_label& l = cl.nodes[i].node.labels[j];
        string k = Normalize(l.key ? l.key : "");
        if (k == kCapType || k == kZone || k == kZoneID || k == kResID || k == kResType)
          labels[i][std::move(k)] = l.value ? l.value : "";
      }
    gb->cands.Build(cl, labels);
  }
  pt.lap("general: candidates");
  gb->res_mode = !C.B->res_cls ? 0 : 2;
  gb->opt_stride = 100;
  // the shared region: read-only data of every simulation + the template-options table
  Blob blob;
  PutShared(blob, C, gb->so);
  pt.lap("general: shared blob");
  {  // per shape-level, the positions that can ever take one of its pods (DeviceArgs::ex_ulist): the kernel's
     // count-independent checks on the pristine state
    const int E = (int)C.ex_input.size(), SLn = (int)C.shape_reqs.size();
    vector<int32_t> sl_shape(SLn, 0), off(SLn + 1, 0), list, uidx((size_t)SLn * std::max(E, 1), 0);
    for (size_t s = 0; s < C.shape_level_base.size(); s++)
      for (int l = 0; l < C.shape_nlevels[s]; l++) sl_shape[C.shape_level_base[s] + l] = (int32_t)s;
    for (int sl = 0; sl < SLn; sl++) {
      off[sl] = (int32_t)list.size();
      const int s = sl_shape[sl];
      const int64_t* pq = &C.shape_requests[(size_t)s * KP_NRES];
      const uint64_t tol = C.shape_tolerates[sl], hpc = C.hp_any ? C.shape_hp_conf[s] : 0;
      for (int e = 0; e < E; e++) {
        uidx[(size_t)sl * E + e] = (int32_t)(list.size() - off[sl]);
        bool ok = gb->ex_static[e] && ((tol >> C.ex_taintset[e]) & 1) && !(hpc && (C.ex_hp[e] & hpc));
        for (uint32_t m = gb->rmask; m && ok; m &= m - 1) {
          const int r = __builtin_ctz(m);
          ok = C.ex_available[(size_t)e * KP_NRES + r] - C.ex_requests[(size_t)e * KP_NRES + r] >= pq[r];
        }
        if (ok) list.push_back(e);
      }
    }
    off[SLn] = (int32_t)list.size();
    gb->ulist_total = list.size();  // (the batched arenas' existing-node memo: one entry per list entry)
    if (list.empty()) list.push_back(0);
    gb->so.exul = blob.put(list);
    gb->so.exuo = blob.put(off);
    gb->so.exui = blob.put(uidx);
  }
  pt.lap("general: usable lists");
  const size_t host_bytes = blob.host.size();
  const int NT = (int)C.B->tmpl_reqs.size(), SLi = (int)C.shape_reqs.size();
  gb->tfeas_on = NT > 0 && SLi > 0 && ctx->ov.template_table == 0;
  gb->tf_words = C.B->TW + KP_NRES / 2 + 1;
  gb->so.tfeas = blob.reserve_dev(gb->tfeas_on ? (size_t)SLi * NT * gb->tf_words * sizeof(uint64_t) : 8);
  HIPCHK(gb->shared.alloc(blob.total()));
  uint8_t* sh = (uint8_t*)gb->shared.p;
  HIPCHK(hipMemcpyAsync(sh, blob.host.data(), host_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (gb->tfeas_on) {
    SolveArgs a;
    BindSolve(a, C, gb->so, sh, sh, 0, 1, gb->rmask, gb->res_mode);
    HIPCHK(launch_tmpl_feas(TfeasOf(a, sh, gb->so, SLi, gb->tf_words), ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  pt.lap("general: upload + table");
  out = gb;
  return KP_OK;
}

// The arena layout for simulations of up to Pc pods: host template + the device copy of the common mutable part.
static int32_t GeneralBatchLayout(kp_ctx* ctx, GeneralBatch& gb, int Pc) {
  if (gb.Pc == Pc) return KP_OK;
  const Compiled& C = *gb.C;
  SolveOffs o = gb.so;
  Blob blob;
  const vector<int32_t> zeros(Pc, 0);
  PutArena(blob, C, zeros, zeros, Pc, gb.ex_static, gb.rmask, o);
  ReserveArenaDev(blob, C, Pc, gb.opt_stride, std::min(SortCapacity(C.ov), Pc), false, o, gb.ulist_total);
  gb.tmpl.assign(blob.host.begin(), blob.host.begin() + o.mut_end);
  gb.stride = (o.arena_end + 255) & ~(size_t)255;
  HIPCHK(gb.pristine.alloc(o.mut_end - o.common + 16));
  HIPCHK(hipMemcpyAsync(gb.pristine.p, gb.tmpl.data() + o.common, o.mut_end - o.common, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  gb.o = o;
  gb.Pc = Pc;
  return KP_OK;
}

// One simulation's per-subset inputs: its queue (superset pods) and the patch of [0, common) of its arena. Returns 1
// when the batch cannot take the subset (an inverse anti-affinity group would vanish).
struct GenScratch {
  vector<int32_t> inv, hdec, regdec, touched;
  vector<char> shape_seen;
};
// The host work of a batched launch is per simulation (the overlays before it, the decisions after it): split over up
// to kMaxHostThreads threads, f(begin, end, thread index). Workers never call fail() (its message is thread-local).
constexpr int kMaxHostThreads = 16;
extern "C++" template <class F>
static void ParallelFor(int n, F f) {
  static const int hw = (int)std::max(1u, std::thread::hardware_concurrency());
  const int T = std::max(1, std::min(std::min(hw, kMaxHostThreads), n / 128));
  if (T <= 1) {
    f(0, n, 0);
    return;
  }
  vector<std::thread> th;
  th.reserve(T - 1);
  for (int t = 1; t < T; t++) th.emplace_back(f, (int)((int64_t)n * t / T), (int)((int64_t)n * (t + 1) / T), t);
  f(0, (int)((int64_t)n / T), 0);
  for (auto& x : th) x.join();
}
static int GeneralPatch(const GeneralBatch& gb, const kp_cluster& cl, const vector<uint32_t>& cand, GenScratch& s,
                        vector<int32_t>& queue, uint8_t* patch) {
  const Compiled& C = *gb.C;
  const int G = C.G, E = (int)C.ex_input.size();
  if (G) {  // an inverse group whose every owner sits on the subset's nodes does not exist in its Solve
    s.inv.assign(G, 0);
    bool vanish = false;
    for (uint32_t c : cand)
      for (int32_t g : C.node_inv[gb.node_input[c]])
        if (++s.inv[g] == C.tg_inv_total[g]) vanish = true;
    if (vanish) return 1;
  }
  queue = gb.base_pods;
  const size_t nb = queue.size();
  for (uint32_t c : cand) queue.insert(queue.end(), gb.node_pods[c].begin(), gb.node_pods[c].end());
  auto byq = [&](int32_t x, int32_t y) { return gb.pod_qpos[x] < gb.pod_qpos[y]; };
  std::sort(queue.begin() + nb, queue.end(), byq);
  std::inplace_merge(queue.begin(), queue.begin() + nb, queue.end(), byq);
  const SolveOffs& o = gb.o;
  memcpy(patch, gb.tmpl.data(), o.common);
  int32_t* ps = (int32_t*)(patch + o.pod_shape);
  int32_t* qu = (int32_t*)(patch + o.queue);
  for (size_t i = 0; i < queue.size(); i++) {
    ps[i] = gb.pod_shape[queue[i]];
    qu[i] = (int32_t)i;
  }
  uint8_t* exso = patch + o.exso;
  for (uint32_t c : cand) exso[gb.node_sorted[c]] = 0;
  if (!G) return 0;
  int32_t* cnt = (int32_t*)(patch + o.tgc);
  int32_t* live = (int32_t*)(patch + o.tglv);
  uint64_t* reg = (uint64_t*)(patch + o.tgreg);
  uint8_t* hcx = patch + o.hcx;
  s.regdec.resize((size_t)G * 64);
  s.hdec.assign(G, 0);
  s.touched.clear();
  for (uint32_t c : cand) {
    const int e = gb.node_input[c];
    for (int32_t x : C.node_cnt[e]) cnt[x]--;
    for (int32_t x : C.node_reg[e]) {
      if (s.regdec[x]++ == 0) s.touched.push_back(x);
    }
    for (int32_t g : C.node_hrec[e]) s.hdec[g]++;
  }
  for (int32_t x : s.touched) {
    const int g = x / 64, ord = x % 64;
    if (s.regdec[x] == gb.regcnt[x] && !((C.tg_reg_static[g] >> ord) & 1)) reg[g] &= ~(1ull << ord);
    s.regdec[x] = 0;
  }
  for (int g = 0; g < G; g++)
    if (s.hdec[g] && s.hdec[g] == C.tg_hrec_total[g]) reg[g] &= ~1ull;  // hostname row: no domain has a count
  // liveness: the base pods' shapes, then the subset's
  for (int g = 0; g < G; g++) live[g] = gb.live0[g];
  s.shape_seen.assign(cl.n_shapes, 0);
  for (size_t i = nb; i < queue.size(); i++) {
    const int sh = gb.pod_shape[queue[i]];
    if (s.shape_seen[sh]) continue;
    s.shape_seen[sh] = 1;
    for (int32_t g : C.shape_l0[sh]) live[g] = 1;
  }
  for (int g = 0; g < G; g++)  // a hostname spread group created not live: its unregistered nodes hold 255
    if (C.tg_live[g] && !live[g] && C.tg_spread[g] && C.tg_row[g] >= 0)
      for (int32_t pos : C.tg_unreg[g]) hcx[(size_t)C.tg_row[g] * E + pos] = 255;
  return 0;
}

// The verdict kernels' gathers (drift_verdict_kernel, validate_verdict_kernel), uploaded once per superset Solve: pod
// kind and cluster pod per superset pod, the "not initialized" byte per existing position
static int32_t RecordTables(kp_ctx* ctx, GeneralBatch& gb, const kp_cluster& cl) {
  if (gb.rec_tab.p) return KP_OK;
  const size_t P = gb.pod_kind.size(), E = gb.pos_node.size();
  const size_t o_cl = (P + 255) & ~(size_t)255, o_un = (o_cl + sizeof(int32_t) * P + 255) & ~(size_t)255;
  vector<uint8_t> h(o_un + std::max<size_t>(E, 1), 0);
  if (P) memcpy(h.data(), gb.pod_kind.data(), P);
  if (P) memcpy(h.data() + o_cl, gb.pod_cluster.data(), sizeof(int32_t) * P);
  for (size_t e = 0; e < E; e++) h[o_un + e] = cl.nodes[gb.pos_node[e]].node.initialized ? 0 : 1;
  HIPCHK(gb.rec_tab.alloc(h.size()));
  HIPCHK(hipMemcpyAsync(gb.rec_tab.p, h.data(), h.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const uint8_t* d = (const uint8_t*)gb.rec_tab.p;
  gb.d_pod_kind = d;
  gb.d_pod_cluster = reinterpret_cast<const int32_t*>(d + o_cl);
  gb.d_pos_uninit = d + o_un;
  return KP_OK;
}

// The simulation's input order and existing-node index, as kp_abi.h states them for kp_cluster_drift's replacements and
// kp_cluster_command's commands: pending pods, the deleting nodes' pods in node order, the subset's pods in subset
// order; the nodes neither in the subset nor being deleted, in cluster order.
struct CommandIndex {
  const kp_cluster& cl;
  vector<int32_t> pod_idx;     // [P] input index of a queued pod, -1
  vector<int32_t> del_before;  // [N + 1] deleting nodes before node i
  vector<uint32_t> sorted;     // the current subset's nodes, ascending
  vector<uint32_t> cand_pods;
  int n_base = 0;
  explicit CommandIndex(const kp_cluster& c) : cl(c), pod_idx(std::max<uint32_t>(c.n_pods, 1), -1), del_before(c.n_nodes + 1, 0) {
    for (uint32_t j = 0; j < cl.n_pending; j++) pod_idx[cl.pending_pods[j]] = n_base++;
    for (uint32_t i = 0; i < cl.n_nodes; i++) {
      del_before[i + 1] = del_before[i] + (cl.nodes[i].deleting ? 1 : 0);
      if (cl.nodes[i].deleting)
        for (uint32_t j = 0; j < cl.nodes[i].n_pods; j++) pod_idx[cl.nodes[i].pods[j]] = n_base++;
    }
  }
  int Enter(const uint32_t* cand, uint32_t n) {  // -> pods queued
    sorted.assign(cand, cand + n);
    std::sort(sorted.begin(), sorted.end());
    int k = n_base;
    for (uint32_t i = 0; i < n; i++)
      for (uint32_t j = 0; j < cl.nodes[cand[i]].n_pods; j++) {
        cand_pods.push_back(cl.nodes[cand[i]].pods[j]);
        pod_idx[cand_pods.back()] = k++;
      }
    return k;
  }
  void Leave() {
    for (uint32_t p : cand_pods) pod_idx[p] = -1;
    cand_pods.clear();
  }
  int Existing(uint32_t node) const {  // -1: in the subset or being deleted
    if (node >= cl.n_nodes || cl.nodes[node].deleting) return -1;
    auto it = std::lower_bound(sorted.begin(), sorted.end(), node);
    if (it != sorted.end() && *it == node) return -1;
    return (int)node - del_before[node] - (int)(it - sorted.begin());
  }
};

// The Solve result of simulation j of a finished launch, read from its arena (still resident: the slot is reused by
// the launch after the next, which is not queued yet): what kp_solve_run copies back, in the indices of
// kp_cluster_drift's replacements and kp_cluster_command's commands (pods in the simulation's input order, existing
// nodes among those neither in the subset nor being deleted).
static int32_t ArenaSolveResult(kp_cluster_plan* plan, GeneralBatch& gb, const GenSlot& sl, int j, const vector<uint32_t>& cand,
                                std::unique_ptr<kp_solve_result>& out) {
  kp_ctx* ctx = plan->ctx;
  const kp_cluster& cl = plan->cluster()->cl;
  const Compiled& C = *gb.C;
  const SolveOffs& o = gb.o;
  const int Pc = gb.Pc, opt_stride = gb.opt_stride;
  const uint8_t* ar = (const uint8_t*)sl.arenas.p + gb.stride * (size_t)j;
  const vector<int32_t>& q = sl.queues[j];
  hipStream_t st = ctx->stream;
  uint64_t stats[KP_SOLVE_STATS];
  HIPCHK(hipMemcpyAsync(stats, ar + o.stats, sizeof stats, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int P = (int)q.size();
  if (P > Pc) return fail(KP_E_DEVICE, "drift result: %d pods in an arena of %d", P, Pc);
  ArenaResult a;
  const ResultOffs ro{o.place, o.events, o.nct, o.ncrq, o.opts, o.nrem, o.nopt, o.ncr, o.held};
  if (int32_t rc = FetchArenaResult(st, ar, ro, Pc, opt_stride, gb.res_mode != 0, (int)stats[3], a)) return rc;
  CommandIndex ix(cl);  // (queue position -> superset pod -> cluster pod -> input index)
  ix.Enter(cand.data(), (uint32_t)cand.size());
  auto res = std::make_unique<kp_solve_result>();
  if (int32_t rc = AssembleResult(*C.B, stats, a, P, opt_stride, [&](int p) { return ix.pod_idx[gb.pod_cluster[q[p]]]; },
                                  [&](int pos) { return pos < (int)gb.pos_node.size() ? ix.Existing((uint32_t)gb.pos_node[pos]) : -1; }, *res))
    return rc;
  memset(&res->stats, 0, sizeof res->stats);
  res->stats.attempts = stats[0];
  res->stats.bytes_algorithmic = stats[1];
  res->stats.pops = stats[2];
  res->stats.scanned = stats[5];
  res->stats.cursor_starts = stats[6];
  res->stats.prepare_ms = plan->prepare_ms;
  out = std::move(res);
  return KP_OK;
}

// ---- the launch loop (GeneralBatchRun) and its result modes: consolidation decisions and commands, drift verdicts,
// the validation of commands ------------------------------------------------------------------------------------
// What one GeneralBatchRun call fixes before its first launch, and its host argument blocks
struct GenRun {
  GeneralBatch& gb;
  const vector<vector<uint32_t>>& cands;
  vector<int> order;   // the call's subsets, longest simulations first; a launch takes order[b0 .. b0 + n)
  vector<size_t> len;  // per subset: the pods it queues
  int Pc = 64;            // the arena size in pods
  size_t per_launch = 1;  // simulations per launch
  hipStream_t up = nullptr, dn = nullptr;  // the copy streams
  vector<SolveArgs> sargs;                 // the launch being queued: [0] holds the tables every simulation shares
  vector<FinalizeArgs> fargs;
  // a consolidation launch's results in the slot's pinned download buffer
  size_t r_stats = 0, r_place = 0, r_nct = 0, r_nopt = 0, r_opts = 0, r_fin = 0, r_held = 0, r_end = 0;
  // the slot's pinned upload buffer: overlays, the two argument blocks, the record-modes' mirror of the record buffer
  size_t u_args = 0, u_fargs = 0, u_end = 0, u_rec = 0;
  // the slot's record buffer: queue pods [n][Pc], lengths [n], caller indices [n], then the record
  size_t d_qlen = 0, d_cidx = 0, d_rec = 0;
};
// The hooks run in this order for a launch on slot sl (which holds its n, b0, kernel stream and device arguments)
struct GeneralMode {
  kp_cluster_plan* plan;
  GenTotals& T;
  kp_cancel* cancel;
  int32_t stop_nc;  // SolveArgs::stop_nc: the NodeClaim count that ends a simulation's Solve (0: the whole Solve)
  GeneralMode(kp_cluster_plan* p, GenTotals& t, kp_cancel* c, int32_t stop) : plan(p), T(t), cancel(c), stop_nc(stop) {}
  virtual ~GeneralMode() = default;
  virtual hipError_t Reserve(const GenRun& R, GenSlot& sl) = 0;      // the slot's pinned buffers (and the mode's own), sized
  virtual int32_t Upload(const GenRun&, GenSlot&) { return KP_OK; }  // the mode's uploads, on R.up behind the arguments
  virtual int32_t Enqueue(const GenRun& R, GenSlot& sl) = 0;         // its kernels, on sl.ks behind launch_solve_batch
  virtual int32_t Download(const GenRun& R, GenSlot& sl) = 0;        // its downloads into sl.down, on R.dn
  // the launch has finished: its results are in sl.down, its arenas resident until the launch after the next is queued
  virtual int32_t Decide(const GenRun& R, GenSlot& sl) = 0;
  // subset s compiled and solved on its own (not batchable, or no room for the arenas)
  virtual int32_t SimOne(const vector<uint32_t>& cand, int s) = 0;
};

// kp_cluster_simulate / kp_cluster_command: the decision per subset on the host, from the launch's downloaded results;
// commands (or null): the command of every subset that decided DELETE or REPLACE
struct ConsolidateMode final : GeneralMode {
  const vector<std::map<string, string>>& labels;
  int32_t multi_node;
  vector<SimOut>& outs;
  kp_solve_result** commands;
  kp_sim_why* whys;  // kp_cluster_simulate_explained (or null): the reason record of every subset
  ConsolidateMode(kp_cluster_plan* p, GenTotals& t, kp_cancel* c, const vector<std::map<string, string>>& l, int32_t mn,
                  vector<SimOut>& o, kp_solve_result** cmds, kp_sim_why* w = nullptr)
      : GeneralMode(p, t, c, 2), labels(l), multi_node(mn), outs(o), commands(cmds), whys(w) {}  // (a second NodeClaim: no-op)
  hipError_t Reserve(const GenRun& R, GenSlot& sl) override {
    const hipError_t e = sl.up.reserve(R.u_end);
    return e != hipSuccess ? e : sl.down.reserve(R.r_end);
  }
  int32_t Enqueue(const GenRun& R, GenSlot& sl) override {
    HIPCHK(launch_finalize_batch(R.fargs[0], sl.dfargs, sl.n, sl.ks));
    return KP_OK;
  }
  int32_t Download(const GenRun& R, GenSlot& sl) override {
    const GeneralBatch& gb = R.gb;
    const SolveOffs& o = gb.o;
    auto down = [&](size_t roff, size_t off, size_t width) {
      return hipMemcpy2DAsync(sl.down.at(roff), width, (const uint8_t*)sl.arenas.p + off, gb.stride, width, sl.n,
                              hipMemcpyDeviceToHost, R.dn);
    };
    HIPCHK(down(R.r_stats, o.stats, sizeof(uint64_t) * KP_SOLVE_STATS));
    HIPCHK(down(R.r_place, o.place, sizeof(int32_t) * R.Pc));
    HIPCHK(down(R.r_nct, o.nct, sizeof(int32_t)));
    HIPCHK(down(R.r_nopt, o.nopt, sizeof(uint32_t)));
    HIPCHK(down(R.r_opts, o.opts, sizeof(uint32_t) * gb.opt_stride));
    HIPCHK(down(R.r_fin, o.ncr, sizeof(KReqs)));
    if (gb.res_mode) HIPCHK(down(R.r_held, o.held, sizeof(uint64_t)));
    return KP_OK;
  }
  int32_t Decide(const GenRun& R, GenSlot& sl) override {
    GeneralBatch& gb = R.gb;
    const Compiled& C = *gb.C;
    const kp_cluster& cl = plan->cluster()->cl;
    const int n = sl.n, Pc = R.Pc;
    const size_t b0 = sl.b0;
    const uint64_t* stats = reinterpret_cast<uint64_t*>(sl.down.at(R.r_stats));
    const int32_t* place = reinterpret_cast<int32_t*>(sl.down.at(R.r_place));
    const int32_t* nct = reinterpret_cast<int32_t*>(sl.down.at(R.r_nct));
    const uint32_t* nopt = reinterpret_cast<uint32_t*>(sl.down.at(R.r_nopt));
    uint32_t* opts = reinterpret_cast<uint32_t*>(sl.down.at(R.r_opts));
    const KReqs* fin = reinterpret_cast<KReqs*>(sl.down.at(R.r_fin));
    const uint64_t* held = reinterpret_cast<uint64_t*>(sl.down.at(R.r_held));
    std::atomic<int> bad_runaway{-1}, cancelled{0};
    uint64_t tcount[kMaxHostThreads][3] = {}, tphase[kMaxHostThreads][8] = {};
    // kp_cluster_command: the options each decision kept and whether it was taken as spot-to-spot
    vector<vector<int>> keptv(commands ? n : 0);
    vector<uint8_t> s2sv(commands ? n : 0, 0);
    ParallelFor(n, [&](int j_lo, int j_hi, int t) {
    for (int j = j_lo; j < j_hi; j++) {
      const int i = R.order[b0 + j];
      const uint64_t* sj = &stats[(size_t)j * KP_SOLVE_STATS];
      if (sj[7]) {
        bad_runaway = i;
        return;
      }
      if (sj[46]) {
        cancelled = 1;
        return;
      }
      for (int k = 0; k < 3; k++) tcount[t][k] += sj[k];
      for (int k = 0; k < 8; k++) tphase[t][k] += sj[8 + k];  // (zero unless kp_overrides.timing)
      const int n_nc = (int)sj[3];
      const vector<int32_t>& q = sl.queues[j];
      SimOut& out = outs[i];
      out.n_pods = (uint32_t)q.size();
      bool all = true;  // (a no-op at the first failure)
      for (size_t p = 0; p < q.size() && all; p++)
        all = !PodUnscheduled(gb.pod_kind[q[p]], place[(size_t)j * Pc + p],
                              [&](int pos) { return cl.nodes[gb.pos_node[pos]].node.initialized != 0; });
      KReqs Rq = fin[j];
      int ci = 0;
      uint32_t np = 0;
      if (n_nc == 1) {
        if (gb.res_mode) ApplyHeld(*C.B, held[j], Rq);
        ci = C.B->tmpl_catalog[nct[j]];
        np = (uint32_t)C.B->tmpl_nodepool[nct[j]];
      }
      bool s2s = false;
      WhySolve ws;
      if (whys) {  // the Solve's fields from the downloaded placements, queue positions ascending (scan_unscheduled's rule)
        kp_sim_why* w = ws.why = &whys[i];
        WhyClear(w);
        w->n_nodeclaims = (uint32_t)std::min(n_nc, 2);
        for (size_t p = 0; p < q.size(); p++) {
          const int kind = gb.pod_kind[q[p]];
          const int32_t pl = place[(size_t)j * Pc + p];
          if (PodUnscheduled(kind, pl, [&](int pos) { return cl.nodes[gb.pos_node[pos]].node.initialized != 0; })) {
            if (w->n_unscheduled++ == 0) w->first_unscheduled = gb.pod_cluster[q[p]], ws.bad_pos = (int64_t)p;
          } else if (kind != 2 && pl >= 0) {
            if (ws.nc_np++ == 0) ws.nc_pod = gb.pod_cluster[q[p]], ws.nc_pos = (int64_t)p;
          }
        }
      }
      GeneralDecide(cl, labels, R.cands[i], *C.B, all, n_nc, &Rq, ci, np, &opts[(size_t)j * gb.opt_stride],
                    n_nc == 1 ? nopt[j] : 0, multi_node, out, &gb.offers, &gb.cands, commands ? &keptv[j] : nullptr, &s2s,
                    whys ? &ws : nullptr);
      if (commands) s2sv[j] = s2s ? 1 : 0;
    }
    });
    for (int t = 0; t < kMaxHostThreads; t++) {
      for (int k = 0; k < 3; k++) T.counters[k] += tcount[t][k];
      for (int k = 0; k < 8; k++) plan->general_phase[k] += tphase[t][k];
    }
    if (bad_runaway >= 0)
      return fail(KP_E_DEVICE, "solve_kernel exceeded its Queue.Pop bound in simulation %d: aborted", bad_runaway.load());
    if (cancelled) return fail(KP_E_CANCELED, "consolidation simulations cancelled (kp_cancel_set)");
    // kp_cluster_command: the command of every simulation that decided DELETE or REPLACE, from its arena while the
    // slot still holds it, as drift reads its winner (ArenaSolveResult), then cut to the options the decision kept. A
    // simulation that stopped at its second NodeClaim decided no-op and is not read.
    for (int j = 0; commands && j < n; j++) {
      const int i = R.order[b0 + j];
      if (outs[i].decision == KP_DECISION_NOOP) continue;
      std::unique_ptr<kp_solve_result> res;
      if (int32_t rc = ArenaSolveResult(plan, gb, sl, j, R.cands[i], res)) return rc;
      const bool replace = outs[i].decision == KP_DECISION_REPLACE;
      if (res->ncs.size() != (replace ? 1u : 0u))
        return fail(KP_E_DEVICE, "command of subset %d: %zu NodeClaims in its arena", i, res->ncs.size());
      if (replace) CutToCommand(C.B->d, *res, keptv[j], s2sv[j] != 0);
      commands[i] = res.release();
    }
    return KP_OK;
  }
  int32_t SimOne(const vector<uint32_t>& cand, int s) override {
    return GeneralSimOne(plan, cand, labels, multi_node, outs[s], T, cancel, commands ? &commands[s] : nullptr,
                         whys ? &whys[s] : nullptr);
  }
};

// Per-subset verdicts of a record-mode call, caller order: the device array the launches' kernels write, and the
// entries taken on the host instead (subsets compiled on their own)
extern "C++" template <class Out>
struct Verdicts {
  vector<Out> host;
  vector<char> on_host;
  Out* dev = nullptr;  // [n_subsets]
  explicit Verdicts(uint32_t n) : host(n, Out{}), on_host(n, 0) {}
  Out& OnHost(int s) {
    on_host[s] = 1;
    return host[s];
  }
  // the verdicts of every launch: one copy (the launches have drained: their records were read); the host's entries stay
  int32_t Merge(hipStream_t st, const vector<int>& batched) {
    vector<Out> got(host.size());
    HIPCHK(hipMemcpyAsync(got.data(), dev, sizeof(Out) * got.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int s : batched)
      if (!on_host[s]) host[s] = got[s];
    return KP_OK;
  }
  // the call's answer: the budget-blocked subsets (never simulated) get `stamp`
  void Emit(const vector<char>& blocked, const Out& stamp, void* out) {
    for (size_t s = 0; s < host.size(); s++)
      if (blocked[s]) host[s] = stamp;
    if (out && !host.empty()) memcpy(out, host.data(), sizeof(Out) * host.size());
  }
};

// Drift and validation: the verdicts stay on the device (Verdicts::dev) and a launch downloads one record. The slot's
// record buffer holds the simulations' queue pods [n][Pc], lengths [n] and caller indices [n], then the record; the
// upload buffer mirrors it behind the arguments. (DriftArgs / DriftRec: kp_device.h's names for the record-mode
// arguments and the launch's record, whichever mode fills them.)
struct RecordMode : GeneralMode {
  const char* what;  // the cancellation message's word
  DriftArgs da;      // the launch being queued (Upload fills it; Enqueue and Download read it)
  RecordMode(kp_cluster_plan* p, GenTotals& t, kp_cancel* c, int32_t stop, const char* w) : GeneralMode(p, t, c, stop), what(w) {}
  hipError_t Reserve(const GenRun& R, GenSlot& sl) override {
    hipError_t e = sl.up.reserve(R.u_rec + R.d_rec);
    if (e == hipSuccess) e = sl.down.reserve(sizeof(DriftRec));
    if (e == hipSuccess && sl.rec_bytes < R.d_rec + sizeof(DriftRec)) {
      e = sl.rec.alloc(R.d_rec + sizeof(DriftRec));
      sl.rec_bytes = e == hipSuccess ? R.d_rec + sizeof(DriftRec) : 0;
    }
    return e;
  }
  int32_t Upload(const GenRun& R, GenSlot& sl) override {
    const GeneralBatch& gb = R.gb;
    const int n = sl.n, Pc = R.Pc;
    uint8_t* hd = sl.up.at(R.u_rec);
    uint8_t* dd = (uint8_t*)sl.rec.p;
    int32_t* qpod = reinterpret_cast<int32_t*>(hd);
    int32_t* qlen = reinterpret_cast<int32_t*>(hd + R.d_qlen);
    int32_t* cidx = reinterpret_cast<int32_t*>(hd + R.d_cidx);
    for (int j = 0; j < n; j++) {
      const vector<int32_t>& q = sl.queues[j];
      memcpy(qpod + (size_t)j * Pc, q.data(), sizeof(int32_t) * q.size());
      qlen[j] = (int32_t)q.size();
      cidx[j] = R.order[sl.b0 + j];
    }
    HIPCHK(hipMemcpyAsync(dd, hd, sizeof(int32_t) * (size_t)Pc * n, hipMemcpyHostToDevice, R.up));
    HIPCHK(hipMemcpyAsync(dd + R.d_qlen, hd + R.d_qlen, sizeof(int32_t) * n, hipMemcpyHostToDevice, R.up));
    HIPCHK(hipMemcpyAsync(dd + R.d_cidx, hd + R.d_cidx, sizeof(int32_t) * n, hipMemcpyHostToDevice, R.up));
    memset(&da, 0, sizeof da);
    da.n = n;
    da.Pc = Pc;
    da.n_existing = (int32_t)gb.C->ex_input.size();
    da.n_super = (int32_t)gb.pod_kind.size();
    da.arenas = (uint8_t*)sl.arenas.p;
    da.stride = gb.stride;
    da.off_place = gb.o.place;
    da.off_stats = gb.o.stats;
    da.qpod = reinterpret_cast<const int32_t*>(dd);
    da.qlen = reinterpret_cast<const int32_t*>(dd + R.d_qlen);
    da.cidx = reinterpret_cast<const int32_t*>(dd + R.d_cidx);
    da.pod_kind = gb.d_pod_kind;
    da.pod_cluster = gb.d_pod_cluster;
    da.pos_uninit = gb.d_pos_uninit;
    da.rec = reinterpret_cast<DriftRec*>(dd + R.d_rec);
    return KP_OK;
  }
  int32_t Download(const GenRun& R, GenSlot& sl) override {  // the record only (the verdicts: Verdicts::Merge)
    HIPCHK(hipMemcpyAsync(sl.down.at(0), da.rec, sizeof(DriftRec), hipMemcpyDeviceToHost, R.dn));
    return KP_OK;
  }
  static const DriftRec& Record(const GenSlot& sl) { return *reinterpret_cast<const DriftRec*>(sl.down.at(0)); }
  int32_t Decide(const GenRun&, GenSlot& sl) override {  // the launch's record: counters, a runaway Solve, cancellation
    const DriftRec& rec = Record(sl);
    T.counters[0] += rec.attempts;
    T.counters[1] += rec.bytes;
    T.counters[2] += rec.pops;
    if (rec.runaway >= 0)
      return fail(KP_E_DEVICE, "solve_kernel exceeded its Queue.Pop bound in simulation %lld: aborted", (long long)rec.runaway);
    if (rec.cancelled) return fail(KP_E_CANCELED, "%s simulations cancelled (kp_cancel_set)", what);
    return KP_OK;
  }
};

// kp_cluster_drift: every Solve runs whole; a launch leaves AllNonPendingPodsScheduled per subset in the verdict array
// and, in its record, its lowest feasible subset, whose NodeClaims it finalizes; the host fetches that result when it
// lowers the call's first
struct DriftMode final : RecordMode {
  Verdicts<DriftOut> v;
  int64_t first = -1;                    // the lowest feasible caller-order subset so far
  std::unique_ptr<kp_solve_result> res;  // its Solve result
  DriftMode(kp_cluster_plan* p, GenTotals& t, kp_cancel* c, uint32_t n_subsets) : RecordMode(p, t, c, 0, "drift"), v(n_subsets) {}
  int32_t Enqueue(const GenRun& R, GenSlot& sl) override {
    // the verdicts, the launch's record, then every NodeClaim of its first feasible simulation finalized while the
    // arena is resident (at most as many as the launch's longest queue, its first simulation's)
    da.out = v.dev;
    HIPCHK(launch_drift_verdict(da, sl.ks));
    HIPCHK(launch_drift_first(da, sl.ks));
    HIPCHK(launch_finalize_drift(sl.dfargs, da.rec, std::max(1, std::min(R.Pc, (int)R.len[R.order[sl.b0]])), sl.ks));
    return KP_OK;
  }
  int32_t Decide(const GenRun& R, GenSlot& sl) override {
    if (int32_t rc = RecordMode::Decide(R, sl)) return rc;
    const DriftRec& rec = Record(sl);
    if (rec.first >= 0 && (first < 0 || rec.first < first)) {
      if (rec.local < 0 || rec.local >= sl.n || R.order[sl.b0 + (size_t)rec.local] != rec.first)
        return fail(KP_E_DEVICE, "drift record: simulation %lld of the launch is not subset %lld", (long long)rec.local,
                    (long long)rec.first);
      if (int32_t rc = ArenaSolveResult(plan, R.gb, sl, (int)rec.local, R.cands[rec.first], res)) return rc;
      first = rec.first;
    }
    return KP_OK;
  }
  // the verdict from the subset's own Solve (queue order: the Solve's own)
  int32_t SimOne(const vector<uint32_t>& cand, int s) override {
    SimOneSolve so;
    if (int32_t rc = GeneralSolveOne(plan, cand, so, T, cancel)) return rc;
    const kp_solve_result* r = so.res.get();
    DriftOut o;
    memset(&o, 0, sizeof o);
    o.n_nodeclaims = (uint32_t)r->ncs.size();
    o.n_pods = (uint32_t)so.kind.size();
    o.first_unscheduled = -1;
    for (int32_t p : so.sp->cp->queue)
      if (PodUnscheduled(so.kind[p], r->placement[p], [&](int pos) { return so.ex[(size_t)pos].initialized != 0; }))
        if (o.n_unscheduled++ == 0) o.first_unscheduled = (int32_t)so.cluster_pod[p];
    o.feasible = o.n_unscheduled == 0 ? 1 : 0;
    v.OnHost(s) = o;
    if (o.feasible && (first < 0 || s < first)) {
      first = s;
      res.reset(so.res.release());
    }
    return KP_OK;
  }
};

// kp_cluster_validate: the Solves stop at the second NodeClaim and are finalized as the consolidation launches are,
// then validate_verdict_kernel (and validate_sum_kernel) leave the verdicts and the launch's record
struct ValidateMode final : RecordMode {
  const kp_command_check* checks;
  vector<vector<string>> names;  // per subset: the check's names as a set (CheckNames)
  Verdicts<ValOut> v;
  const uint64_t* d_want = nullptr;  // the compiled checks on the device (ValidateCompile)
  const uint32_t* d_unknown = nullptr;
  const uint8_t* d_replace = nullptr;
  ValidateMode(kp_cluster_plan* p, GenTotals& t, kp_cancel* c, const kp_command_check* ch, uint32_t n_subsets)
      : RecordMode(p, t, c, 2, "validation"), checks(ch), names(n_subsets), v(n_subsets) {}
  int32_t Enqueue(const GenRun& R, GenSlot& sl) override {
    const GeneralBatch& gb = R.gb;
    const SolveOffs& o = gb.o;
    const SolveArgs& a0 = R.sargs[0];
    HIPCHK(launch_finalize_batch(R.fargs[0], sl.dfargs, sl.n, sl.ks));
    ValidateArgs va;
    memset(&va, 0, sizeof va);
    va.d = da;
    va.off_nct = o.nct, va.off_nopt = o.nopt, va.off_opts = o.opts, va.off_ncr = o.ncr;
    va.opt_stride = gb.opt_stride;
    va.n_tmpl = (int32_t)gb.C->B->tmpl_catalog.size();
    va.n_catalogs = (int32_t)gb.C->B->cats.size();
    va.dict = a0.dict;
    va.cats = a0.cats;
    va.tmpl_catalog = a0.tmpl_catalog;
    va.want = d_want;
    va.unknown = d_unknown;
    va.replace = d_replace;
    va.out = v.dev;
    HIPCHK(launch_validate_verdict(va, sl.ks));
    return KP_OK;
  }
  // The rule applied on the host to the subset's own whole Solve (GeneralSolveOne). kp_solve_run has applied the held
  // reservations and Truncate's minValues check to the NodeClaim (HostMinValuesOK: options cleared, pods unplaced).
  int32_t SimOne(const vector<uint32_t>& cand, int s) override {
    SimOneSolve so;
    if (int32_t rc = GeneralSolveOne(plan, cand, so, T, cancel)) return rc;
    const kp_cluster& cl = plan->cluster()->cl;
    const kp_solve_result* res = so.res.get();
    const bool repl = checks[s].decision == KP_DECISION_REPLACE;
    ValOut& o = v.OnHost(s);
    memset(&o, 0, sizeof o);
    o.n_pods = (uint32_t)so.kind.size();
    if (res->ncs.size() > 1) {
      o.verdict = KP_INVALID_MULTIPLE;
      o.n_nodeclaims = 2;
      return KP_OK;
    }
    o.n_nodeclaims = (uint32_t)res->ncs.size();
    for (size_t p = 0; p < so.kind.size(); p++)
      if (PodUnscheduled(so.kind[p], res->placement[p], [&](int pos) { return so.ex[(size_t)pos].initialized != 0; }))
        o.n_unscheduled++;
    if (o.n_unscheduled) {
      o.verdict = KP_INVALID_UNSCHEDULED;
    } else if (res->ncs.empty()) {
      o.verdict = repl ? KP_INVALID_NO_REPLACEMENT_NEEDED : KP_VALID;
    } else if (!repl) {
      o.verdict = KP_INVALID_NEEDS_REPLACEMENT;
    } else {
      const vector<HostType>& types = cl.catalogs[res->nc_cat[0]]->types;
      std::set<string> have;
      for (uint32_t t : res->ncs[0].options)
        if (t < types.size()) have.insert(types[t].name);
      for (const string& nm : names[s])
        if (!have.count(nm)) o.n_missing++;
      o.verdict = o.n_missing ? KP_INVALID_NOT_SUBSET : KP_VALID;
    }
    return KP_OK;
  }
};

// Runs the batchable subsets `idx` (their candidate lists in cands) as batched Solves, pipelined over the plan's two
// launch slots; what the launches leave behind is the mode's.
static int32_t GeneralBatchRun(GeneralBatch& gb, const vector<vector<uint32_t>>& cands, const vector<int>& idx,
                               GeneralMode& mode) {
  kp_cluster_plan* plan = mode.plan;
  GenTotals& T = mode.T;
  kp_cancel* cancel = mode.cancel;
  kp_ctx* ctx = plan->ctx;
  const kp_cluster& cl = plan->cluster()->cl;
  const Compiled& C = *gb.C;
  hipStream_t st = ctx->stream;
  // kp_cancel: solve_kernel polls the flag (every ~1,024 pops of each simulation) and the host reads it before each
  // launch; any early return (cancellation, an error) first drains the launches this call queued
  const int32_t* dcancel = nullptr;
  if (cancel) {
    void* dp = nullptr;
    HIPCHK(hipHostGetDevicePointer(&dp, cancel->flag, 0));
    dcancel = (const int32_t*)dp;
  }
  struct Drain {
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
  } drain{st};
  // the arena size: every simulation of the batch fits (rounded up, so that nearby batches share a layout)
  GenRun R{gb, cands, idx, vector<size_t>(cands.size(), 0)};
  size_t max_pods = 1;
  for (int i : idx) {
    size_t n = gb.base_pods.size();
    for (uint32_t c : cands[i]) n += gb.node_pods[c].size();
    R.len[i] = n;
    max_pods = std::max(max_pods, n);
  }
  while ((size_t)R.Pc < max_pods) R.Pc *= 2;
  const int Pc = R.Pc;
  if (int32_t rc = GeneralBatchLayout(ctx, gb, Pc)) return rc;
  const SolveOffs& o = gb.o;
  const size_t patch_bytes = o.common;
  // simulations per launch: two launch slots (the host prepares one while the device runs the other), each at most
  // an eighth of the free device memory in arenas and 4096 simulations (one Solve workgroup per CU runs at a time;
  // the rest queue behind it)
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)8 << 30;
  const size_t held_b = gb.slot[0].arenas_bytes + gb.slot[1].arenas_bytes;
  const size_t budget = std::max<size_t>((free_b + held_b) / 8, (size_t)1 << 30);
  size_t per_launch = std::max<size_t>(1, std::min<size_t>(4096, budget / gb.stride));
  if (idx.size() > per_launch && idx.size() < 2 * per_launch) per_launch = (idx.size() + 1) / 2;  // two even launches
  // kp_overrides.general_launch (read now, not when the plan was prepared): small batches reach the reused arenas
  if (ctx->ov.general_launch > 0) per_launch = std::min<size_t>(per_launch, (size_t)ctx->ov.general_launch);
  R.per_launch = per_launch;
  // longest simulations first (queue length: pending + the candidates' pods): they start on the first CUs instead
  // of trailing the launch
  const vector<int>& order = R.order;
  std::stable_sort(R.order.begin(), R.order.end(), [&](int x, int y) { return R.len[x] > R.len[y]; });
  if (ctx->ov.host_timing)
    fprintf(stderr, "[kp general] arena stride %.2f MB, %zu simulations per launch, Pc %d; batch_init per simulation: copy %zu B, "
            "fills stats %zu npods %zu place %zu ver %zu fail %zu hcnc %zu B\n", gb.stride / 1e6, per_launch, Pc,
            gb.o.exr - gb.o.common - (__builtin_popcount(gb.rmask) <= 4 ? gb.o.exroom - gb.o.exrq : 0),
            sizeof(uint64_t) * KP_SOLVE_STATS, sizeof(int32_t) * (size_t)Pc, sizeof(int32_t) * (size_t)Pc,
            gb.o.ver_end - gb.o.ver0, gb.o.fail_end - gb.o.fail0, gb.o.n_hcnc);
  const int sort_cap = std::min(SortCapacity(C.ov), Pc);
  const size_t dyn = std::max<size_t>((size_t)2 * sort_cap * sizeof(int32_t), o.chk_on ? CHK_LDS_BYTES : 0);
  vector<GenScratch> scratches(kMaxHostThreads);
  vector<SolveArgs>& sargs = R.sargs;
  vector<FinalizeArgs>& fargs = R.fargs;
  R.r_place = R.r_stats + sizeof(uint64_t) * KP_SOLVE_STATS * per_launch;
  R.r_nct = R.r_place + sizeof(int32_t) * (size_t)Pc * per_launch;
  R.r_nopt = R.r_nct + sizeof(int32_t) * per_launch;
  R.r_opts = R.r_nopt + sizeof(uint32_t) * per_launch;
  R.r_fin = (R.r_opts + sizeof(uint32_t) * (size_t)gb.opt_stride * per_launch + 63) & ~(size_t)63;
  R.r_held = R.r_fin + sizeof(KReqs) * per_launch;
  R.r_end = R.r_held + sizeof(uint64_t) * per_launch;
  R.u_args = (patch_bytes * per_launch + 255) & ~(size_t)255;
  R.u_fargs = R.u_args + ((sizeof(SolveArgs) * per_launch + 255) & ~(size_t)255);
  R.u_end = R.u_fargs + sizeof(FinalizeArgs) * per_launch;
  R.u_rec = (R.u_end + 255) & ~(size_t)255;
  R.d_qlen = sizeof(int32_t) * (size_t)Pc * per_launch;
  R.d_cidx = R.d_qlen + sizeof(int32_t) * per_launch;
  R.d_rec = (R.d_cidx + sizeof(int32_t) * per_launch + 255) & ~(size_t)255;

  // a finished launch: its results have landed; its kernels' time; then the mode's decisions
  auto decide = [&](GenSlot& sl) -> int32_t {
    HIPCHK(hipEventSynchronize(sl.done));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, sl.t0, sl.t1));
    T.dev_ms += ms;
    const auto th1 = std::chrono::steady_clock::now();
    if (int32_t rc = mode.Decide(R, sl)) return rc;
    T.host_ms[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th1).count();
    return KP_OK;
  };

  GenSlot* slots = gb.slot;
  for (int k = 0; k < 2; k++)
    if (!slots[k].done) {
      HIPCHK(hipEventCreateWithFlags(&slots[k].done, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&slots[k].uploaded, hipEventDisableTiming));
      HIPCHK(hipEventCreate(&slots[k].t0));
      HIPCHK(hipEventCreate(&slots[k].t1));
    }
  if (!gb.cs.up)
    for (hipStream_t* x : {&gb.cs.up, &gb.cs.down, &gb.cs.k[0], &gb.cs.k[1]})
      HIPCHK(hipStreamCreateWithFlags(x, hipStreamNonBlocking));
  hipStream_t up = R.up = gb.cs.up, dn = R.dn = gb.cs.down;
  slots[0].ks = gb.cs.k[0], slots[1].ks = gb.cs.k[1];
  struct DrainCopies {  // (early returns: nothing left in flight on the copy or kernel streams either)
    hipStream_t u, d, k0, k1;
    ~DrainCopies() {
      for (hipStream_t x : {k0, k1, u, d}) (void)hipStreamSynchronize(x);
    }
  } drain_copies{up, dn, gb.cs.k[0], gb.cs.k[1]};
  int pending = -1;  // the slot whose launch is in flight and not yet decided
  int launch_no = 0;
  for (size_t b0 = 0; b0 < idx.size(); b0 += per_launch, launch_no++) {
    if (cancel && __atomic_load_n(cancel->flag, __ATOMIC_SEQ_CST))
      return fail(KP_E_CANCELED, "consolidation simulations cancelled (kp_cancel_set) after %zu of %zu", b0, idx.size());
    GenSlot& sl = slots[launch_no & 1];
    const auto th0 = std::chrono::steady_clock::now();
    const int n = (int)std::min(per_launch, idx.size() - b0);
    // arenas for this launch's n simulations, grown geometrically (a few subsets do not pin gigabytes on the plan);
    // when the device cannot hold them, this batch and the rest run one simulation at a time (the mode's SimOne)
    hipError_t ae = hipSuccess;
    if (sl.arenas_bytes < gb.stride * n) {
      const size_t sims = std::min(per_launch, std::max<size_t>((size_t)n, 2 * sl.arenas_bytes / gb.stride));
      ae = sl.arenas.alloc(gb.stride * sims);
      sl.arenas_bytes = ae == hipSuccess ? gb.stride * sims : 0;
    }
    const size_t args_need = (sizeof(SolveArgs) + sizeof(FinalizeArgs)) * (size_t)n + 512;
    if (ae == hipSuccess && sl.args_bytes < args_need) {
      ae = sl.args.alloc(args_need);
      sl.args_bytes = ae == hipSuccess ? args_need : 0;
    }
    if (ae == hipSuccess) ae = mode.Reserve(R, sl);
    if (ae != hipSuccess) {
      (void)hipGetLastError();
      if (pending >= 0) {
        if (int32_t rc = decide(slots[pending])) return rc;
        pending = -1;
      }
      for (size_t j = b0; j < idx.size(); j++)
        if (int32_t rc = mode.SimOne(cands[order[j]], order[j])) return rc;
      break;
    }
    // (this slot's previous launch was decided before the launch in flight was queued)
    sl.n = n;
    sl.b0 = b0;
    uint8_t* arenas = (uint8_t*)sl.arenas.p;
    uint8_t* sh = (uint8_t*)gb.shared.p;
    uint8_t* patches = reinterpret_cast<uint8_t*>(sl.up.at(0));
    sl.queues.resize(n);
    vector<vector<int32_t>>& queues = sl.queues;
    sargs.resize(n);
    fargs.resize(n);
    std::atomic<int> unbatchable{-1};
    const bool ht = ctx->ov.host_timing != 0;
    double tpatch[kMaxHostThreads] = {};  // (kp_overrides.host_timing: the overlays' own share)
    ParallelFor(n, [&](int j_lo, int j_hi, int t) {
    for (int j = j_lo; j < j_hi; j++) {
      const int i = order[b0 + j];
      const auto tp0 = ht ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point{};
      if (GeneralPatch(gb, cl, cands[i], scratches[t], queues[j], patches + patch_bytes * j)) {
        unbatchable = i;
        return;
      }
      if (ht) tpatch[t] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp0).count();
      uint8_t* ar = arenas + gb.stride * j;
      SolveArgs& a = sargs[j];
      BindSolve(a, C, o, sh, ar, (int)queues[j].size(), Pc, gb.rmask, gb.res_mode);
      a.cancel = dcancel;
      a.stop_nc = mode.stop_nc;
      a.ex_reqs_ro = (const uint8_t*)gb.pristine.p + (o.exr - o.common);  // (the arena's copy is written on demand)
      a.ex_ulist = (const int32_t*)(sh + gb.so.exul);
      a.ex_ulist_off = (const int32_t*)(sh + gb.so.exuo);
      a.ex_uidx = (const int32_t*)(sh + gb.so.exui);
      if (gb.tfeas_on) {
        a.tfeas = (const uint64_t*)(sh + o.tfeas);
        a.tfeas_words = gb.tf_words;
      }
      FinalizeArgs& f = fargs[j];
      memset(&f, 0, sizeof f);
      f.dict = a.dict;
      f.cats = a.cats;
      f.vint = a.vint;
      f.nc_tmpl = a.nc_tmpl;
      f.tmpl_catalog = a.tmpl_catalog;
      f.nc_reqs = a.nc_reqs;
      f.nc_X = a.nc_X;
      f.max_types = 100;
      f.opt_stride = gb.opt_stride;
      f.out_options = (uint32_t*)(ar + o.opts);
      f.out_n_remaining = (uint32_t*)(ar + o.nrem);
      f.out_n_options = (uint32_t*)(ar + o.nopt);
      f.nc_held = a.res_mode ? a.nc_held : nullptr;
      f.solve_stats = a.stats;
    }
    });
    if (unbatchable >= 0) return fail(KP_E_INVAL, "subset %d: not batchable after the check", unbatchable.load());
    if (ht) {
      double tp = 0;
      for (double x : tpatch) tp += x;
      fprintf(stderr, "[kp general] launch %d: %d sims, patch %zu B each, GeneralPatch %.2f thread-ms, overlays %.2f ms\n",
              launch_no, n, patch_bytes, tp,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count());
    }
    memcpy(reinterpret_cast<uint8_t*>(sl.up.at(R.u_args)), sargs.data(), sizeof(SolveArgs) * n);
    memcpy(reinterpret_cast<uint8_t*>(sl.up.at(R.u_fargs)), fargs.data(), sizeof(FinalizeArgs) * n);
    SolveArgs* dargs = (SolveArgs*)sl.args.p;
    FinalizeArgs* dfargs = (FinalizeArgs*)((uint8_t*)sl.args.p + ((sizeof(SolveArgs) * n + 255) & ~(size_t)255));
    sl.dfargs = dfargs;
    BatchInitArgs bi;
    memset(&bi, 0, sizeof bi);
    bi.base = arenas;
    bi.stride = gb.stride;
    bi.pristine = (const uint8_t*)gb.pristine.p;
    bi.dst_off = o.common;
    bi.n_copy = (o.exr - o.common + 15) & ~(size_t)15;  // not the existing nodes' requirements: copy-on-write
    if (__builtin_popcount(gb.rmask) <= 4) {
      // the existing nodes' request rows are read only for a fifth requested resource and beyond (the first four are
      // their headroom rows); with four or fewer a commit's read-modify-write leaves the unread values unread
      bi.skip_off = o.exrq - o.common;
      bi.skip_len = (o.exroom - o.exrq) & ~(size_t)15;
    }
    auto fill = [&](size_t off, size_t len, uint32_t byte) {
      bi.fill_off[bi.n_fill] = off;
      bi.fill_len[bi.n_fill] = (len + 15) & ~(size_t)15;
      bi.fill_byte[bi.n_fill] = byte;
      bi.n_fill++;
    };
    fill(o.stats, sizeof(uint64_t) * KP_SOLVE_STATS, 0);
    fill(o.npods, sizeof(int32_t) * Pc, 0);
    fill(o.place, sizeof(int32_t) * Pc, 0xFF);
    fill(o.ver0, o.ver_end - o.ver0, 0);
    fill(o.fail0, o.fail_end - o.fail0, 0xFF);
    if (o.n_hcnc) fill(o.hcnc, o.n_hcnc, 0);
    T.host_ms[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count();
    // uploads on their own stream (they overlap the previous launch's kernels; this slot's arenas and buffers were
    // last used by the launch before that one, whose results decide() has already waited for); batch_init writes
    // [common, mut_end) of the arenas, the overlays [0, common)
    HIPCHK(hipMemcpy2DAsync(arenas, gb.stride, patches, patch_bytes, patch_bytes, n, hipMemcpyHostToDevice, up));
    HIPCHK(hipMemcpyAsync(dargs, reinterpret_cast<uint8_t*>(sl.up.at(R.u_args)), sizeof(SolveArgs) * n, hipMemcpyHostToDevice, up));
    HIPCHK(hipMemcpyAsync(dfargs, reinterpret_cast<uint8_t*>(sl.up.at(R.u_fargs)), sizeof(FinalizeArgs) * n, hipMemcpyHostToDevice, up));
    if (int32_t rc = mode.Upload(R, sl)) return rc;
    HIPCHK(hipEventRecord(sl.uploaded, up));
    HIPCHK(launch_batch_init(bi, n, sl.ks));
    HIPCHK(hipStreamWaitEvent(sl.ks, sl.uploaded, 0));
    HIPCHK(hipEventRecord(sl.t0, sl.ks));
    HIPCHK(launch_solve_batch(sargs[0], dargs, n, dyn, sl.ks));
    if (int32_t rc = mode.Enqueue(R, sl)) return rc;
    HIPCHK(hipEventRecord(sl.t1, sl.ks));
    // downloads on their own stream once the kernels are done (the next launch's kernels need not wait for them)
    HIPCHK(hipStreamWaitEvent(dn, sl.t1, 0));
    if (int32_t rc = mode.Download(R, sl)) return rc;
    HIPCHK(hipEventRecord(sl.done, dn));
    // the previous launch's decisions while this one runs
    if (pending >= 0) {
      if (int32_t rc = decide(slots[pending])) return rc;
    }
    pending = launch_no & 1;
    ++T.n_launches;
  }
  if (pending >= 0) {
    if (int32_t rc = decide(slots[pending])) return rc;
  }
  return KP_OK;
}

// The subsets of a general-path call, checked and split: cands[s] the members of subset s; batched / single the
// subsets the superset Solve takes / those compiled on their own; the budget-blocked ones are in neither (bg->blocked
// counts them). Builds the plan's superset Solve when it has none (again after an offering refresh of its catalogues).
// drift: a superset compile carrying minValues is not batched (Truncate's minValues check needs the options on the host).
static int32_t GeneralPartition(kp_cluster_plan* plan, const uint32_t* offsets, const uint32_t* nodes, uint32_t n_subsets,
                                BudgetGate* bg, bool drift, vector<vector<uint32_t>>& cands_out, vector<int>& batched,
                                vector<int>& single, vector<char>* blocked_out = nullptr) {
  kp_ctx* ctx = plan->ctx;
  const kp_cluster& cl = plan->cluster()->cl;
  const int N = (int)cl.n_nodes;
  if (int32_t rc = CatalogsAlive(plan->cluster()->alive)) return rc;
  if (offsets[0] != 0) return fail(KP_E_INVAL, "offsets[0] != 0");
  if (offsets[n_subsets] && !nodes) return fail(KP_E_INVAL, "null nodes");
  for (uint32_t s = 0; s < n_subsets; s++)
    if (offsets[s + 1] < offsets[s]) return fail(KP_E_INVAL, "offsets not monotone at %u", s);
  // the subsets' candidate lists, checked on up to 16 threads (each with its own membership marks); the error reported
  // is the first subset's, as the serial check would report it
  vector<vector<uint32_t>>& cands = cands_out;
  cands.assign(n_subsets, {});
  std::atomic<int64_t> bad_s{INT64_MAX};
  vector<vector<char>> inS(kMaxHostThreads);
  ParallelFor((int)n_subsets, [&](int s_lo, int s_hi, int t) {
    vector<char>& mark = inS[t];
    mark.assign(N, 0);
    for (int s = s_lo; s < s_hi; s++) {
      cands[s].assign(nodes + offsets[s], nodes + offsets[s + 1]);
      bool ok = true;
      size_t k = 0;
      for (; k < cands[s].size(); k++) {
        const uint32_t c = cands[s][k];
        if (c >= (uint32_t)N || cl.nodes[c].deleting || mark[c]) {
          ok = false;
          break;
        }
        mark[c] = 1;
      }
      for (size_t j = 0; j < k; j++) mark[cands[s][j]] = 0;
      if (!ok) {
        int64_t cur = bad_s.load();
        while (s < cur && !bad_s.compare_exchange_weak(cur, s)) {
        }
        return;
      }
    }
  });
  if (bad_s.load() != INT64_MAX) {  // the serial check's message for the first bad subset
    const uint32_t s = (uint32_t)bad_s.load();
    vector<char> mark(N, 0);
    for (uint32_t k = offsets[s]; k < offsets[s + 1]; k++) {
      const uint32_t c = nodes[k];
      if (c >= (uint32_t)N) return fail(KP_E_INVAL, "subset %u: node %u", s, c);
      if (cl.nodes[c].deleting) return fail(KP_E_INVAL, "subset %u: node %u is being deleted", s, c);
      if (mark[c]) return fail(KP_E_INVAL, "subset %u: node %u twice", s, c);
      mark[c] = 1;
    }
  }
  if (bg)  // disruption budgets: every member must be owned by a NodePool of the cluster
    for (uint32_t s = 0; s < n_subsets; s++)
      for (uint32_t k = offsets[s]; k < offsets[s + 1]; k++)
        if (plan->node_pool[nodes[k]] == 0xFFFF)
          return fail(KP_E_INVAL, "subset %u: node %u has no NodePool of the cluster (karpenter.sh/nodepool)", s, nodes[k]);
  // the batched path: built once per plan (again after an offering refresh of its catalogues)
  if (plan->gb) {
    const SolveBase& B = *plan->gb->C->B;
    if (CatalogsAlive(B.alive) || plan->gb->base_version != B.version || SeqnumsOf(B.catalogs) != B.seqnums) {
      plan->gb.reset();
      plan->gb_tried = false;
    }
  }
  const bool batch_on = ctx->ov.general_batch == 0;
  if (batch_on && !plan->gb_tried) {
    plan->gb_tried = true;
    int32_t rc = GeneralBatchBuild(plan, plan->gb);
    if (rc == KP_E_NOMEM || rc == KP_E_DEVICE) (void)hipGetLastError(), rc = KP_E_UNSUPPORTED;  // (as at prepare)
    if (rc && rc != KP_E_UNSUPPORTED) return rc;
    if (rc) plan->gb.reset();
  }
  vector<char> batchable(n_subsets, 0), blocked(n_subsets, 0);
  ParallelFor((int)n_subsets, [&](int s_lo, int s_hi, int) {
    vector<uint32_t> per_pool(bg ? plan->n_pools : 0);
    for (int s = s_lo; s < s_hi; s++) {
      if (bg) {  // the budget gate's rule (budget_gate_kernel): no NodePool owns more members than it allows
        std::fill(per_pool.begin(), per_pool.end(), 0u);
        for (uint32_t c : cands[s])
          if (++per_pool[plan->node_pool[c]] > bg->allowed[plan->node_pool[c]]) blocked[s] = 1;
        if (blocked[s]) continue;  // neither batched nor compiled: the zero no-op
      }
      bool ok = batch_on && plan->gb && !(drift && plan->gb->min_values);
      if (ok && plan->gb->C->G) {  // an inverse anti-affinity group would vanish: the per-subset compile
        const Compiled& C = *plan->gb->C;
        std::map<int, int> inv;
        for (uint32_t c : cands[s])
          for (int32_t g : C.node_inv[plan->gb->node_input[c]])
            if (++inv[g] == C.tg_inv_total[g]) ok = false;
      }
      batchable[s] = ok ? 1 : 0;
    }
  });
  for (uint32_t s = 0; s < n_subsets; s++) {
    if (blocked[s]) {
      bg->blocked++;
      continue;
    }
    (batchable[s] ? batched : single).push_back((int)s);
  }
  if (blocked_out) blocked_out->swap(blocked);
  return KP_OK;
}

// the nodes' labels as NodeCandidatePrice reads them, built once per plan
static const vector<std::map<string, string>>& PlanLabels(kp_cluster_plan* plan) {
  const kp_cluster& cl = plan->cluster()->cl;
  const int N = (int)cl.n_nodes;
  vector<std::map<string, string>>& labels = plan->general_labels;
  if ((int)labels.size() != N) {
    labels.assign(N, {});
    for (int i = 0; i < N; i++)
      for (uint32_t j = 0; j < cl.nodes[i].node.n_labels; j++) {
        const kp_label& l = cl.nodes[i].node.labels[j];
        labels[i][Normalize(l.key ? l.key : "")] = l.value ? l.value : "";
      }
  }
  return labels;
}
// whys (kp_cluster_simulate_explained, or null): [n_subsets] reason records, the budget-blocked subsets' included
static int32_t GeneralSimLocked(kp_cluster_plan* plan, const uint32_t* offsets, const uint32_t* nodes,
                                uint32_t n_subsets, int32_t multi_node, SimArgs& a, kp_cancel* cancel, BudgetGate* bg,
                                kp_solve_result** commands = nullptr, kp_sim_why* whys = nullptr) {
  kp_ctx* ctx = plan->ctx;
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  const vector<std::map<string, string>>& labels = PlanLabels(plan);
  vector<vector<uint32_t>> cands;
  vector<int> batched, single;
  vector<char> blocked;
  if (int32_t rc = GeneralPartition(plan, offsets, nodes, n_subsets, bg, false, cands, batched, single, &blocked)) return rc;
  for (uint32_t s = 0; whys && s < n_subsets; s++) {
    WhyClear(&whys[s]);
    if (blocked[s]) whys[s].reason = KP_UNCONS_BUDGET;
  }
  const double t_setup = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  vector<SimOut> outs(n_subsets);
  memset(outs.data(), 0, sizeof(SimOut) * outs.size());
  GenTotals T;
  T.batched = batched.size(), T.single = single.size();
  memset(plan->general_phase, 0, sizeof plan->general_phase);
  ConsolidateMode mode(plan, T, cancel, labels, multi_node, outs, commands, whys);
  const auto t1 = clk::now();
  if (!batched.empty())
    if (int32_t rc = GeneralBatchRun(*plan->gb, cands, batched, mode)) return rc;
  const double t_batch = std::chrono::duration<double, std::milli>(clk::now() - t1).count();
  const auto t2 = clk::now();
  for (int s : single)
    if (int32_t rc = mode.SimOne(cands[s], s)) return rc;
  const double t_single = std::chrono::duration<double, std::milli>(clk::now() - t2).count();
  // results and counters in device buffers, as the batched kernel leaves them
  const size_t need = sizeof(SimOut) * std::max<uint32_t>(n_subsets, 1) + 256 + sizeof(uint64_t) * 8;
  if (need > plan->batch_bytes) {
    if (plan->batch.p) HIPCHK(hipFree(plan->batch.p));
    plan->batch.p = nullptr;
    HIPCHK(hipMalloc(&plan->batch.p, need));
    plan->batch_bytes = need;
  }
  a = SimArgs{};
  a.out = (SimOut*)plan->batch.p;
  a.stats = (uint64_t*)((uint8_t*)plan->batch.p + ((sizeof(SimOut) * std::max<uint32_t>(n_subsets, 1) + 255) & ~(size_t)255));
  uint64_t st[8] = {T.counters[0], T.counters[1], T.counters[2], T.batched, T.single, 0, T.n_launches, 0};
  if (n_subsets) HIPCHK(hipMemcpyAsync(a.out, outs.data(), sizeof(SimOut) * n_subsets, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(a.stats, st, sizeof st, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  plan->general_ms = T.dev_ms;
  plan->general_batched = (uint32_t)batched.size();
  if (ctx->ov.host_timing)
    fprintf(stderr, "[kp general] %u sims (%zu batched, %zu single): setup %.2f batch %.2f (overlays %.2f decisions %.2f "
            "device %.2f) single %.2f ms\n", n_subsets, batched.size(), single.size(), t_setup, t_batch, T.host_ms[0],
            T.host_ms[1], T.dev_ms, t_single);
  return KP_OK;
}

// ---- Drift (kp_cluster_drift) ----------------------------------------------------------------------------------
// Each subset is the simulation above run as a whole Solve; what comes back is AllNonPendingPodsScheduled per subset
// and the Solve result of the first feasible one (DriftMode). Batched subsets: solve_kernel (stop_nc 0),
// drift_verdict_kernel, drift_first_kernel and finalize_drift_kernel per launch; the others: their own Solve, the
// verdict taken on the host from the result kp_solve_run has already copied back.
static int32_t DriftLocked(kp_cluster_plan* plan, kp_cancel* cancel, const uint32_t* offsets, const uint32_t* nodes,
                           uint32_t n_subsets, BudgetGate* bg, kp_drift_result* out, int64_t* first,
                           kp_solve_result** replacements, kp_solve_stats* stats) {
  kp_ctx* ctx = plan->ctx;
  if (cancel && __atomic_load_n(cancel->flag, __ATOMIC_SEQ_CST)) return fail(KP_E_CANCELED, "cancelled before the simulations");
  if (!plan->cluster()) return fail(KP_E_INVAL, "the plan holds no cluster");
  if (!plan->general) {  // a plan of the batched simulation kernel: its stale-plan refusal, as kp_cluster_simulate's
    if (int32_t rc = CatalogsAlive(plan->cp->B->alive)) return rc;
    if (SeqnumsOf(plan->cp->B->catalogs) != plan->cp->B->seqnums)
      return fail(KP_E_INVAL, "stale plan: a catalogue's seqnum changed since it was prepared (kp_cluster_refresh)");
  }
  const auto t0 = std::chrono::steady_clock::now();
  vector<vector<uint32_t>> cands;
  vector<int> batched, single;
  vector<char> blocked;
  if (int32_t rc = GeneralPartition(plan, offsets, nodes, n_subsets, bg, true, cands, batched, single, &blocked)) return rc;
  // (the general path's per-call diagnostics: a drift call reports no solve_kernel phase cycles, and leaves none of an
  // earlier simulate call behind)
  memset(plan->general_phase, 0, sizeof plan->general_phase);
  plan->general_ms = 0;
  plan->general_batched = 0;
  GenTotals T;
  T.batched = batched.size(), T.single = single.size();
  DriftMode mode(plan, T, cancel, n_subsets);
  if (!batched.empty()) {
    GeneralBatch& gb = *plan->gb;
    if (int32_t rc = RecordTables(ctx, gb, plan->cluster()->cl)) return rc;
    if (gb.drift_out_n < n_subsets) {
      HIPCHK(gb.drift_out.alloc(sizeof(DriftOut) * n_subsets));
      gb.drift_out_n = n_subsets;
    }
    mode.v.dev = (DriftOut*)gb.drift_out.p;
    if (int32_t rc = GeneralBatchRun(gb, cands, batched, mode)) return rc;
    if (int32_t rc = mode.v.Merge(ctx->stream, batched)) return rc;
  }
  for (int s : single)
    if (int32_t rc = mode.SimOne(cands[s], s)) return rc;
  static_assert(sizeof(DriftOut) == sizeof(kp_drift_result), "DriftOut mirrors kp_drift_result");
  DriftOut stamp{};
  stamp.blocked = 1, stamp.first_unscheduled = -1;
  mode.v.Emit(blocked, stamp, out);
  *first = mode.first;
  if (replacements) *replacements = mode.res.release();
  if (stats) FillStats(stats, plan, T, t0);
  if (ctx->ov.host_timing)
    fprintf(stderr, "[kp drift] %u sims (%zu batched, %zu single, %llu launches): overlays %.2f records %.2f device %.2f ms\n",
            n_subsets, batched.size(), single.size(), (unsigned long long)T.n_launches, T.host_ms[0], T.host_ms[1], T.dev_ms);
  return KP_OK;
}

int32_t kp_cluster_drift(kp_cluster_plan* plan, kp_cancel* cancel, const uint32_t* offsets, const uint32_t* nodes,
                         uint32_t n_subsets, const uint32_t* allowed, uint32_t n_allowed, kp_drift_result* out,
                         int64_t* first, kp_solve_result** replacements, uint64_t* n_blocked, kp_solve_stats* stats) {
  if (n_blocked) *n_blocked = 0;
  if (first) *first = -1;
  if (replacements) *replacements = nullptr;
  if (!plan || !first || (n_subsets && !offsets)) return fail(KP_E_INVAL, "null argument");
  if (cancel && cancel->ctx.p != plan->ctx.p) return fail(KP_E_INVAL, "the cancel token belongs to another context");
  kp_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  if (stats) memset(stats, 0, sizeof *stats);
  BudgetGate bg{allowed, n_allowed};
  if (allowed)
    if (int32_t rc = CheckBudget(plan, &bg)) return rc;
  if (n_subsets == 0) return KP_OK;
  const int32_t rc = DriftLocked(plan, cancel, offsets, nodes, n_subsets, allowed ? &bg : nullptr, out, first, replacements, stats);
  if (!rc && n_blocked) *n_blocked = bg.blocked;
  return rc;
}

// kp_cluster_command on a plan of the batched kernel: where the launch left the subsets' command records
struct CmdEmit {
  const uint8_t* rec = nullptr;  // [n_subsets] records (device), sim_cmd_stride(cap) bytes each
  size_t stride = 0;
  int cap = 0;
  kp_solve_result** commands = nullptr;  // general-path plans: filled from the batched launches' arenas
};
// kp_cluster_validate on a plan of the batched kernel: the checks compiled for the device (ValidateCompile), and where
// the launch leaves the verdict records and, with budgets, the gate's bytes
struct ValCheck {
  vector<uint64_t> want;     // [n_subsets][n_catalogs][TW] type bitmask of the command's options
  vector<uint32_t> unknown;  // [n_subsets][n_catalogs] its names the catalogue does not hold
  vector<uint8_t> replace;   // [n_subsets] 1: the command carries a replacement
  const uint8_t* val = nullptr;   // device: [n_subsets] ValOut
  const uint8_t* gate = nullptr;  // device: [n_subsets] 1 admissible, 0 blocked (budgets only)
};
// kp_cluster_simulate_explained on a plan of the batched kernel: where the launch leaves the reason records and their
// histogram (why_count_kernel, which also writes the budget-blocked subsets' records)
struct WhyEmit {
  const uint8_t* rec = nullptr;     // device: [n_subsets] WhyOut
  const uint64_t* counts = nullptr; // device: [KP_UNCONS_COUNT]
  kp_sim_why* host = nullptr;       // general-path plans: the caller's records, filled by the decision code
};
static_assert(sizeof(WhyOut) == sizeof(kp_sim_why) && WHY_REASONS == KP_UNCONS_COUNT, "WhyOut mirrors kp_sim_why");
static int32_t SimLaunchLocked(kp_cluster_plan* plan, const uint32_t* offsets, const uint32_t* nodes, uint32_t n_subsets,
                               int32_t multi_node, SimArgs& a_out, kp_cancel* cancel, BudgetGate* bg = nullptr,
                               CmdEmit* em = nullptr, ValCheck* vc = nullptr, WhyEmit* wy = nullptr) {
  kp_ctx* ctx = plan->ctx;
  if (cancel && __atomic_load_n(cancel->flag, __ATOMIC_SEQ_CST))
    return fail(KP_E_CANCELED, "cancelled before the simulations");
  if (bg) {
    if (int32_t rc = CheckBudget(plan, bg)) return rc;
    bg->blocked = 0;
  }
  if (plan->general)
    return GeneralSimLocked(plan, offsets, nodes, n_subsets, multi_node, a_out, cancel, bg, em ? em->commands : nullptr,
                            wy ? wy->host : nullptr);
  if (int32_t rc = CatalogsAlive(plan->cp->B->alive)) return rc;
  if (SeqnumsOf(plan->cp->B->catalogs) != plan->cp->B->seqnums)
    return fail(KP_E_INVAL, "stale plan: a catalogue's seqnum changed since it was prepared (kp_cluster_refresh)");
  if (offsets[0] != 0) return fail(KP_E_INVAL, "offsets[0] != 0");
  const uint32_t n_flat = offsets[n_subsets];
  if (n_flat && !nodes) return fail(KP_E_INVAL, "null nodes");
  int cap = 1;
  const bool any_deleting = plan->n_base > 0;
  for (uint32_t s = 0; s < n_subsets; s++) {
    if (offsets[s + 1] < offsets[s]) return fail(KP_E_INVAL, "offsets not monotone at %u", s);
    uint64_t np = (uint64_t)plan->n_base;  // every simulation also schedules the pending and deleting-node pods
    for (uint32_t j = offsets[s]; j < offsets[s + 1]; j++) {
      if (nodes[j] >= (uint32_t)plan->N) return fail(KP_E_INVAL, "subset %u: node %u", s, nodes[j]);
      if (any_deleting && plan->deleting[nodes[j]]) return fail(KP_E_INVAL, "subset %u: node %u is being deleted", s, nodes[j]);
      if (bg && plan->node_pool[nodes[j]] == 0xFFFF)
        return fail(KP_E_INVAL, "subset %u: node %u has no NodePool of the cluster (karpenter.sh/nodepool)", s, nodes[j]);
      np += plan->node_npods[nodes[j]];
    }
    if (np > 65535) return fail(KP_E_UNSUPPORTED, "subset %u reschedules %llu pods (max 65535)", s, (unsigned long long)np);
    cap = std::max(cap, (int)np);
  }
  SimArgs& a = a_out;
  a = plan->a;
  int cap2 = 1;
  while (cap2 < std::max(cap, 2 * plan->T2)) cap2 <<= 1;
  a.cap = cap;
  a.cap2 = cap2;
  a.wave_lds = (int)(((size_t)16 * a.EW + (size_t)6 * cap2 + 15) & ~(size_t)15);
  a.multi_node = multi_node ? 1 : 0;
  a.cancel = nullptr;
  if (cancel) {
    void* dp = nullptr;
    HIPCHK(hipHostGetDevicePointer(&dp, cancel->flag, 0));
    a.cancel = (const int32_t*)dp;
  }
  hipFuncAttributes fa;
  HIPCHK(hipFuncGetAttributes(&fa, wy   ? sim_why_kernel_ptr()
                                   : vc ? sim_check_kernel_ptr()
                                   : em ? sim_emit_kernel_ptr()
                                        : sim_kernel_ptr(bg != nullptr)));
  const size_t lds_wg = fa.sharedSizeBytes + (size_t)SIM_WAVES * a.wave_lds;
  if (lds_wg > 160 * 1024) return fail(KP_E_UNSUPPORTED, "simulation LDS %zu B per workgroup (cluster or subsets too large)", lds_wg);
  const int wg_per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / lds_wg));
  int blocks = std::min<int>((int)((n_subsets + SIM_WAVES - 1) / SIM_WAVES), plan->n_cu * wg_per_cu);
  // kp_overrides.sim_slots (read now, not when the plan was prepared): fewer waves, so each runs many subsets
  if (ctx->ov.sim_slots > 0) blocks = std::min(blocks, (ctx->ov.sim_slots + SIM_WAVES - 1) / SIM_WAVES);
  blocks = std::max(blocks, 1);
  const int slots = blocks * SIM_WAVES;
  plan->sim_waves[0] = (uint64_t)slots;
  plan->sim_waves[1] = (n_subsets + (uint32_t)slots - 1) / (uint32_t)slots;
  a.n_slots = slots;
  a.n_subsets = (int32_t)n_subsets;
  // per-wave scratch
  const size_t sz_pod = sizeof(uint64_t) * (size_t)slots * cap;
  const size_t sz_start = sizeof(int32_t) * (size_t)slots * std::max(a.SL, 1);
  const size_t sz_ovl = sizeof(int64_t) * (size_t)slots * std::max(a.E, 1) * std::max(a.RU, 1);
  const size_t sz_nc = sizeof(SimNC) * (size_t)slots;
  const size_t sz_fail = sizeof(int32_t) * (size_t)slots * std::max(a.SL, 1);
  const size_t sz_ovlhp = a.hp_any ? sizeof(uint64_t) * (size_t)slots * std::max(a.E, 1) : 8;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t need = al(sz_pod) + al(sz_start) + al(sz_ovl) + al(sz_nc) + al(sz_fail) + al(sz_ovlhp) + al(sizeof(uint64_t) * 8);
  if (need > plan->scratch_bytes) {
    if (plan->scratch.p) HIPCHK(hipFree(plan->scratch.p));
    plan->scratch.p = nullptr;
    HIPCHK(hipMalloc(&plan->scratch.p, need));
    plan->scratch_bytes = need;
  }
  uint8_t* sb = (uint8_t*)plan->scratch.p;
  size_t o = 0;
  a.s_pod = (uint64_t*)(sb + o);
  o += al(sz_pod);
  a.s_start = (int32_t*)(sb + o);
  o += al(sz_start);
  a.s_ovl = (int64_t*)(sb + o);
  o += al(sz_ovl);
  a.s_nc = (SimNC*)(sb + o);
  o += al(sz_nc);
  a.s_ncfail = (int32_t*)(sb + o);
  o += al(sz_fail);
  a.s_ovlhp = (uint64_t*)(sb + o);
  o += al(sz_ovlhp);
  a.stats = (uint64_t*)(sb + o);
  // batch: subsets + results
  const size_t b_off = al(sizeof(uint32_t) * (n_subsets + 1)), b_nodes = al(sizeof(uint32_t) * std::max<uint32_t>(n_flat, 1));
  const size_t b_out = al(sizeof(SimOut) * n_subsets);
  // the budget gate's regions: gate bytes, live list, block counts and offsets, allowed[], the live count
  const uint32_t n_gblk = (n_subsets + GATE_BLOCK - 1) / GATE_BLOCK;
  const size_t g_gate = bg ? al(n_subsets) : 0, g_live = bg || em || vc || wy ? al(sizeof(uint32_t) * n_subsets) : 0;
  const size_t g_blk = bg ? al(sizeof(uint32_t) * n_gblk) : 0, g_allowed = bg ? al(sizeof(uint32_t) * (plan->n_pools + 1)) : 0;
  // the command records (kp_cluster_command), sized from the batch: behind everything else
  const size_t o_rec = b_off + b_nodes + b_out + g_gate + g_live + 2 * g_blk + g_allowed + (bg ? 256 : 0);
  const size_t rec_stride = em ? sim_cmd_stride(cap) : 0;
  // (the call is meant for the few subsets a pass ends on; a batch whose records would not fit a 32-bit byte count is
  // handed back rather than run in parts)
  if (em && rec_stride * (size_t)n_subsets > ((size_t)4 << 30))
    return fail(KP_E_UNSUPPORTED, "%u subsets of up to %d pods: %zu B of command records (max 4 GiB per call)", n_subsets, cap,
                rec_stride * (size_t)n_subsets);
  // the checks and the verdict records (kp_cluster_validate): behind those
  const size_t o_chk = o_rec + al(rec_stride * n_subsets);
  const size_t v_want = vc ? al(sizeof(uint64_t) * vc->want.size()) : 0, v_unk = vc ? al(sizeof(uint32_t) * vc->unknown.size()) : 0;
  const size_t v_rep = vc ? al(n_subsets) : 0, v_val = vc ? al(sizeof(ValOut) * n_subsets) : 0;
  // the reason records, the histogram's partials and the histogram (kp_cluster_simulate_explained): behind those
  const size_t o_why = o_chk + v_want + v_unk + v_rep + v_val;
  const size_t y_rec = wy ? al(sizeof(WhyOut) * n_subsets) : 0;
  const size_t y_part = wy ? al(sizeof(uint64_t) * WHY_REASONS * WHY_COUNT_MAX_BLOCKS) : 0;
  const size_t b_total = o_why + y_rec + y_part + (wy ? al(sizeof(uint64_t) * WHY_REASONS) : 0);
  if (b_total > plan->batch_bytes) {
    if (plan->batch.p) HIPCHK(hipFree(plan->batch.p));
    plan->batch.p = nullptr;
    plan->batch_bytes = 0;
    HIPCHK(hipMalloc(&plan->batch.p, b_total));
    plan->batch_bytes = b_total;
  }
  uint8_t* bb = (uint8_t*)plan->batch.p;
  a.sub_off = (const uint32_t*)bb;
  a.sub_nodes = (const uint32_t*)(bb + b_off);
  a.out = (SimOut*)(bb + b_off + b_nodes);
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(bb, offsets, sizeof(uint32_t) * (n_subsets + 1), hipMemcpyHostToDevice, st));
  if (n_flat) HIPCHK(hipMemcpyAsync(bb + b_off, nodes, sizeof(uint32_t) * n_flat, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(a.s_ncfail, 0xFF, sz_fail, st));
  HIPCHK(hipMemsetAsync(a.stats, 0, sizeof(uint64_t) * 8, st));
  SimEmit se{nullptr, bb + o_rec, rec_stride};
  SimCheck sc{nullptr, (const uint64_t*)(bb + o_chk), (const uint32_t*)(bb + o_chk + v_want), bb + o_chk + v_want + v_unk,
              (uint32_t*)(bb + o_chk + v_want + v_unk + v_rep)};
  if (vc) {
    HIPCHK(hipMemcpyAsync((void*)sc.want, vc->want.data(), sizeof(uint64_t) * vc->want.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync((void*)sc.unknown, vc->unknown.data(), sizeof(uint32_t) * vc->unknown.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync((void*)sc.replace, vc->replace.data(), n_subsets, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(sc.val, 0, sizeof(ValOut) * n_subsets, st));
    vc->val = (const uint8_t*)sc.val;
  }
  if (em) {
    em->rec = bb + o_rec;
    em->stride = rec_stride;
    em->cap = cap;
  }
  SimWhy sw{nullptr, (uint32_t*)(bb + o_why)};
  uint64_t* why_part = (uint64_t*)(bb + o_why + y_rec);
  uint64_t* why_counts = (uint64_t*)(bb + o_why + y_rec + y_part);
  if (wy) {
    wy->rec = bb + o_why;
    wy->counts = why_counts;
  }
  if (bg) {
    // the gate on the resident batch, then the live count (4 bytes) sizes the simulation grid
    uint8_t* gp = bb + b_off + b_nodes + b_out;
    GateArgs g;
    memset(&g, 0, sizeof g);
    g.n_subsets = (int32_t)n_subsets;
    g.n_pools = (int32_t)plan->n_pools;
    g.n_nodes = plan->N;
    g.sub_off = a.sub_off;
    g.sub_nodes = a.sub_nodes;
    g.node_pool = plan->d_node_pool;
    g.out = a.out;
    g.gate = gp;
    g.live = (uint32_t*)(gp + g_gate);
    g.blk_cnt = (uint32_t*)(gp + g_gate + g_live);
    g.blk_off = (uint32_t*)(gp + g_gate + g_live + g_blk);
    g.allowed = (const uint32_t*)(gp + g_gate + g_live + 2 * g_blk);
    g.n_live = (uint32_t*)(gp + g_gate + g_live + 2 * g_blk + g_allowed);
    if (plan->n_pools)
      HIPCHK(hipMemcpyAsync((void*)g.allowed, bg->allowed, sizeof(uint32_t) * plan->n_pools, hipMemcpyHostToDevice, st));
    HIPCHK(launch_budget_gate(g, st));
    uint32_t n_live = 0;
    HIPCHK(hipMemcpyAsync(&n_live, g.n_live, sizeof n_live, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_live > n_subsets) return fail(KP_E_DEVICE, "budget gate: %u live of %u subsets", n_live, n_subsets);
    bg->blocked = n_subsets - n_live;
    blocks = std::max(1, std::min<int>((int)((n_live + SIM_WAVES - 1) / SIM_WAVES), blocks));
    a.n_slots = blocks * SIM_WAVES;  // (the scratch above holds the ungated grid's slots: at least as many)
    plan->sim_waves[0] = n_live ? (uint64_t)a.n_slots : 0;  // (no live subset: nothing is launched)
    plan->sim_waves[1] = (n_live + (uint32_t)a.n_slots - 1) / (uint32_t)a.n_slots;
    HIPCHK(hipEventRecord(ctx->ev0, st));
    se.live = sc.live = sw.live = g.live;
    if (vc) vc->gate = g.gate;
    if (wy) {
      if (n_live) HIPCHK(launch_sim_why(a, sw, (int)n_live, blocks, (size_t)SIM_WAVES * a.wave_lds, st));
      HIPCHK(launch_why_count(sw.rec, g.gate, (int)n_subsets, why_part, why_counts, st));
    } else if (n_live && vc) HIPCHK(launch_sim_check(a, sc, (int)n_live, blocks, (size_t)SIM_WAVES * a.wave_lds, st));
    else if (n_live && em) HIPCHK(launch_sim_emit(a, se, (int)n_live, blocks, (size_t)SIM_WAVES * a.wave_lds, st));
    else if (n_live) HIPCHK(launch_sim_gated(a, g.live, (int)n_live, blocks, (size_t)SIM_WAVES * a.wave_lds, st));
    HIPCHK(hipEventRecord(ctx->ev1, st));
    return KP_OK;
  }
  if (em || vc || wy) {
    // No budgets: the emitting (and the checking) instantiation walks every subset, in order, through an identity list. An ungated
    // emitting policy would be a fourth sim_kernel instantiation (its own code object and resource figures to hold)
    // to save one 4 * n_subsets byte upload on a call made for a few subsets.
    uint32_t* live = (uint32_t*)(bb + b_off + b_nodes + b_out);
    plan->cmd_live.resize(n_subsets);
    for (uint32_t s = 0; s < n_subsets; s++) plan->cmd_live[s] = s;
    HIPCHK(hipMemcpyAsync(live, plan->cmd_live.data(), sizeof(uint32_t) * n_subsets, hipMemcpyHostToDevice, st));
    se.live = sc.live = sw.live = live;
    HIPCHK(hipEventRecord(ctx->ev0, st));
    if (wy) {
      HIPCHK(launch_sim_why(a, sw, (int)n_subsets, blocks, (size_t)SIM_WAVES * a.wave_lds, st));
      HIPCHK(launch_why_count(sw.rec, nullptr, (int)n_subsets, why_part, why_counts, st));
    } else if (vc) HIPCHK(launch_sim_check(a, sc, (int)n_subsets, blocks, (size_t)SIM_WAVES * a.wave_lds, st));
    else HIPCHK(launch_sim_emit(a, se, (int)n_subsets, blocks, (size_t)SIM_WAVES * a.wave_lds, st));
    HIPCHK(hipEventRecord(ctx->ev1, st));
    return KP_OK;
  }
  HIPCHK(hipEventRecord(ctx->ev0, st));
  HIPCHK(launch_sim(a, blocks, (size_t)SIM_WAVES * a.wave_lds, st));
  HIPCHK(hipEventRecord(ctx->ev1, st));
  return KP_OK;
}

// kp_cluster_command on a plan of the batched kernel: the commands of the subsets that decided DELETE or REPLACE, from
// the records the emitting sim_kernel left (recs: their host copy). Existing positions become the ABI's existing
// index, queue positions the simulation's input order, the spot-to-spot narrowing is applied and the requirements
// are rendered as AssembleResult renders a Solve's.
static int32_t BuildSimCommands(kp_cluster_plan* plan, const uint32_t* offsets, const uint32_t* nodes, uint32_t n_subsets,
                                const kp_sim_result* out, const uint8_t* recs, const CmdEmit& em, kp_solve_result** commands) {
  const Compiled& C = *plan->cp;
  const SolveBase& B = *C.B;
  const Dict& d = B.d;
  if (!plan->owned) return fail(KP_E_INVAL, "the plan keeps no cluster");
  CommandIndex ix(plan->owned->cl);
  const uint32_t P = plan->owned->cl.n_pods;
  for (uint32_t s = 0; s < n_subsets; s++) {
    if (out[s].decision == KP_DECISION_NOOP) continue;
    const SimCmdHdr* h = reinterpret_cast<const SimCmdHdr*>(recs + em.stride * s);
    const uint32_t* rq = reinterpret_cast<const uint32_t*>(h + 1);
    const int32_t* rp = reinterpret_cast<const int32_t*>(rq + em.cap);
    const uint32_t* ro = reinterpret_cast<const uint32_t*>(rp + em.cap);
    const bool replace = out[s].decision == KP_DECISION_REPLACE;
    const int nq = ix.Enter(nodes + offsets[s], offsets[s + 1] - offsets[s]);
    struct Exit {
      CommandIndex& ix;
      ~Exit() { ix.Leave(); }
    } exit_{ix};
    if ((int)h->n_queue != nq || nq > em.cap || (int)h->n_added > nq)
      return fail(KP_E_DEVICE, "command record of subset %u: %u pods queued (%d expected), %u added", s, h->n_queue, nq, h->n_added);
    auto res = std::make_unique<kp_solve_result>();
    memset(&res->stats, 0, sizeof res->stats);
    res->placement.assign(nq, -1);
    vector<int32_t> at(nq, -1);  // queue position -> input index
    for (int i = 0; i < nq; i++) {
      const int32_t idx = rq[i] < P ? ix.pod_idx[C.queue[rq[i]]] : -1;
      if (idx < 0 || idx >= nq) return fail(KP_E_DEVICE, "command record of subset %u: queue position %d names rank %u", s, i, rq[i]);
      at[i] = idx;
      const int32_t pl = rp[i];
      if (pl == 0 && replace) {
        res->placement[idx] = 0;
      } else if (pl <= -2) {
        const int pos = -2 - pl;
        const int e = pos < (int)C.ex_input.size() ? ix.Existing((uint32_t)C.ex_input[pos]) : -1;
        if (e < 0) return fail(KP_E_DEVICE, "command record of subset %u: a pod on existing position %d", s, pos);
        res->placement[idx] = -2 - e;
      } else if (pl != -1) {
        return fail(KP_E_DEVICE, "command record of subset %u: placement %d", s, pl);
      }
    }
    if (replace) {
      if (h->tmpl < 0 || h->tmpl >= (int)B.tmpl_catalog.size() || h->n_kept > SIM_CMD_OPTS || h->n_kept != out[s].n_options)
        return fail(KP_E_DEVICE, "command record of subset %u: template %d, %u options (%u decided)", s, h->tmpl, h->n_kept,
                    out[s].n_options);
      res->ncs.resize(1);
      auto& nc = res->ncs[0];
      nc.nodepool = (uint32_t)B.tmpl_nodepool[h->tmpl];
      nc.n_remaining = h->n_remaining;
      nc.options.assign(h->options, h->options + h->n_kept);
      memset(&nc.requests, 0, sizeof nc.requests);
      for (int r = 0; r < KP_NRES; r++) {
        nc.requests.milli[r] = h->requests[r];
        if (nc.requests.milli[r]) nc.requests.present |= 1u << r;
      }
      for (uint32_t j = 0; j < h->n_added; j++) {
        if (ro[j] >= (uint32_t)nq) return fail(KP_E_DEVICE, "command record of subset %u: add %u names position %u", s, j, ro[j]);
        nc.pods.push_back((uint32_t)at[ro[j]]);
      }
      KReqs fin = h->reqs;
      if (h->s2s) NarrowToSpot(d, fin);
      nc.reqs = DecodeReqs(d, fin);
      res->fin.push_back(fin);
      res->nc_cat.push_back(B.tmpl_catalog[h->tmpl]);
    }
    commands[s] = res.release();
  }
  return KP_OK;
}

static int32_t SimulateImpl(kp_cluster_plan* plan, kp_cancel* cancel, const uint32_t* offsets, const uint32_t* nodes,
                            uint32_t n_subsets, int32_t multi_node, kp_sim_result* out, kp_solve_stats* stats,
                            BudgetGate* bg, kp_solve_result** commands = nullptr) {
  auto t0 = std::chrono::steady_clock::now();
  if (!plan || (n_subsets && (!offsets || !out))) return fail(KP_E_INVAL, "null argument");
  if (cancel && cancel->ctx.p != plan->ctx.p) return fail(KP_E_INVAL, "the cancel token belongs to another context");
  kp_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  if (stats) memset(stats, 0, sizeof *stats);
  if (bg)
    if (int32_t rc = CheckBudget(plan, bg)) return rc;
  if (n_subsets == 0) return KP_OK;
  SimArgs a;
  CmdEmit em;
  em.commands = commands;
  int32_t rc = SimLaunchLocked(plan, offsets, nodes, n_subsets, multi_node, a, cancel, bg, commands ? &em : nullptr);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  uint64_t kst[8];
  vector<uint8_t> recs;  // the command records of a batched-kernel plan
  if (em.rec) {
    recs.resize(em.stride * n_subsets);
    HIPCHK(hipMemcpyAsync(recs.data(), em.rec, recs.size(), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipMemcpyAsync(out, a.out, sizeof(SimOut) * n_subsets, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(kst, a.stats, sizeof kst, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (!plan->general && kst[5]) return fail(KP_E_CANCELED, "consolidation simulations cancelled (kp_cancel_set)");
  float ms = (float)plan->general_ms;
  if (!plan->general) HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  for (uint32_t s = 0; s < n_subsets; s++)
    if (out[s].n_pods == 0xFFFFFFFFu) return fail(KP_E_DEVICE, "subset %u overflowed the pod queue", s);
  if (em.rec)
    if (int32_t rc2 = BuildSimCommands(plan, offsets, nodes, n_subsets, out, recs.data(), em, commands)) return rc2;
  if (stats) {
    FillStats(stats, plan, TotalsOf(kst, ms), t0);
    if (plan->general) {
      for (int k = 0; k < 8; k++) stats->attempt_cycles[k] = plan->general_phase[k];  // (timing diagnostics)
    } else {  // batched sweep: wave slots launched, most subsets any wave ran
      stats->phase_cycles[1] = plan->sim_waves[0];
      stats->phase_cycles[2] = plan->sim_waves[1];
    }
  }
  return KP_OK;
}

int32_t kp_cluster_simulate_cancellable(kp_cluster_plan* plan, kp_cancel* cancel, const uint32_t* offsets,
                                        const uint32_t* nodes, uint32_t n_subsets, int32_t multi_node, kp_sim_result* out,
                                        kp_solve_stats* stats) {
  return SimulateImpl(plan, cancel, offsets, nodes, n_subsets, multi_node, out, stats, nullptr);
}

int32_t kp_cluster_simulate(kp_cluster_plan* plan, const uint32_t* offsets, const uint32_t* nodes, uint32_t n_subsets,
                            int32_t multi_node, kp_sim_result* out, kp_solve_stats* stats) {
  return kp_cluster_simulate_cancellable(plan, nullptr, offsets, nodes, n_subsets, multi_node, out, stats);
}

int32_t kp_cluster_simulate_budgeted(kp_cluster_plan* plan, kp_cancel* cancel, const uint32_t* offsets,
                                     const uint32_t* nodes, uint32_t n_subsets, int32_t multi_node,
                                     const uint32_t* allowed, uint32_t n_allowed, kp_sim_result* out, uint64_t* n_blocked,
                                     kp_solve_stats* stats) {
  if (n_blocked) *n_blocked = 0;
  if (!allowed) return SimulateImpl(plan, cancel, offsets, nodes, n_subsets, multi_node, out, stats, nullptr);
  BudgetGate bg{allowed, n_allowed};
  const int32_t rc = SimulateImpl(plan, cancel, offsets, nodes, n_subsets, multi_node, out, stats, &bg);
  if (!rc && n_blocked) *n_blocked = bg.blocked;
  return rc;
}

int32_t kp_cluster_command(kp_cluster_plan* plan, kp_cancel* cancel, const uint32_t* offsets, const uint32_t* nodes,
                           uint32_t n_subsets, int32_t multi_node, const uint32_t* allowed, uint32_t n_allowed,
                           kp_sim_result* out, kp_solve_result** commands, uint64_t* n_blocked, kp_solve_stats* stats) {
  if (n_blocked) *n_blocked = 0;
  if (n_subsets && !commands) return fail(KP_E_INVAL, "null argument");
  for (uint32_t s = 0; s < n_subsets; s++) commands[s] = nullptr;
  BudgetGate bg{allowed, n_allowed};
  const int32_t rc = SimulateImpl(plan, cancel, offsets, nodes, n_subsets, multi_node, out, stats, allowed ? &bg : nullptr,
                                  n_subsets ? commands : nullptr);
  if (rc) {  // no command outlives a failed call
    for (uint32_t s = 0; s < n_subsets; s++) {
      kp_result_destroy(commands[s]);
      commands[s] = nullptr;
    }
    return rc;
  }
  if (n_blocked && allowed) *n_blocked = bg.blocked;
  return KP_OK;
}

// ---- Why a subset cannot be consolidated (kp_cluster_simulate_explained) ------------------------------------------
int32_t kp_cluster_simulate_explained(kp_cluster_plan* plan, kp_cancel* cancel, const uint32_t* offsets,
                                      const uint32_t* nodes, uint32_t n_subsets, int32_t multi_node,
                                      const uint32_t* allowed, uint32_t n_allowed, kp_sim_result* out, kp_sim_why* why,
                                      uint64_t* counts, uint64_t* n_blocked, kp_solve_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  if (n_blocked) *n_blocked = 0;
  if (counts) memset(counts, 0, sizeof(uint64_t) * KP_UNCONS_COUNT);
  if (!plan || (n_subsets && (!offsets || !out || (!why && !counts)))) return fail(KP_E_INVAL, "null argument");
  if (cancel && cancel->ctx.p != plan->ctx.p) return fail(KP_E_INVAL, "the cancel token belongs to another context");
  kp_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  if (stats) memset(stats, 0, sizeof *stats);
  BudgetGate gate{allowed, n_allowed};
  BudgetGate* bg = allowed ? &gate : nullptr;
  if (bg)
    if (int32_t rc = CheckBudget(plan, bg)) return rc;
  if (n_subsets == 0) return KP_OK;
  // why == NULL: the histogram alone. The records then stay on the device, unless the host needs them: a general-path
  // plan fills them on the host, and with NodePool limits the MULTIPLE_NODECLAIMS ones are settled below.
  bool limited = false;
  if (!plan->general)
    for (uint32_t lp : plan->cp->tmpl_limit_present) limited = limited || lp != 0;
  vector<kp_sim_why> own;
  if (!why && (plan->general || limited)) {
    own.resize(n_subsets);
    why = own.data();
  }
  SimArgs a;
  WhyEmit wy;
  wy.host = why;
  if (int32_t rc = SimLaunchLocked(plan, offsets, nodes, n_subsets, multi_node, a, cancel, bg, nullptr, nullptr, &wy)) return rc;
  hipStream_t st = ctx->stream;
  uint64_t kst[8];
  uint64_t hist[KP_UNCONS_COUNT] = {};
  HIPCHK(hipMemcpyAsync(out, a.out, sizeof(SimOut) * n_subsets, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(kst, a.stats, sizeof kst, hipMemcpyDeviceToHost, st));
  if (!plan->general) {
    if (why) HIPCHK(hipMemcpyAsync(why, wy.rec, sizeof(WhyOut) * n_subsets, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hist, wy.counts, sizeof hist, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  if (!plan->general && kst[5]) return fail(KP_E_CANCELED, "consolidation simulations cancelled (kp_cancel_set)");
  float ms = (float)plan->general_ms;
  if (!plan->general) HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  for (uint32_t s = 0; s < n_subsets; s++)
    if (out[s].n_pods == 0xFFFFFFFFu) return fail(KP_E_DEVICE, "subset %u overflowed the pod queue", s);
  GenTotals T = TotalsOf(kst, ms);
  uint64_t reruns = 0;
  if (plan->general) {
    for (uint32_t s = 0; s < n_subsets; s++)
      if ((uint32_t)why[s].reason < KP_UNCONS_COUNT) hist[why[s].reason]++;
  } else {
    // NodePool limits: sim_kernel stops where a pod would open a second NodeClaim, judged by the limits the pass began
    // with, while the first NodeClaim has taken its largest option out of its pool's remaining limits (subtractMax): that
    // second NodeClaim may not exist and the pod fail instead. MULTIPLE_NODECLAIMS against UNSCHEDULABLE is this call's
    // answer, so every such record is settled by the subset's own whole Solve and the decision code's reasons (as
    // kp_cluster_validate settles its rule 3). out[s] stays the kernel's: a Solve that would change it (a pending pod
    // was the one without a second NodeClaim) leaves the kernel's record too.
    if (limited) {
      if (!plan->cluster()) return fail(KP_E_INVAL, "the plan keeps no cluster");
      const vector<std::map<string, string>>& labels = PlanLabels(plan);
      for (uint32_t s = 0; s < n_subsets; s++) {
        if (why[s].reason != KP_UNCONS_MULTIPLE_NODECLAIMS) continue;
        const vector<uint32_t> cand(nodes + offsets[s], nodes + offsets[s + 1]);
        SimOut r;
        memset(&r, 0, sizeof r);
        kp_sim_why w;
        if (int32_t rc = GeneralSimOne(plan, cand, labels, multi_node, r, T, cancel, nullptr, &w)) return rc;
        reruns++;
        if (r.decision != out[s].decision || (uint32_t)w.reason >= KP_UNCONS_COUNT) continue;
        hist[KP_UNCONS_MULTIPLE_NODECLAIMS]--;
        hist[w.reason]++;
        why[s] = w;
      }
    }
  }
  if (counts) memcpy(counts, hist, sizeof hist);
  if (n_blocked && bg) *n_blocked = gate.blocked;
  if (stats) {
    FillStats(stats, plan, T, t0);
    if (plan->general) {
      for (int k = 0; k < 8; k++) stats->attempt_cycles[k] = plan->general_phase[k];  // (timing diagnostics)
    } else {  // batched sweep: wave slots launched, most subsets any wave ran, subsets settled by their own Solve
      stats->phase_cycles[1] = plan->sim_waves[0];
      stats->phase_cycles[2] = plan->sim_waves[1];
      stats->phase_cycles[3] = reruns;
    }
  }
  return KP_OK;
}

// ---- Command validation (kp_cluster_validate) --------------------------------------------------------------------
static_assert(sizeof(ValOut) == sizeof(kp_validation), "ValOut mirrors kp_validation");

// A check's names as a set, in first-mention order; KP_E_INVAL as kp_abi.h lists it.
static int32_t CheckNames(const kp_command_check& c, uint32_t s, vector<string>& names) {
  names.clear();
  if (c.decision != KP_DECISION_DELETE && c.decision != KP_DECISION_REPLACE)
    return fail(KP_E_INVAL, "check %u: decision %d (KP_DECISION_DELETE or KP_DECISION_REPLACE)", s, c.decision);
  if (c.decision == KP_DECISION_DELETE) return KP_OK;
  if (!c.n_options || !c.options) return fail(KP_E_INVAL, "check %u: a replacement without options", s);
  std::set<string> seen;
  for (uint32_t j = 0; j < c.n_options; j++) {
    if (!c.options[j]) return fail(KP_E_INVAL, "check %u: option %u is a null name", s, j);
    if (seen.insert(c.options[j]).second) names.push_back(c.options[j]);
  }
  return KP_OK;
}

// The checks for the device: per (subset, catalogue) the options' type bitmask, names resolved through that
// catalogue's name table, and the count of names it does not hold.
static int32_t ValidateCompile(const vector<const kp_catalog*>& cats, int TW, const kp_command_check* checks,
                               uint32_t n_subsets, ValCheck& vc) {
  const size_t NC = cats.size();
  vector<std::unordered_map<string, int>> table(NC);
  vc.want.assign((size_t)n_subsets * NC * TW, 0);
  vc.unknown.assign((size_t)n_subsets * NC, 0);
  vc.replace.assign(n_subsets, 0);
  vector<string> names;
  for (uint32_t s = 0; s < n_subsets; s++) {
    if (int32_t rc = CheckNames(checks[s], s, names)) return rc;
    if (checks[s].decision != KP_DECISION_REPLACE) continue;
    vc.replace[s] = 1;
    for (size_t c = 0; c < NC; c++) {
      if (table[c].empty())
        for (size_t t = 0; t < cats[c]->types.size(); t++) table[c].emplace(cats[c]->types[t].name, (int)t);
      uint64_t* row = &vc.want[((size_t)s * NC + c) * TW];
      for (const string& nm : names) {
        auto it = table[c].find(nm);
        if (it == table[c].end() || it->second >= TW * 64) vc.unknown[(size_t)s * NC + c]++;
        else row[it->second >> 6] |= 1ull << (it->second & 63);
      }
    }
  }
  return KP_OK;
}

// General-path plans (ValidateMode). Batched subsets: solve_kernel (stop at the second NodeClaim), finalize_kernel,
// validate_verdict_kernel and validate_sum_kernel per launch; a launch downloads its record, the verdicts come back in
// one copy at the end. Subsets compiled on their own: the mode's SimOne.
static int32_t ValidateGeneralLocked(kp_cluster_plan* plan, kp_cancel* cancel, const uint32_t* offsets, const uint32_t* nodes,
                                     uint32_t n_subsets, const kp_command_check* checks, BudgetGate* bg, kp_validation* out,
                                     GenTotals& T) {
  kp_ctx* ctx = plan->ctx;
  if (cancel && __atomic_load_n(cancel->flag, __ATOMIC_SEQ_CST))
    return fail(KP_E_CANCELED, "cancelled before the simulations");
  ValidateMode mode(plan, T, cancel, checks, n_subsets);
  for (uint32_t s = 0; s < n_subsets; s++)
    if (int32_t rc = CheckNames(checks[s], s, mode.names[s])) return rc;
  vector<vector<uint32_t>> cands;
  vector<int> batched, single;
  vector<char> blocked;
  if (int32_t rc = GeneralPartition(plan, offsets, nodes, n_subsets, bg, false, cands, batched, single, &blocked)) return rc;
  // held reservation ids are merged into a NodeClaim's requirements before Truncate's minValues check (ApplyHeld);
  // validate_verdict_kernel checks the finalized requirements as they are, so a superset compile with both
  // reservations and minValues takes the host's verdict for every subset
  if (plan->gb && plan->gb->res_mode && plan->gb->min_values) {
    single.insert(single.end(), batched.begin(), batched.end());
    std::sort(single.begin(), single.end());
    batched.clear();
  }
  T.batched = batched.size(), T.single = single.size();
  DevBuf dev;  // the compiled checks and the verdict records of this call
  if (!batched.empty()) {
    GeneralBatch& gb = *plan->gb;
    if (int32_t rc = RecordTables(ctx, gb, plan->cluster()->cl)) return rc;
    ValCheck vc;
    if (int32_t rc = ValidateCompile(gb.C->B->catalogs, gb.C->B->TW, checks, n_subsets, vc)) return rc;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_unk = al(sizeof(uint64_t) * vc.want.size()), o_rep = o_unk + al(sizeof(uint32_t) * vc.unknown.size());
    const size_t o_out = o_rep + al(n_subsets);
    HIPCHK(dev.alloc(o_out + sizeof(ValOut) * n_subsets));
    uint8_t* db = (uint8_t*)dev.p;
    hipStream_t st = ctx->stream;
    HIPCHK(hipMemcpyAsync(db, vc.want.data(), sizeof(uint64_t) * vc.want.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(db + o_unk, vc.unknown.data(), sizeof(uint32_t) * vc.unknown.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(db + o_rep, vc.replace.data(), n_subsets, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(db + o_out, 0, sizeof(ValOut) * n_subsets, st));
    HIPCHK(hipStreamSynchronize(st));  // (the launches run on the batch's own streams)
    mode.d_want = (const uint64_t*)db;
    mode.d_unknown = (const uint32_t*)(db + o_unk);
    mode.d_replace = db + o_rep;
    mode.v.dev = (ValOut*)(db + o_out);
    if (int32_t rc = GeneralBatchRun(gb, cands, batched, mode)) return rc;
    if (int32_t rc = mode.v.Merge(st, batched)) return rc;
  }
  for (int s : single)
    if (int32_t rc = mode.SimOne(cands[s], s)) return rc;
  ValOut stamp{};
  stamp.verdict = KP_INVALID_BUDGET, stamp.blocked = 1;
  mode.v.Emit(blocked, stamp, out);
  return KP_OK;
}

int32_t kp_cluster_validate(kp_cluster_plan* plan, kp_cancel* cancel, const uint32_t* offsets, const uint32_t* nodes,
                            uint32_t n_subsets, const kp_command_check* checks, const uint32_t* allowed,
                            uint32_t n_allowed, kp_validation* out, uint64_t* n_blocked, kp_solve_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  if (n_blocked) *n_blocked = 0;
  if (!plan || (n_subsets && (!offsets || !out || !checks))) return fail(KP_E_INVAL, "null argument");
  if (cancel && cancel->ctx.p != plan->ctx.p) return fail(KP_E_INVAL, "the cancel token belongs to another context");
  kp_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  if (stats) memset(stats, 0, sizeof *stats);
  BudgetGate gate{allowed, n_allowed};
  BudgetGate* bg = allowed ? &gate : nullptr;
  if (bg)
    if (int32_t rc = CheckBudget(plan, bg)) return rc;
  if (n_subsets == 0) return KP_OK;
  GenTotals T;
  if (plan->general) {
    gate.blocked = 0;
    memset(plan->general_phase, 0, sizeof plan->general_phase);
    if (int32_t rc = ValidateGeneralLocked(plan, cancel, offsets, nodes, n_subsets, checks, bg, out, T)) return rc;
  } else {
    if (int32_t rc = CatalogsAlive(plan->cp->B->alive)) return rc;
    ValCheck vc;
    if (int32_t rc = ValidateCompile(plan->cp->B->catalogs, plan->cp->B->TW, checks, n_subsets, vc)) return rc;
    SimArgs a;
    if (int32_t rc = SimLaunchLocked(plan, offsets, nodes, n_subsets, 0, a, cancel, bg, nullptr, &vc)) return rc;
    hipStream_t st = ctx->stream;
    vector<uint8_t> gbytes(bg ? n_subsets : 0);
    uint64_t kst[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float ms = 0;
    HIPCHK(hipMemcpyAsync(out, vc.val, sizeof(ValOut) * n_subsets, hipMemcpyDeviceToHost, st));
    if (bg) HIPCHK(hipMemcpyAsync(gbytes.data(), vc.gate, n_subsets, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(kst, a.stats, sizeof kst, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (kst[5]) return fail(KP_E_CANCELED, "validation simulations cancelled (kp_cancel_set)");
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    T = TotalsOf(kst, ms);
    for (uint32_t s = 0; s < n_subsets; s++) {
      if (bg && !gbytes[s]) {  // not simulated
        memset(&out[s], 0, sizeof out[s]);
        out[s].verdict = KP_INVALID_BUDGET;
        out[s].blocked = 1;
      } else if (out[s].n_pods == 0xFFFFFFFFu) {
        return fail(KP_E_DEVICE, "subset %u overflowed the pod queue", s);
      }
    }
    // NodePool limits: sim_kernel stops where a pod would open a second NodeClaim, judged by the limits the pass began
    // with. The first NodeClaim has taken its largest option out of its pool's remaining limits (subtractMax), so that
    // second NodeClaim may no longer exist and the pod fail instead. Such a record is settled by the subset's own
    // whole Solve (ValidateMode::SimOne); every other record is exact as the kernel left it.
    bool limited = false;
    for (uint32_t lp : plan->cp->tmpl_limit_present) limited = limited || lp != 0;
    if (limited) {
      if (!plan->cluster()) return fail(KP_E_INVAL, "the plan keeps no cluster");
      ValidateMode mode(plan, T, cancel, checks, n_subsets);  // (its counters and device time add to the sweep's)
      for (uint32_t s = 0; s < n_subsets; s++) {
        if (out[s].verdict != KP_INVALID_MULTIPLE) continue;
        if (int32_t rc = CheckNames(checks[s], s, mode.names[s])) return rc;
        const vector<uint32_t> cand(nodes + offsets[s], nodes + offsets[s + 1]);
        if (int32_t rc = mode.SimOne(cand, (int)s)) return rc;
        memcpy(&out[s], &mode.v.host[s], sizeof out[s]);
      }
    }
  }
  if (n_blocked && bg) *n_blocked = gate.blocked;
  if (stats) {
    FillStats(stats, plan, T, t0);
    if (!plan->general) {
      stats->phase_cycles[1] = plan->sim_waves[0];
      stats->phase_cycles[2] = plan->sim_waves[1];
    }
  }
  return KP_OK;
}

// ---- Disruption candidates (kp_cluster_candidates) ----------------------------------------------------------------
// The host does strings only: name ranks, the label dictionary and the shapes' bitsets once per plan, the PDB selectors
// compiled against that dictionary per call. Reasons, costs and the order are the device's (kp_cand.hip).
static_assert(sizeof(CandPool) == sizeof(kp_pool_disruption) && sizeof(CandNode) == sizeof(kp_node_disruption) &&
                  sizeof(CandPod) == sizeof(kp_pod_disruption) && sizeof(CandOut) == sizeof(kp_candidate),
              "the device records mirror the ABI's");
static_assert(sizeof(kp_candidate) == 24 && sizeof(kp_node_disruption) == 40 && sizeof(kp_pod_disruption) == 16, "ABI sizes");

static string PairAtom(const char* key, const char* value) {
  string k = "P";
  k += key;
  k += '\0';
  k += value ? value : "";
  return k;
}

static int32_t CandBuild(kp_cluster_plan* plan) {
  kp_ctx* ctx = plan->ctx;
  const kp_cluster& cl = plan->cluster()->cl;
  const uint32_t N = cl.n_nodes, P = cl.n_pods, S = cl.n_shapes;
  if (plan->n_pools >= 0xFFFF)
    return fail(KP_E_UNSUPPORTED, "candidates over %u NodePools (max 65534)", plan->n_pools);
  auto cs = std::make_unique<CandState>();
  vector<uint32_t> off(N + 1, 0), pods, pod_shape(P), st(N), rank(N), inv(N);
  for (uint32_t i = 0; i < N; i++) {
    const kp_cluster_node& n = cl.nodes[i];
    if (n.n_pods && !n.pods) return fail(KP_E_INVAL, "node %u: null pods", i);
    for (uint32_t j = 0; j < n.n_pods; j++) {
      if (n.pods[j] >= P) return fail(KP_E_INVAL, "node %u lists pod %u of %u", i, n.pods[j], P);
      pods.push_back(n.pods[j]);
    }
    if (pods.size() > 0xFFFFFFFFull) return fail(KP_E_UNSUPPORTED, "more than 2^32 pod references");
    off[i + 1] = (uint32_t)pods.size();
    const uint16_t pool = plan->node_pool[i];
    st[i] = (pool == 0xFFFF ? CAND_ST_UNMANAGED : 0) | (n.node.initialized ? 0 : CAND_ST_UNINITIALIZED) |
            (n.deleting ? CAND_ST_DELETING : 0) | ((uint32_t)pool << 16);
  }
  for (uint32_t p = 0; p < P; p++) {
    if (cl.pods[p].shape >= S) return fail(KP_E_INVAL, "pod %u names shape %u of %u", p, cl.pods[p].shape, S);
    pod_shape[p] = cl.pods[p].shape;
  }
  {  // name ranks: bytes, then index, so that they are distinct
    auto name = [&](uint32_t i) { return std::string_view(cl.nodes[i].node.name ? cl.nodes[i].node.name : ""); };
    for (uint32_t i = 0; i < N; i++) inv[i] = i;
    std::sort(inv.begin(), inv.end(), [&](uint32_t x, uint32_t y) {
      const int c = name(x).compare(name(y));
      return c != 0 ? c < 0 : x < y;
    });
    for (uint32_t r = 0; r < N; r++) rank[inv[r]] = r;
  }
  vector<uint32_t> shape_ns(S);
  vector<vector<uint32_t>> shape_atoms(S);
  for (uint32_t s = 0; s < S; s++) {
    const kp_pod_shape& sh = cl.shapes[s];
    if (sh.n_labels && !sh.labels) return fail(KP_E_INVAL, "shape %u: null labels", s);
    shape_ns[s] = cs->ns_id.emplace(sh.namespace_ ? sh.namespace_ : "", (uint32_t)cs->ns_id.size()).first->second;
    for (uint32_t j = 0; j < sh.n_labels; j++) {
      if (!sh.labels[j].key) return fail(KP_E_INVAL, "shape %u: null label key", s);
      auto& ids = cs->atom_id;
      shape_atoms[s].push_back(ids.emplace(PairAtom(sh.labels[j].key, sh.labels[j].value), (uint32_t)ids.size()).first->second);
      shape_atoms[s].push_back(ids.emplace(string("K") + sh.labels[j].key, (uint32_t)ids.size()).first->second);
    }
  }
  if (cs->atom_id.size() >= (1u << 28))
    return fail(KP_E_UNSUPPORTED, "%zu distinct labels and label keys over the shapes (max 2^28 - 1)", cs->atom_id.size());
  const int W = (int)std::max<size_t>(1, (cs->atom_id.size() + 63) / 64);
  vector<uint64_t> bits((size_t)S * W, 0);
  for (uint32_t s = 0; s < S; s++)
    for (uint32_t id : shape_atoms[s]) bits[(size_t)s * W + (id >> 6)] |= 1ull << (id & 63);
  Blob blob;
  const size_t o_off = blob.put(off), o_pods = blob.put(pods), o_shape = blob.put(pod_shape), o_st = blob.put(st),
               o_rank = blob.put(rank), o_inv = blob.put(inv), o_bits = blob.put(bits), o_ns = blob.put(shape_ns);
  HIPCHK(cs->buf.alloc(blob.total()));
  uint8_t* base = (uint8_t*)cs->buf.p;
  HIPCHK(hipMemcpyAsync(base, blob.host.data(), blob.host.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  CandArgs& a = cs->a;
  a.node_off = (const uint32_t*)(base + o_off), a.node_pods = (const uint32_t*)(base + o_pods);
  a.pod_shape = (const uint32_t*)(base + o_shape), a.node_static = (const uint32_t*)(base + o_st);
  a.node_rank = (const uint32_t*)(base + o_rank), a.rank_node = (const uint32_t*)(base + o_inv);
  a.shape_bits = (const uint64_t*)(base + o_bits), a.shape_ns = (const uint32_t*)(base + o_ns);
  a.n_shapes = (int)S, a.words = W, a.n_nodes = (int)N;
  uint64_t pad = CAND_TILE;
  while (pad < N) pad <<= 1;
  a.n_pad = (uint32_t)pad;
  plan->cand = std::move(cs);
  return KP_OK;
}

// One PDB's selector as tokens over the plan's dictionary; *can_match = false when it can select no pod of the snapshot
static int32_t CandCompileSelector(const CandState& cs, const kp_label_selector& sel, uint32_t p, vector<uint32_t>& tok,
                                   bool* can_match) {
  *can_match = false;
  if (sel.is_nil) return KP_OK;
  if ((sel.n_match_labels && !sel.match_labels) || (sel.n_match_expressions && !sel.match_expressions))
    return fail(KP_E_INVAL, "pdb %u: null selector array", p);
  auto atom = [&](const string& k) {
    auto f = cs.atom_id.find(k);
    return f == cs.atom_id.end() ? CAND_NONE : f->second;
  };
  const size_t start = tok.size();
  bool ok = true;
  for (uint32_t j = 0; j < sel.n_match_labels; j++) {
    if (!sel.match_labels[j].key) return fail(KP_E_INVAL, "pdb %u: null selector key", p);
    const uint32_t id = atom(PairAtom(sel.match_labels[j].key, sel.match_labels[j].value));
    if (id == CAND_NONE) ok = false;
    else tok.push_back(CAND_TOK_MUST | id);
  }
  for (uint32_t j = 0; j < sel.n_match_expressions; j++) {
    const kp_selector_requirement& e = sel.match_expressions[j];
    if (!e.key) return fail(KP_E_INVAL, "pdb %u: null selector key", p);
    if (e.n_values && !e.values) return fail(KP_E_INVAL, "pdb %u: null selector values", p);
    for (uint32_t v = 0; v < e.n_values; v++)
      if (!e.values[v]) return fail(KP_E_INVAL, "pdb %u: null selector value", p);
    switch (e.op) {
      case KP_SEL_IN: {
        const size_t first = tok.size();
        for (uint32_t v = 0; v < e.n_values; v++) {
          const uint32_t id = atom(PairAtom(e.key, e.values[v]));
          if (id != CAND_NONE) tok.push_back(CAND_TOK_ANY | id);
        }
        if (tok.size() == first) ok = false;
        else tok.back() |= CAND_TOK_END;
        break;
      }
      case KP_SEL_NOT_IN:
        for (uint32_t v = 0; v < e.n_values; v++) {
          const uint32_t id = atom(PairAtom(e.key, e.values[v]));
          if (id != CAND_NONE) tok.push_back(CAND_TOK_MUSTNOT | id);
        }
        break;
      case KP_SEL_EXISTS:
      case KP_SEL_DOES_NOT_EXIST: {
        const uint32_t id = atom(string("K") + e.key);
        if (id != CAND_NONE) tok.push_back((e.op == KP_SEL_EXISTS ? CAND_TOK_MUST : CAND_TOK_MUSTNOT) | id);
        else if (e.op == KP_SEL_EXISTS) ok = false;
        break;
      }
      default:
        return fail(KP_E_INVAL, "pdb %u: selector operator %d", p, e.op);
    }
  }
  if (!ok) tok.resize(start);
  *can_match = ok;
  return KP_OK;
}

int32_t kp_cluster_candidates(kp_cluster_plan* plan, const kp_candidates_in* in, kp_candidate* out, uint32_t* order,
                              uint32_t* n_candidates, kp_solve_stats* stats) {
  if (n_candidates) *n_candidates = 0;
  if (!plan || !in || !n_candidates) return fail(KP_E_INVAL, "null argument");
  kp_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  if (stats) memset(stats, 0, sizeof *stats);
  const auto t0 = std::chrono::steady_clock::now();
  const OwnedCluster* oc = plan->cluster();
  if (!oc) return fail(KP_E_INVAL, "the plan holds no cluster");
  if (plan->general) {
    if (int32_t rc = CatalogsAlive(oc->alive)) return rc;
  } else {  // a plan of the batched simulation kernel: kp_cluster_simulate's stale-plan refusal
    if (int32_t rc = CatalogsAlive(plan->cp->B->alive)) return rc;
    if (SeqnumsOf(plan->cp->B->catalogs) != plan->cp->B->seqnums)
      return fail(KP_E_INVAL, "stale plan: a catalogue's seqnum changed since it was prepared (kp_cluster_refresh)");
  }
  const kp_cluster& cl = oc->cl;
  if (in->n_pools != cl.n_nodepools || in->n_nodes != cl.n_nodes || in->n_pods != cl.n_pods)
    return fail(KP_E_INVAL, "candidates for %u NodePools, %u nodes, %u pods; the plan's snapshot has %u, %u, %u", in->n_pools,
                in->n_nodes, in->n_pods, cl.n_nodepools, cl.n_nodes, cl.n_pods);
  if ((in->n_pools && !in->pools) || (in->n_nodes && !in->nodes) || (in->n_pods && !in->pods) || (in->n_pdbs && !in->pdbs))
    return fail(KP_E_INVAL, "null pools, nodes, pods or pdbs");
  if (in->n_nodes && (!out || !order)) return fail(KP_E_INVAL, "null out or order");
  if (in->method < KP_METHOD_EMPTINESS || in->method > KP_METHOD_DRIFT) return fail(KP_E_INVAL, "method %d", in->method);
  if (!plan->cand)
    if (int32_t rc = CandBuild(plan)) return rc;
  CandState& cs = *plan->cand;
  const uint32_t N = in->n_nodes, B = in->n_pdbs;
  // the PDBs against the plan's dictionary
  vector<uint32_t> pdb_ns(B), tok_off(B + 1, 0), tok;
  vector<uint8_t> blocks(B, 0);
  for (uint32_t p = 0; p < B; p++) {
    const kp_pdb& b = in->pdbs[p];
    bool can = false;
    if (int32_t rc = CandCompileSelector(cs, b.selector, p, tok, &can)) return rc;
    if (tok.size() >= (1ull << 31)) return fail(KP_E_UNSUPPORTED, "2^31 or more selector terms");
    tok_off[p + 1] = (uint32_t)tok.size();
    auto f = cs.ns_id.find(b.namespace_ ? b.namespace_ : "");
    pdb_ns[p] = f == cs.ns_id.end() ? CAND_NONE : f->second;
    blocks[p] = can && b.disruptions_allowed == 0 && pdb_ns[p] != CAND_NONE;
  }
  if (N == 0) return KP_OK;
  CandArgs a = cs.a;
  Blob blob;
  const size_t o_pools = blob.put(in->pools, in->n_pools), o_nodes = blob.put(in->nodes, N),
               o_pods = blob.put(in->pods, in->n_pods), o_pns = blob.put(pdb_ns), o_blk = blob.put(blocks),
               o_toff = blob.put(tok_off), o_tok = blob.put(tok);
  const size_t o_verdict = blob.reserve_dev(sizeof(uint32_t) * std::max(a.n_shapes, 1)),
               o_out = blob.reserve_dev(sizeof(CandOut) * N), o_keys = blob.reserve_dev(sizeof(uint64_t) * a.n_pad),
               o_ranks = blob.reserve_dev(sizeof(uint32_t) * a.n_pad), o_order = blob.reserve_dev(sizeof(uint32_t) * N),
               o_n = blob.reserve_dev(sizeof(uint32_t));
  if (blob.total() > cs.call_bytes) {
    HIPCHK(cs.call.alloc(blob.total()));
    cs.call_bytes = blob.total();
  }
  uint8_t* base = (uint8_t*)cs.call.p;
  a.pools = (const CandPool*)(base + o_pools), a.nodes = (const CandNode*)(base + o_nodes);
  a.pods = (const CandPod*)(base + o_pods), a.pdb_ns = (const uint32_t*)(base + o_pns);
  a.pdb_blocks = base + o_blk, a.pdb_tok_off = (const uint32_t*)(base + o_toff), a.pdb_tok = (const uint32_t*)(base + o_tok);
  a.n_pdbs = (int)B;
  a.verdict = (uint32_t*)(base + o_verdict), a.out = (CandOut*)(base + o_out), a.keys = (uint64_t*)(base + o_keys);
  a.ranks = (uint32_t*)(base + o_ranks), a.order = (uint32_t*)(base + o_order), a.n_cand = (uint32_t*)(base + o_n);
  a.now = in->now_unix, a.method = in->method;
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(base, blob.host.data(), blob.host.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ctx->ev0, st));
  HIPCHK(launch_candidates(a, st));
  HIPCHK(hipEventRecord(ctx->ev1, st));
  uint32_t n = 0;
  HIPCHK(hipMemcpyAsync(out, a.out, sizeof(CandOut) * N, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(order, a.order, sizeof(uint32_t) * N, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&n, a.n_cand, sizeof n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (n > N) return fail(KP_E_DEVICE, "the device counted %u candidates of %u nodes", n, N);
  *n_candidates = n;
  if (stats) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    stats->device_ms = ms;
    stats->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return KP_OK;
}

}  // extern "C"

// ---- Drift detection (kp_cluster_detect_drift) ---------------------------------------------------------------------
// The host does strings only. Once per plan (DriftBuild): the node -> pool table, each node's type inside its pool's
// catalogue, the nodes' label values as ids of per-key dictionaries, each pool's merged requirement per key evaluated
// against that dictionary into a bitset, and the requirement rows of the types the nodes run. Per call: the hashes and
// ids interned, the id lists sorted, the AMI requirements compiled into tokens. The ladder is the device's
// (kp_driftdet.hip).
static_assert(sizeof(DrOut) == sizeof(kp_node_drift) && sizeof(kp_node_drift) == 16, "DrOut mirrors kp_node_drift");

namespace {
// scheduling.Requirement on strings: a value set or its complement, with the Gt / Lt bounds a complement carries
struct SReq {
  std::set<string> values;
  bool complement = false, has_gt = false, has_lt = false;
  int64_t gt = 0, lt = 0;
  // Operator() is NotIn or DoesNotExist
  bool NegOp() const { return complement ? !values.empty() : values.empty(); }
  bool Within(const string& v) const {
    if (!has_gt && !has_lt) return true;
    int64_t x;
    if (!Atoi(v, &x)) return false;
    return !(has_gt && gt >= x) && !(has_lt && lt <= x);
  }
  // Intersection(In {v}, *this) is not empty
  bool Admits(const string& v) const { return (values.count(v) != 0) != complement && Within(v); }
};
SReq SReqOf(const kp_requirement& q) {  // NewRequirement
  SReq r;
  auto val = [&](uint32_t j) { return string(q.values[j] ? q.values[j] : ""); };
  if (q.op == KP_OP_IN) {
    for (uint32_t j = 0; j < q.n_values; j++) r.values.insert(val(j));
    return r;
  }
  r.complement = q.op != KP_OP_DOES_NOT_EXIST;
  if (q.op == KP_OP_NOT_IN)
    for (uint32_t j = 0; j < q.n_values; j++) r.values.insert(val(j));
  if (q.op == KP_OP_GT || q.op == KP_OP_LT) {
    int64_t x = 0;
    if (q.n_values) (void)Atoi(val(0), &x);  // validated upstream; an Atoi error leaves 0
    if (q.op == KP_OP_GT) r.has_gt = true, r.gt = x;
    else r.has_lt = true, r.lt = x;
  }
  return r;
}
SReq SReqMerge(const SReq& a, const SReq& b) {  // Requirement.Intersection, what Requirements.Add keeps
  SReq o;
  const bool hg = a.has_gt || b.has_gt, hl = a.has_lt || b.has_lt;
  const int64_t gt = a.has_gt && b.has_gt ? std::max(a.gt, b.gt) : a.has_gt ? a.gt : b.gt;
  const int64_t lt = a.has_lt && b.has_lt ? std::min(a.lt, b.lt) : a.has_lt ? a.lt : b.lt;
  if (hg && hl && gt >= lt) return o;  // DoesNotExist
  SReq bound;
  bound.has_gt = hg, bound.gt = gt, bound.has_lt = hl, bound.lt = lt;
  if (a.complement && b.complement) {
    o.values = a.values;
    o.values.insert(b.values.begin(), b.values.end());
  } else {
    const SReq& pos = a.complement ? b : a;
    const SReq& other = a.complement ? a : b;
    for (auto& v : pos.values)
      if ((other.values.count(v) != 0) != other.complement) o.values.insert(v);
  }
  for (auto it = o.values.begin(); it != o.values.end();)
    it = bound.Within(*it) ? std::next(it) : o.values.erase(it);
  o.complement = a.complement && b.complement;
  if (o.complement) o.has_gt = hg, o.gt = gt, o.has_lt = hl, o.lt = lt;
  return o;
}
int32_t CheckReqs(const kp_requirements& r, const char* who, uint32_t i, uint32_t j) {
  if (r.n && !r.items) return fail(KP_E_INVAL, "%s %u.%u: null requirements", who, i, j);
  for (uint32_t k = 0; k < r.n; k++) {
    const kp_requirement& q = r.items[k];
    if (!q.key) return fail(KP_E_INVAL, "%s %u.%u: null requirement key", who, i, j);
    if (q.op < KP_OP_IN || q.op > KP_OP_LT) return fail(KP_E_INVAL, "%s %u.%u: operator %d", who, i, j, q.op);
    if (q.n_values && !q.values) return fail(KP_E_INVAL, "%s %u.%u: null values", who, i, j);
    for (uint32_t v = 0; v < q.n_values; v++)
      if (!q.values[v]) return fail(KP_E_INVAL, "%s %u.%u: null value", who, i, j);
  }
  return KP_OK;
}
// requirements merged per normalized key, in key order
int32_t MergeReqs(const kp_requirements& r, std::map<string, SReq>& out) {
  for (uint32_t k = 0; k < r.n; k++) {
    const SReq q = SReqOf(r.items[k]);
    auto ins = out.emplace(Normalize(r.items[k].key), q);
    if (!ins.second) ins.first->second = SReqMerge(q, ins.first->second);
  }
  return KP_OK;
}
}  // namespace

// The dictionary of a set of instance types' requirements (an AMI's requirements are compiled against it)
struct TypeDict {
  std::unordered_map<string, uint32_t> tkey_id;           // keys of the types' requirements
  vector<std::unordered_map<string, uint32_t>> tval_id;   // per such key the values some type holds
  vector<vector<string>> tvals;                           // the same by id
};
// Each type's requirements merged per key, their keys and values entered into d
static int32_t TypeRows(const vector<const HostType*>& types, TypeDict& d, vector<std::map<string, SReq>>& treqs) {
  treqs.assign(types.size(), {});
  for (size_t u = 0; u < types.size(); u++) {
    const HostType& ht = *types[u];
    for (const RawReq& r : ht.reqs) {
      const char* none = nullptr;
      vector<const char*> vp;
      for (auto& v : r.values) vp.push_back(v.c_str());
      kp_requirement q{r.key.c_str(), r.op, -1, vp.empty() ? &none : vp.data(), (uint32_t)vp.size(), 0};
      const SReq s = SReqOf(q);
      auto ins = treqs[u].emplace(Normalize(r.key), s);
      if (!ins.second) ins.first->second = SReqMerge(s, ins.first->second);
    }
    for (auto& kv : treqs[u]) {
      if (kv.second.complement)
        return fail(KP_E_UNSUPPORTED, "instance type %s: a NotIn / Exists / Gt / Lt requirement on %s", ht.name.c_str(), kv.first.c_str());
      const uint32_t k = d.tkey_id.emplace(kv.first, (uint32_t)d.tkey_id.size()).first->second;
      if (k >= d.tval_id.size()) d.tval_id.resize(k + 1), d.tvals.resize(k + 1);
      for (auto& v : kv.second.values)
        if (d.tval_id[k].emplace(v, (uint32_t)d.tval_id[k].size()).second) d.tvals[k].push_back(v);
    }
  }
  return KP_OK;
}

struct DriftState : TypeDict {                            // (the dictionary of the used types)
  DevBuf buf;
  DriftDetArgs a{};                                          // the resident half of the kernel arguments
  vector<vector<uint32_t>> pool_types;                    // per pool the distinct used types its nodes run
  DevBuf call;
  size_t call_bytes = 0;
};

static int32_t DriftBuild(kp_cluster_plan* plan) {
  kp_ctx* ctx = plan->ctx;
  const kp_cluster& cl = plan->cluster()->cl;
  const uint32_t N = cl.n_nodes, P = cl.n_nodepools;
  if (P >= 0xFFFF) return fail(KP_E_UNSUPPORTED, "drift detection over %u NodePools (max 65534)", P);
  auto ds = std::make_shared<DriftState>();
  // the pools' requirements: the union of their keys, each pool's merged requirement per key
  std::unordered_map<string, uint32_t> key_id;
  struct PoolKey {
    uint32_t key, first;
    SReq req;
  };
  vector<vector<PoolKey>> pkeys(P);
  for (uint32_t p = 0; p < P; p++) {
    const kp_requirements& r = cl.nodepools[p].requirements;
    if (int32_t rc = CheckReqs(r, "NodePool", p, 0)) return rc;
    std::unordered_map<uint32_t, size_t> at;
    for (uint32_t j = 0; j < r.n; j++) {
      const uint32_t k = key_id.emplace(Normalize(r.items[j].key), (uint32_t)key_id.size()).first->second;
      const SReq q = SReqOf(r.items[j]);
      auto f = at.find(k);
      if (f == at.end()) {
        at.emplace(k, pkeys[p].size());
        pkeys[p].push_back({k, j, q});
      } else {
        pkeys[p][f->second].req = SReqMerge(q, pkeys[p][f->second].req);
      }
    }
    if (pkeys[p].size() > 0xFFFF) return fail(KP_E_UNSUPPORTED, "NodePool %u names %zu distinct keys (max 65535)", p, pkeys[p].size());
  }
  const uint32_t K = (uint32_t)key_id.size();
  if (K >= (1u << 28)) return fail(KP_E_UNSUPPORTED, "%u distinct requirement keys (max 2^28 - 1)", K);
  // the nodes' values under those keys, key-major; two labels that normalize to one key with different values leave
  // DoesNotExist, which Compatible treats as it treats a missing label
  vector<std::unordered_map<string, uint32_t>> val_id(K);
  vector<vector<string>> vals(K);
  vector<uint32_t> node_val((size_t)K * N, DR_NONE), node_pool(std::max<uint32_t>(N, 1), DR_NONE), node_type(std::max<uint32_t>(N, 1), DR_NONE);
  vector<uint8_t> clash((size_t)K, 0);
  for (uint32_t i = 0; i < N; i++) {
    const kp_existing_node& n = cl.nodes[i].node;
    if (n.n_labels && !n.labels) return fail(KP_E_INVAL, "node %u: null labels", i);
    std::fill(clash.begin(), clash.end(), 0);
    for (uint32_t j = 0; j < n.n_labels && K; j++) {
      if (!n.labels[j].key) return fail(KP_E_INVAL, "node %u: null label key", i);
      auto f = key_id.find(Normalize(n.labels[j].key));
      if (f == key_id.end()) continue;
      const uint32_t k = f->second;
      const string v = n.labels[j].value ? n.labels[j].value : "";
      auto ins = val_id[k].emplace(v, (uint32_t)val_id[k].size());
      if (ins.second) vals[k].push_back(v);
      uint32_t& slot = node_val[(size_t)k * N + i];
      if (clash[k] || (slot != DR_NONE && slot != ins.first->second)) clash[k] = 1, slot = DR_NONE;
      else slot = ins.first->second;
    }
    if (plan->node_pool[i] != 0xFFFF) node_pool[i] = plan->node_pool[i];
  }
  // each pool's merged requirements against the dictionaries
  vector<uint32_t> pool_key_off(P + 1, 0), pk_key, pk_first, pk_bits;
  vector<uint64_t> pass_bits;
  for (uint32_t p = 0; p < P; p++) {
    for (const PoolKey& e : pkeys[p]) {
      if (e.first >= DR_ABSENT_PASSES || pass_bits.size() >= 0xFFFFFFFFull) return fail(KP_E_UNSUPPORTED, "NodePool %u: too many requirements", p);
      pk_key.push_back(e.key);
      pk_first.push_back(e.first | (e.req.NegOp() ? DR_ABSENT_PASSES : 0));
      pk_bits.push_back((uint32_t)pass_bits.size());
      const size_t base = pass_bits.size();
      pass_bits.resize(base + std::max<size_t>(1, (vals[e.key].size() + 63) / 64), 0);
      for (size_t v = 0; v < vals[e.key].size(); v++)
        if (e.req.Admits(vals[e.key][v])) pass_bits[base + (v >> 6)] |= 1ull << (v & 63);
    }
    pool_key_off[p + 1] = (uint32_t)pk_key.size();
  }
  // each node's type inside its pool's catalogue, and the distinct (catalogue, type) pairs: the used types
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> used;
  vector<std::pair<uint32_t, uint32_t>> used_list;
  vector<std::unordered_map<string, uint32_t>> by_name(cl.n_catalogs);
  vector<std::set<uint32_t>> pool_types(P);
  for (uint32_t i = 0; i < N; i++) {
    if (node_pool[i] == DR_NONE) continue;
    const kp_cluster_node& n = cl.nodes[i];
    const uint32_t pc = cl.nodepools[node_pool[i]].catalog;
    if (pc >= cl.n_catalogs) return fail(KP_E_INVAL, "NodePool %u names catalogue %u of %u", node_pool[i], pc, cl.n_catalogs);
    const vector<HostType>& ptypes = cl.catalogs[pc]->types;
    uint32_t t = DR_NONE;
    if (n.catalog == pc) {
      if (n.instance_type < ptypes.size()) t = n.instance_type;
    } else if (n.catalog < cl.n_catalogs && n.instance_type < cl.catalogs[n.catalog]->types.size()) {
      auto& names = by_name[pc];
      if (names.empty())
        for (uint32_t x = 0; x < ptypes.size(); x++) names.emplace(ptypes[x].name, x);
      auto f = names.find(cl.catalogs[n.catalog]->types[n.instance_type].name);
      if (f != names.end()) t = f->second;
    }
    if (t == DR_NONE) continue;
    auto ins = used.emplace(std::make_pair(pc, t), (uint32_t)used.size());
    if (ins.second) used_list.push_back({pc, t});
    node_type[i] = ins.first->second;
    pool_types[node_pool[i]].insert(ins.first->second);
  }
  const uint32_t U = (uint32_t)used_list.size();
  ds->pool_types.resize(P);
  for (uint32_t p = 0; p < P; p++) ds->pool_types[p].assign(pool_types[p].begin(), pool_types[p].end());
  // the used types' requirement rows: keys, per key the values some used type holds, per (type, key) the held set
  vector<std::map<string, SReq>> treqs;
  vector<const HostType*> used_types(U);
  for (uint32_t u = 0; u < U; u++) used_types[u] = &cl.catalogs[used_list[u].first]->types[used_list[u].second];
  if (int32_t rc = TypeRows(used_types, *ds, treqs)) return rc;
  const uint32_t TK = (uint32_t)ds->tkey_id.size();
  if (TK > DR_TOK_KEY) return fail(KP_E_UNSUPPORTED, "%u distinct keys over the instance types (max 2^24 - 1)", TK);
  vector<uint32_t> tkey_off(std::max<uint32_t>(TK, 1), 0);
  size_t TW = 0;
  for (uint32_t k = 0; k < TK; k++) {
    tkey_off[k] = (uint32_t)TW;
    TW += std::max<size_t>(1, (ds->tvals[k].size() + 63) / 64);
  }
  if (TW > 0x7FFFFFFFull || (uint64_t)U * std::max<uint32_t>(TK, 1) > 0x7FFFFFFFull)
    return fail(KP_E_UNSUPPORTED, "the instance types' requirement table is too large");
  vector<uint32_t> type_cnt((size_t)U * TK, DR_NONE);
  vector<uint64_t> type_bits((size_t)U * TW, 0);
  for (uint32_t u = 0; u < U; u++)
    for (auto& kv : treqs[u]) {
      const uint32_t k = ds->tkey_id[kv.first];
      type_cnt[(size_t)u * TK + k] = (uint32_t)kv.second.values.size();
      for (auto& v : kv.second.values) {
        const uint32_t id = ds->tval_id[k][v];
        type_bits[(size_t)u * TW + tkey_off[k] + (id >> 6)] |= 1ull << (id & 63);
      }
    }
  Blob blob;
  const size_t o_pool = blob.put(node_pool), o_type = blob.put(node_type), o_val = blob.put(node_val),
               o_koff = blob.put(pool_key_off), o_pkk = blob.put(pk_key), o_pkf = blob.put(pk_first),
               o_pkb = blob.put(pk_bits), o_pass = blob.put(pass_bits), o_tcnt = blob.put(type_cnt),
               o_tbits = blob.put(type_bits), o_toff = blob.put(tkey_off);
  HIPCHK(ds->buf.alloc(blob.total()));
  uint8_t* base = (uint8_t*)ds->buf.p;
  HIPCHK(hipMemcpyAsync(base, blob.host.data(), blob.host.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  DriftDetArgs& a = ds->a;
  a.node_pool = (const uint32_t*)(base + o_pool), a.node_type = (const uint32_t*)(base + o_type);
  a.node_val = (const uint32_t*)(base + o_val), a.pool_key_off = (const uint32_t*)(base + o_koff);
  a.pk_key = (const uint32_t*)(base + o_pkk), a.pk_first = (const uint32_t*)(base + o_pkf);
  a.pk_bits = (const uint32_t*)(base + o_pkb), a.pass_bits = (const uint64_t*)(base + o_pass);
  a.type_cnt = (const uint32_t*)(base + o_tcnt), a.type_bits = (const uint64_t*)(base + o_tbits);
  a.tkey_off = (const uint32_t*)(base + o_toff);
  a.n_types = (int)U, a.n_tkeys = (int)TK, a.type_words = (int)TW, a.n_nodes = (int)N;
  plan->drift = std::move(ds);
  return KP_OK;
}

// One AMI's requirements as tokens over the types' dictionary (kp_driftdet.h)
static void DriftCompileAmi(const TypeDict& ds, const std::map<string, SReq>& reqs, vector<uint32_t>& tok) {
  const size_t start = tok.size();
  for (auto& kv : reqs) {
    const SReq& r = kv.second;
    auto f = ds.tkey_id.find(kv.first);
    if (f == ds.tkey_id.end()) {  // no type defines the key
      if (r.NegOp()) continue;
      tok.resize(start);
      tok.push_back(DR_TOK_NEVER);
      return;
    }
    const uint32_t k = f->second;
    const size_t hdr = tok.size();
    tok.push_back(k | (r.complement ? DR_TOK_NOT : DR_TOK_ANY) | (r.NegOp() ? DR_TOK_NEGOP : 0));
    tok.push_back(0);
    if (!r.complement) {  // a value no type carries meets nothing
      for (auto& v : r.values) {
        auto id = ds.tval_id[k].find(v);
        if (id != ds.tval_id[k].end()) tok.push_back(id->second);
      }
    } else {              // ... and is refused in vain
      for (uint32_t id = 0; id < ds.tvals[k].size(); id++)
        if (r.values.count(ds.tvals[k][id]) || !r.Within(ds.tvals[k][id])) tok.push_back(id);
    }
    tok[hdr + 1] = (uint32_t)(tok.size() - hdr - 2);
  }
}

extern "C" {

int32_t kp_cluster_detect_drift(kp_cluster_plan* plan, const kp_drift_in* in, kp_node_drift* out, uint64_t* counts,
                                kp_solve_stats* stats) {
  if (!plan || !in) return fail(KP_E_INVAL, "null argument");
  if (!out && !counts) return fail(KP_E_INVAL, "null out and counts");
  kp_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  if (stats) memset(stats, 0, sizeof *stats);
  const auto t0 = std::chrono::steady_clock::now();
  const OwnedCluster* oc = plan->cluster();
  if (!oc) return fail(KP_E_INVAL, "the plan holds no cluster");
  if (plan->general) {
    if (int32_t rc = CatalogsAlive(oc->alive)) return rc;
  } else {  // a plan of the batched simulation kernel: kp_cluster_simulate's stale-plan refusal
    if (int32_t rc = CatalogsAlive(plan->cp->B->alive)) return rc;
    if (SeqnumsOf(plan->cp->B->catalogs) != plan->cp->B->seqnums)
      return fail(KP_E_INVAL, "stale plan: a catalogue's seqnum changed since it was prepared (kp_cluster_refresh)");
  }
  const kp_cluster& cl = oc->cl;
  if (in->n_pools != cl.n_nodepools || in->n_nodes != cl.n_nodes)
    return fail(KP_E_INVAL, "drift inputs for %u NodePools, %u nodes; the plan's snapshot has %u, %u", in->n_pools, in->n_nodes,
                cl.n_nodepools, cl.n_nodes);
  if ((in->n_pools && !in->pools) || (in->n_nodes && !in->nodes) || (in->n_nodeclasses && !in->nodeclasses))
    return fail(KP_E_INVAL, "null nodeclasses, pools or nodes");
  const uint32_t N = in->n_nodes, P = in->n_pools, C = in->n_nodeclasses;
  if (C > 0x7FFFFFFFu) return fail(KP_E_UNSUPPORTED, "%u nodeclasses", C);
  for (uint32_t p = 0; p < P; p++)
    if (in->pools[p].nodeclass < -1 || in->pools[p].nodeclass >= (int32_t)C)
      return fail(KP_E_INVAL, "NodePool %u: nodeclass %d of %u", p, in->pools[p].nodeclass, C);
  for (uint32_t c = 0; c < C; c++) {
    const kp_nodeclass_status& s = in->nodeclasses[c];
    if ((s.n_amis && !s.amis) || (s.n_subnets && !s.subnets) || (s.n_security_groups && !s.security_groups) ||
        (s.n_capacity_reservations && !s.capacity_reservations))
      return fail(KP_E_INVAL, "nodeclass %u: null array", c);
    for (uint32_t j = 0; j < s.n_amis; j++) {
      if (!s.amis[j].id) return fail(KP_E_INVAL, "nodeclass %u: AMI %u has a null id", c, j);
      if (int32_t rc = CheckReqs(s.amis[j].requirements, "AMI", c, j)) return rc;
    }
    for (uint32_t j = 0; j < s.n_subnets; j++)
      if (!s.subnets[j]) return fail(KP_E_INVAL, "nodeclass %u: null subnet id", c);
    for (uint32_t j = 0; j < s.n_security_groups; j++)
      if (!s.security_groups[j]) return fail(KP_E_INVAL, "nodeclass %u: null security-group id", c);
    for (uint32_t j = 0; j < s.n_capacity_reservations; j++)
      if (!s.capacity_reservations[j]) return fail(KP_E_INVAL, "nodeclass %u: null capacity-reservation id", c);
  }
  for (uint32_t i = 0; i < N; i++) {
    const kp_node_drift_in& n = in->nodes[i];
    if (!(n.flags & KP_DRIFT_HAS_INSTANCE)) continue;
    if (!n.image_id || !n.subnet_id) return fail(KP_E_INVAL, "node %u: an instance with a null image or subnet id", i);
    if (n.n_security_groups && !n.security_groups) return fail(KP_E_INVAL, "node %u: null security groups", i);
    for (uint32_t j = 0; j < n.n_security_groups; j++)
      if (!n.security_groups[j]) return fail(KP_E_INVAL, "node %u: null security-group id", i);
  }
  if (!plan->drift)
    if (int32_t rc = DriftBuild(plan)) return rc;
  DriftState& ds = *plan->drift;
  const uint32_t U = (uint32_t)ds.a.n_types;
  if ((uint64_t)C * std::max<uint32_t>(U, 1) > 0x7FFFFFFFull) return fail(KP_E_UNSUPPORTED, "%u nodeclasses x %u instance types", C, U);
  // strings to integers
  std::unordered_map<string, uint32_t> ids;
  auto intern = [&](const char* s) { return s ? ids.emplace(s, (uint32_t)ids.size()).first->second : DR_NONE; };
  auto sorted_ids = [&](const char* const* s, uint32_t n, vector<uint32_t>& into) {
    const size_t lo = into.size();
    for (uint32_t j = 0; j < n; j++) into.push_back(intern(s[j]));
    std::sort(into.begin() + lo, into.end());
    into.erase(std::unique(into.begin() + lo, into.end()), into.end());
    return (uint32_t)(into.size() - lo);
  };
  vector<DrClass> classes(std::max<uint32_t>(C, 1));
  vector<uint32_t> class_ids, ami_id, ami_tok_off(1, 0), ami_tok;
  for (uint32_t c = 0; c < C; c++) {
    const kp_nodeclass_status& s = in->nodeclasses[c];
    DrClass& d = classes[c];
    d.hash = intern(s.hash), d.version = intern(s.hash_version);
    d.ami_off = (uint32_t)ami_id.size(), d.n_amis = s.n_amis;
    for (uint32_t j = 0; j < s.n_amis; j++) {
      ami_id.push_back(intern(s.amis[j].id));
      std::map<string, SReq> merged;
      MergeReqs(s.amis[j].requirements, merged);
      DriftCompileAmi(ds, merged, ami_tok);
      if (ami_tok.size() >= (1ull << 31) || ami_id.size() >= (1ull << 31)) return fail(KP_E_UNSUPPORTED, "2^31 or more AMIs or AMI terms");
      ami_tok_off.push_back((uint32_t)ami_tok.size());
    }
    d.sg_off = (uint32_t)class_ids.size(), d.n_sg = sorted_ids(s.security_groups, s.n_security_groups, class_ids);
    d.subnet_off = (uint32_t)class_ids.size(), d.n_subnets = sorted_ids(s.subnets, s.n_subnets, class_ids);
    d.res_off = (uint32_t)class_ids.size();
    d.n_res = sorted_ids(s.capacity_reservations, s.n_capacity_reservations, class_ids);
    if (class_ids.size() >= (1ull << 31)) return fail(KP_E_UNSUPPORTED, "2^31 or more nodeclass ids");
  }
  vector<DrPool> pools(std::max<uint32_t>(P, 1));
  vector<uint8_t> want((size_t)C * U, 0);
  vector<uint32_t> pairs;
  for (uint32_t p = 0; p < P; p++) {
    pools[p] = DrPool{in->pools[p].nodeclass, intern(in->pools[p].hash), intern(in->pools[p].hash_version), 0};
    if (in->pools[p].nodeclass < 0) continue;
    for (uint32_t u : ds.pool_types[p]) {
      const size_t pair = (size_t)in->pools[p].nodeclass * U + u;
      if (!want[pair]) want[pair] = 1, pairs.push_back((uint32_t)pair);
    }
  }
  vector<DrNode> nodes(std::max<uint32_t>(N, 1));
  vector<uint32_t> node_sg_off(N + 1, 0), node_sg;
  for (uint32_t i = 0; i < N; i++) {
    const kp_node_drift_in& n = in->nodes[i];
    const bool inst = (n.flags & KP_DRIFT_HAS_INSTANCE) != 0;
    nodes[i] = DrNode{inst ? KP_DRIFT_HAS_INSTANCE : 0u,
                      intern(n.nodepool_hash),
                      intern(n.nodepool_hash_version),
                      intern(n.nodeclass_hash),
                      intern(n.nodeclass_hash_version),
                      inst ? intern(n.image_id) : DR_NONE,
                      inst ? intern(n.subnet_id) : DR_NONE,
                      inst ? intern(n.capacity_reservation_id) : DR_NONE};
    if (inst) sorted_ids(n.security_groups, n.n_security_groups, node_sg);
    if (node_sg.size() >= (1ull << 31)) return fail(KP_E_UNSUPPORTED, "2^31 or more security-group references");
    node_sg_off[i + 1] = (uint32_t)node_sg.size();
  }
  DriftDetArgs a = ds.a;
  Blob blob;
  const size_t o_pools = blob.put(pools), o_nodes = blob.put(nodes), o_classes = blob.put(classes),
               o_sgoff = blob.put(node_sg_off), o_sg = blob.put(node_sg), o_cids = blob.put(class_ids),
               o_amiid = blob.put(ami_id), o_toff = blob.put(ami_tok_off), o_tok = blob.put(ami_tok),
               o_pairs = blob.put(pairs);
  const size_t o_amiof = blob.reserve_dev(sizeof(uint32_t) * std::max<size_t>((size_t)C * U, 1)),
               o_out = blob.reserve_dev(sizeof(DrOut) * std::max<uint32_t>(N, 1)),
               o_part = blob.reserve_dev(sizeof(uint64_t) * DR_REASONS * DR_COUNT_MAX_BLOCKS),
               o_counts = blob.reserve_dev(sizeof(uint64_t) * DR_REASONS);
  if (blob.total() > ds.call_bytes) {
    HIPCHK(ds.call.alloc(blob.total()));
    ds.call_bytes = blob.total();
  }
  uint8_t* base = (uint8_t*)ds.call.p;
  a.pools = (const DrPool*)(base + o_pools), a.nodes = (const DrNode*)(base + o_nodes);
  a.classes = (const DrClass*)(base + o_classes), a.node_sg_off = (const uint32_t*)(base + o_sgoff);
  a.node_sg = (const uint32_t*)(base + o_sg), a.class_ids = (const uint32_t*)(base + o_cids);
  a.ami_id = (const uint32_t*)(base + o_amiid), a.ami_tok_off = (const uint32_t*)(base + o_toff);
  a.ami_tok = (const uint32_t*)(base + o_tok), a.pairs = (const uint32_t*)(base + o_pairs);
  a.n_pairs = (int)pairs.size();
  a.ami_of = (uint32_t*)(base + o_amiof), a.out = (DrOut*)(base + o_out);
  a.part = (uint64_t*)(base + o_part), a.counts = (uint64_t*)(base + o_counts);
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(base, blob.host.data(), blob.host.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ctx->ev0, st));
  HIPCHK(launch_detect_drift(a, st));
  HIPCHK(hipEventRecord(ctx->ev1, st));
  uint64_t hist[DR_REASONS] = {};
  if (out && N) HIPCHK(hipMemcpyAsync(out, a.out, sizeof(DrOut) * N, hipMemcpyDeviceToHost, st));
  if (counts) HIPCHK(hipMemcpyAsync(hist, a.counts, sizeof hist, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (counts) memcpy(counts, hist, sizeof hist);
  if (stats) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    stats->device_ms = ms;
    stats->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return KP_OK;
}

}  // extern "C"

// ---- Interruption messages (kp_cluster_interruptions) ---------------------------------------------------------------
// The host does strings only. Once per plan (InterruptBuild): each node's (instance-type label, zone label) pair
// interned to an integer, resident with the deleting flags. Per call: every id copied into a zero-padded 32-byte slot.
// The host builds no map over ids: the join, the fold and the two compactions are the device's (kp_interrupt.hip).
static_assert(sizeof(IrNodeOut) == sizeof(kp_interrupt_node) && sizeof(IrDelete) == sizeof(kp_interrupt_delete) &&
                  sizeof(IrMark) == sizeof(kp_interrupt_mark),
              "the device records mirror the ABI's");

struct InterruptState {
  DevBuf buf;  // node_pair, node_deleting
  InterruptArgs a{};
  DevBuf call;
  size_t call_bytes = 0;
};

// What needs no plan; *n_with_id receives the number of nodes that have an id
static int32_t InterruptCheck(const kp_interrupt_in* in, uint32_t* n_with_id) {
  if (!in) return fail(KP_E_INVAL, "null argument");
  if (in->n_messages >= (1u << 31) || in->n_ids >= (1u << 31))
    return fail(KP_E_UNSUPPORTED, "%u messages, %u ids (max 2^31 - 1 each)", in->n_messages, in->n_ids);
  if (in->n_messages && (!in->kinds || !in->id_offsets)) return fail(KP_E_INVAL, "null kinds or id_offsets");
  if (in->n_ids && !in->ids) return fail(KP_E_INVAL, "null ids");
  if (in->n_nodes && !in->node_ids) return fail(KP_E_INVAL, "null node_ids");
  if (in->table_log2 > 30) return fail(KP_E_INVAL, "table_log2 %u (max 30)", in->table_log2);
  for (uint32_t m = 0; m < in->n_messages; m++)
    if (in->kinds[m] < KP_MSG_NO_OP || in->kinds[m] > KP_MSG_INSTANCE_TERMINATED)
      return fail(KP_E_INVAL, "message %u: kind %d", m, in->kinds[m]);
  if (in->id_offsets) {
    if (in->id_offsets[0] != 0) return fail(KP_E_INVAL, "id_offsets start at %u", in->id_offsets[0]);
    for (uint32_t m = 0; m < in->n_messages; m++)
      if (in->id_offsets[m + 1] < in->id_offsets[m]) return fail(KP_E_INVAL, "id_offsets decrease at message %u", m);
    if (in->id_offsets[in->n_messages] != in->n_ids)
      return fail(KP_E_INVAL, "id_offsets end at %u of %u ids", in->id_offsets[in->n_messages], in->n_ids);
  } else if (in->n_ids) {
    return fail(KP_E_INVAL, "id_offsets end at 0 of %u ids", in->n_ids);
  }
  for (uint32_t j = 0; j < in->n_ids; j++) {
    if (!in->ids[j]) return fail(KP_E_INVAL, "id %u is null", j);
    if (strnlen(in->ids[j], IR_KEY_BYTES) >= IR_KEY_BYTES)
      return fail(KP_E_UNSUPPORTED, "id %u is longer than %d bytes", j, IR_KEY_BYTES - 1);
  }
  uint32_t with_id = 0;
  for (uint32_t i = 0; i < in->n_nodes; i++) {
    if (!in->node_ids[i]) continue;
    if (strnlen(in->node_ids[i], IR_KEY_BYTES) >= IR_KEY_BYTES)
      return fail(KP_E_UNSUPPORTED, "node %u: an instance id longer than %d bytes", i, IR_KEY_BYTES - 1);
    with_id++;
  }
  if (in->table_log2 && (1ull << in->table_log2) <= with_id)
    return fail(KP_E_INVAL, "a forced table of %llu slots for %u nodes with an id", 1ull << in->table_log2, with_id);
  if (n_with_id) *n_with_id = with_id;
  return KP_OK;
}

static int32_t InterruptBuild(kp_cluster_plan* plan) {
  kp_ctx* ctx = plan->ctx;
  const kp_cluster& cl = plan->cluster()->cl;
  const uint32_t N = cl.n_nodes;
  auto is = std::make_shared<InterruptState>();
  std::map<std::pair<string, string>, uint32_t> pairs;
  vector<uint32_t> node_pair(std::max<uint32_t>(N, 1), IR_NONE);
  vector<uint8_t> deleting(std::max<uint32_t>(N, 1), 0);
  for (uint32_t i = 0; i < N; i++) {
    const kp_existing_node& n = cl.nodes[i].node;
    if (n.n_labels && !n.labels) return fail(KP_E_INVAL, "node %u: null labels", i);
    const char *type = nullptr, *zone = nullptr;
    for (uint32_t j = 0; j < n.n_labels; j++) {
      if (!n.labels[j].key) return fail(KP_E_INVAL, "node %u: null label key", i);
      if (!strcmp(n.labels[j].key, "node.kubernetes.io/instance-type")) type = n.labels[j].value;
      else if (!strcmp(n.labels[j].key, "topology.kubernetes.io/zone")) zone = n.labels[j].value;
    }
    if (type && zone && *type && *zone)
      node_pair[i] = pairs.emplace(std::make_pair(string(type), string(zone)), (uint32_t)pairs.size()).first->second;
    deleting[i] = cl.nodes[i].deleting ? 1 : 0;
  }
  Blob blob;
  const size_t o_pair = blob.put(node_pair), o_del = blob.put(deleting);
  HIPCHK(is->buf.alloc(blob.total()));
  uint8_t* base = (uint8_t*)is->buf.p;
  HIPCHK(hipMemcpyAsync(base, blob.host.data(), blob.host.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  is->a.node_pair = (const uint32_t*)(base + o_pair), is->a.node_deleting = base + o_del;
  is->a.n_pairs = (int)pairs.size(), is->a.n_nodes = (int)N;
  plan->interrupt = std::move(is);
  return KP_OK;
}

extern "C" {

int32_t kp_interruptions_validate(const kp_interrupt_in* in) { return InterruptCheck(in, nullptr); }

int32_t kp_cluster_interruptions(kp_cluster_plan* plan, const kp_interrupt_in* in, kp_interrupt_node* out_nodes,
                                 uint32_t* out_matches, kp_interrupt_delete* deletes, uint32_t* n_deletes,
                                 kp_interrupt_mark* marks, uint32_t* n_marks, uint64_t* counts, kp_solve_stats* stats) {
  if (n_deletes) *n_deletes = 0;
  if (n_marks) *n_marks = 0;
  if (!plan || !in || !n_deletes || !n_marks) return fail(KP_E_INVAL, "null argument");
  kp_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  if (stats) memset(stats, 0, sizeof *stats);
  const auto t0 = std::chrono::steady_clock::now();
  const OwnedCluster* oc = plan->cluster();
  if (!oc) return fail(KP_E_INVAL, "the plan holds no cluster");
  if (plan->general) {
    if (int32_t rc = CatalogsAlive(oc->alive)) return rc;
  } else {  // a plan of the batched simulation kernel: kp_cluster_simulate's stale-plan refusal
    if (int32_t rc = CatalogsAlive(plan->cp->B->alive)) return rc;
    if (SeqnumsOf(plan->cp->B->catalogs) != plan->cp->B->seqnums)
      return fail(KP_E_INVAL, "stale plan: a catalogue's seqnum changed since it was prepared (kp_cluster_refresh)");
  }
  if (in->n_nodes != oc->cl.n_nodes)
    return fail(KP_E_INVAL, "interruptions for %u nodes; the plan's snapshot has %u", in->n_nodes, oc->cl.n_nodes);
  uint32_t with_id = 0;
  if (int32_t rc = InterruptCheck(in, &with_id)) return rc;
  if (!plan->interrupt)
    if (int32_t rc = InterruptBuild(plan)) return rc;
  InterruptState& is = *plan->interrupt;
  const uint32_t N = in->n_nodes, M = in->n_messages, E = in->n_ids;
  if (!in->table_log2 && with_id >= (1u << 30)) return fail(KP_E_UNSUPPORTED, "%u nodes with an id", with_id);
  uint32_t slots = 2;  // chosen: the least power of two that leaves the table at most half full
  if (in->table_log2) slots = 1u << in->table_log2;
  else
    while (slots < 2 * (with_id + 1)) slots <<= 1;
  // strings to 32-byte slots
  vector<uint8_t> node_key((size_t)std::max<uint32_t>(N, 1) * IR_KEY_BYTES, 0), has_id(std::max<uint32_t>(N, 1), 0);
  for (uint32_t i = 0; i < N; i++) {
    if (!in->node_ids[i]) continue;
    has_id[i] = 1;
    memcpy(&node_key[(size_t)i * IR_KEY_BYTES], in->node_ids[i], strlen(in->node_ids[i]));
  }
  vector<uint8_t> entry_key((size_t)std::max<uint32_t>(E, 1) * IR_KEY_BYTES, 0), kind(std::max<uint32_t>(M, 1), 0);
  vector<uint32_t> entry_msg(std::max<uint32_t>(E, 1), 0);
  for (uint32_t m = 0; m < M; m++) {
    kind[m] = (uint8_t)in->kinds[m];
    for (uint32_t j = in->id_offsets[m]; j < in->id_offsets[m + 1]; j++) {
      entry_msg[j] = m;
      memcpy(&entry_key[(size_t)j * IR_KEY_BYTES], in->ids[j], strlen(in->ids[j]));
    }
  }
  InterruptArgs a = is.a;
  const size_t P = (size_t)std::max(a.n_pairs, 1), N1 = std::max<uint32_t>(N, 1), E1 = std::max<uint32_t>(E, 1);
  const size_t nb = (size_t)std::max(interrupt_blocks((int)N), 1);
  Blob blob;
  const size_t o_nkey = blob.put(node_key), o_has = blob.put(has_id), o_ekey = blob.put(entry_key),
               o_emsg = blob.put(entry_msg), o_kind = blob.put(kind);
  // the regions one fill sets to all-ones words, then those one fill zeroes: each group contiguous
  const size_t o_table = blob.reserve_dev(4 * ((size_t)slots + N1 + P));
  const size_t o_zero = blob.reserve_dev(4 * (N1 + N1 + P));
  const size_t o_sums = blob.reserve_dev(4 * IR_SUMS * nb), o_tot = blob.reserve_dev(4 * IR_SUMS),
               o_nodes = blob.reserve_dev(sizeof(IrNodeOut) * N1), o_match = blob.reserve_dev(4 * E1),
               o_del = blob.reserve_dev(sizeof(IrDelete) * N1), o_mark = blob.reserve_dev(sizeof(IrMark) * N1);
  if (blob.total() > is.call_bytes) {
    HIPCHK(is.call.alloc(blob.total()));
    is.call_bytes = blob.total();
  }
  uint8_t* base = (uint8_t*)is.call.p;
  a.node_key = (const IrKey*)(base + o_nkey), a.node_has_id = base + o_has;
  a.entry_key = (const IrKey*)(base + o_ekey), a.entry_msg = (const uint32_t*)(base + o_emsg), a.msg_kind = base + o_kind;
  a.n_nodes = (int)N, a.n_entries = (int)E, a.table_mask = slots - 1;
  a.table = (uint32_t*)(base + o_table), a.node_first = a.table + slots, a.pair_first = a.node_first + N1;
  a.node_kinds = (uint32_t*)(base + o_zero), a.node_count = a.node_kinds + N1, a.pair_count = a.node_count + N1;
  a.block_sums = (uint32_t*)(base + o_sums), a.totals = (uint32_t*)(base + o_tot);
  a.out_nodes = (IrNodeOut*)(base + o_nodes), a.out_matches = (uint32_t*)(base + o_match);
  a.deletes = (IrDelete*)(base + o_del), a.marks = (IrMark*)(base + o_mark);
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(base, blob.host.data(), blob.host.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ctx->ev0, st));
  HIPCHK(hipMemsetAsync(base + o_table, 0xFF, 4 * ((size_t)slots + N1 + P), st));
  HIPCHK(hipMemsetAsync(base + o_zero, 0, 4 * (N1 + N1 + P), st));
  HIPCHK(launch_interruptions(a, st));
  HIPCHK(hipEventRecord(ctx->ev1, st));
  uint32_t tot[IR_SUMS] = {};
  HIPCHK(hipMemcpyAsync(tot, a.totals, sizeof tot, hipMemcpyDeviceToHost, st));
  if (out_nodes && N) HIPCHK(hipMemcpyAsync(out_nodes, a.out_nodes, sizeof(IrNodeOut) * N, hipMemcpyDeviceToHost, st));
  if (out_matches && E) HIPCHK(hipMemcpyAsync(out_matches, a.out_matches, 4 * (size_t)E, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (tot[0] > N || tot[1] > N) return fail(KP_E_DEVICE, "the device counted %u deletes, %u marks over %u nodes", tot[0], tot[1], N);
  // the two lists are as long as the device counted them
  if (deletes && tot[0]) HIPCHK(hipMemcpyAsync(deletes, a.deletes, sizeof(IrDelete) * tot[0], hipMemcpyDeviceToHost, st));
  if (marks && tot[1]) HIPCHK(hipMemcpyAsync(marks, a.marks, sizeof(IrMark) * tot[1], hipMemcpyDeviceToHost, st));
  if ((deletes && tot[0]) || (marks && tot[1])) HIPCHK(hipStreamSynchronize(st));
  *n_deletes = tot[0], *n_marks = tot[1];
  if (counts) {
    for (int k = 0; k < KP_MESSAGE_KIND_COUNT; k++) counts[k] = 0;
    for (int k = KP_MSG_SCHEDULED_CHANGE; k <= KP_MSG_INSTANCE_TERMINATED; k++) counts[k] = tot[k];
  }
  if (stats) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    stats->device_ms = ms;
    stats->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return KP_OK;
}

}  // extern "C"

// ---- Launch-template configs (kp_launch_templates) ------------------------------------------------------------------
// The host does strings only. Once per launch plan (LtBuild): the requirement rows of the types its requests list against
// their own dictionary, laid out for lanes over types. Per call: the AMI requirements compiled into kp_driftdet.h's
// tokens against that dictionary; an AMI is its index. The selection never comes back to the host between launch_kernel
// and the grouping (kp_ltgroup.hip).
static_assert(sizeof(LtOut) == sizeof(kp_lt_result) && sizeof(LtConfig) == sizeof(kp_lt_config),
              "the device records mirror the ABI's");

struct LtState : TypeDict {
  DevBuf buf;  // the resident tables, ami_of and the four outputs
  LtArgs a{};
  DevBuf call;  // the call's AMI tokens
  size_t call_bytes = 0;
};

static int32_t LtCheckAmis(const kp_ami* amis, uint32_t n_amis) {
  if (n_amis > LT_MAX_AMIS) return fail(KP_E_UNSUPPORTED, "%u AMIs (max %d)", n_amis, LT_MAX_AMIS);
  if (n_amis && !amis) return fail(KP_E_INVAL, "null amis");
  for (uint32_t j = 0; j < n_amis; j++) {
    if (!amis[j].id) return fail(KP_E_INVAL, "AMI %u has a null id", j);
    if (int32_t rc = CheckReqs(amis[j].requirements, "AMI", 0, j)) return rc;
  }
  return KP_OK;
}

static int32_t LtBuild(kp_launch_plan* plan) {
  kp_ctx* ctx = plan->ctx;
  const uint32_t T = (uint32_t)plan->T, n = plan->n;
  auto ls = std::make_shared<LtState>();
  // only the types some request lists: no other row is read, and a type nobody lists refuses nothing
  const vector<uint32_t>& used = plan->used;
  vector<const HostType*> types(used.size());
  for (size_t u = 0; u < used.size(); u++) {
    const HostType& ht = plan->cat->types[used[u]];
    types[u] = &ht;
    const int64_t pods = ((ht.cap_present >> KP_RES_PODS) & 1) ? ht.cap[KP_RES_PODS] : 0;
    const int64_t efa = ((ht.cap_present >> KP_RES_EFA) & 1) ? ht.cap[KP_RES_EFA] : 0;
    if (pods < 0 || pods > 0x7FFFFFFFll * 1000) return fail(KP_E_UNSUPPORTED, "instance type %s: pods capacity %lld", ht.name.c_str(), (long long)pods);
    if (efa < 0 || efa > 65535ll * 1000) return fail(KP_E_UNSUPPORTED, "instance type %s: EFA capacity %lld", ht.name.c_str(), (long long)efa);
  }
  vector<std::map<string, SReq>> treqs;
  if (int32_t rc = TypeRows(types, *ls, treqs)) return rc;
  const uint32_t TK = (uint32_t)ls->tkey_id.size();
  vector<uint32_t> tkey_off(std::max<uint32_t>(TK, 1), 0);
  size_t TW = 0;
  for (uint32_t k = 0; k < TK; k++) {
    tkey_off[k] = (uint32_t)TW;
    TW += std::max<size_t>(1, (ls->tvals[k].size() + 63) / 64);
  }
  // (T <= 4096 on a launch plan; a key has at most T * values-per-type values)
  if (TW * std::max<uint32_t>(T, 1) > 0x7FFFFFFFull) return fail(KP_E_UNSUPPORTED, "the instance types' requirement table is too large");
  vector<uint32_t> type_cnt((size_t)TK * T, DR_NONE);
  vector<uint64_t> type_bits(TW * T, 0);
  for (size_t u = 0; u < used.size(); u++)
    for (auto& kv : treqs[u]) {
      const uint32_t k = ls->tkey_id[kv.first], t = used[u];
      type_cnt[(size_t)k * T + t] = (uint32_t)kv.second.values.size();
      for (auto& v : kv.second.values) {
        const uint32_t id = ls->tval_id[k][v];
        type_bits[((size_t)tkey_off[k] + (id >> 6)) * T + t] |= 1ull << (id & 63);
      }
    }
  const size_t n1 = std::max<uint32_t>(n, 1);
  Blob blob;
  const size_t o_tcnt = blob.put(type_cnt), o_tbits = blob.put(type_bits), o_toff = blob.put(tkey_off),
               o_used = blob.put(plan->used), o_efa = blob.put(plan->req_efa);
  const size_t o_amiof = blob.reserve_dev(sizeof(uint32_t) * std::max<uint32_t>(T, 1)),
               o_lt = blob.reserve_dev(sizeof(LtOut) * n1),
               o_tc = blob.reserve_dev(sizeof(int32_t) * n1 * plan->max_types),
               o_cfg = blob.reserve_dev(sizeof(LtConfig) * n1 * plan->ovr_stride),
               o_ovr = blob.reserve_dev(sizeof(uint32_t) * n1 * plan->ovr_stride);
  HIPCHK(ls->buf.alloc(blob.total()));
  uint8_t* base = (uint8_t*)ls->buf.p;
  HIPCHK(hipMemcpyAsync(base, blob.host.data(), blob.host.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  LtArgs& a = ls->a;
  a.type_cnt = (const uint32_t*)(base + o_tcnt), a.type_bits = (const uint64_t*)(base + o_tbits);
  a.tkey_off = (const uint32_t*)(base + o_toff), a.used = (const uint32_t*)(base + o_used);
  a.req_efa = base + o_efa;
  a.T = (int32_t)T, a.n_tkeys = (int32_t)TK, a.type_words = (int32_t)TW, a.n_used = (int32_t)plan->used.size();
  a.ami_of = (uint32_t*)(base + o_amiof), a.lt_out = (LtOut*)(base + o_lt), a.type_config = (int32_t*)(base + o_tc);
  a.configs = (LtConfig*)(base + o_cfg), a.overrides = (uint32_t*)(base + o_ovr);
  plan->lt = std::move(ls);
  return KP_OK;
}

extern "C" {

int32_t kp_launch_templates_validate(const kp_ami* amis, uint32_t n_amis) { return LtCheckAmis(amis, n_amis); }

// kp_launch_run followed by the template kernels on the same stream; results copied only into the non-NULL buffers.
int32_t kp_launch_run_templates(kp_launch_plan* plan, const kp_ami* amis, uint32_t n_amis, kp_launch_result* out,
                                uint32_t* out_types, kp_lt_result* lt_out, int32_t* out_type_config,
                                kp_lt_config* out_configs, uint32_t* out_overrides, kp_solve_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  if (!plan) return fail(KP_E_INVAL, "null argument");
  kp_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  if (int32_t rc = CatalogsAlive({plan->alive})) return rc;
  if (plan->cat->seqnum != plan->seqnum)
    return fail(KP_E_INVAL, "stale plan: catalogue seqnum %llu, plan built at %llu (kp_launch_refresh)",
                (unsigned long long)plan->cat->seqnum, (unsigned long long)plan->seqnum);
  if (int32_t rc = LtCheckAmis(amis, n_amis)) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  if (!plan->lt)
    if (int32_t rc = LtBuild(plan)) return rc;
  LtState& ls = *plan->lt;
  const auto t1 = std::chrono::steady_clock::now();
  vector<uint32_t> tok_off(1, 0), tok;
  for (uint32_t j = 0; j < n_amis; j++) {
    std::map<string, SReq> merged;
    MergeReqs(amis[j].requirements, merged);
    DriftCompileAmi(ls, merged, tok);
    if (tok.size() >= (1ull << 31)) return fail(KP_E_UNSUPPORTED, "2^31 or more AMI terms");
    tok_off.push_back((uint32_t)tok.size());
  }
  Blob blob;
  const size_t o_toff = blob.put(tok_off), o_tok = blob.put(tok);
  if (blob.total() > ls.call_bytes) {
    HIPCHK(ls.call.alloc(blob.total()));
    ls.call_bytes = blob.total();
  }
  const double compile_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
  hipStream_t st = ctx->stream;
  uint8_t* cb = (uint8_t*)ls.call.p;
  LtArgs a = ls.a;
  a.la = plan->la;
  a.ami_tok_off = (const uint32_t*)(cb + o_toff), a.ami_tok = (const uint32_t*)(cb + o_tok);
  a.n_amis = (int32_t)n_amis;
  uint8_t* base = (uint8_t*)plan->buf.p;
  const uint32_t n = plan->n;
  HIPCHK(hipMemcpyAsync(cb, blob.host.data(), blob.host.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(a.ami_of, 0xFF, sizeof(uint32_t) * std::max<int32_t>(a.T, 1), st));  // DR_NONE
  HIPCHK(hipMemsetAsync(base + plan->o_stats, 0, sizeof(uint64_t) * 2, st));
  HIPCHK(hipEventRecord(ctx->ev0, st));
  if (n) HIPCHK(launch_launch(plan->la, st));
  if (n) HIPCHK(launch_lt(a, st));
  HIPCHK(hipEventRecord(ctx->ev1, st));
  uint64_t ls_st[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(ls_st, base + plan->o_stats, sizeof ls_st, hipMemcpyDeviceToHost, st));
  const size_t nt = (size_t)n * plan->max_types, no = (size_t)n * plan->ovr_stride;
  if (n && out) HIPCHK(hipMemcpyAsync(out, base + plan->o_out, sizeof(kp_launch_result) * n, hipMemcpyDeviceToHost, st));
  if (n && out_types) HIPCHK(hipMemcpyAsync(out_types, base + plan->o_types, sizeof(uint32_t) * nt, hipMemcpyDeviceToHost, st));
  if (n && lt_out) HIPCHK(hipMemcpyAsync(lt_out, a.lt_out, sizeof(LtOut) * n, hipMemcpyDeviceToHost, st));
  if (n && out_type_config) HIPCHK(hipMemcpyAsync(out_type_config, a.type_config, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
  if (n && out_configs) HIPCHK(hipMemcpyAsync(out_configs, a.configs, sizeof(LtConfig) * no, hipMemcpyDeviceToHost, st));
  if (n && out_overrides) HIPCHK(hipMemcpyAsync(out_overrides, a.overrides, sizeof(uint32_t) * no, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->device_ms = ms;
    stats->attempts = ls_st[0];
    stats->bytes_algorithmic = ls_st[1];
    stats->prepare_ms = compile_ms;  // this call's host compile (the AMI tokens); the first call also builds the type table
    stats->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return KP_OK;
}

int32_t kp_launch_templates(kp_ctx* ctx, const kp_catalog* cat, const kp_launch_request* reqs, uint32_t n,
                            const char* const* subnet_zones, uint32_t n_subnet_zones, uint32_t max_types,
                            const kp_ami* amis, uint32_t n_amis, kp_launch_result* out, uint32_t* out_types,
                            kp_lt_result* lt_out, int32_t* out_type_config, kp_lt_config* out_configs,
                            uint32_t* out_overrides, kp_solve_stats* stats) {
  if (int32_t rc = LtCheckAmis(amis, n_amis)) return rc;
  kp_launch_plan* plan = nullptr;
  int32_t rc = kp_launch_prepare(ctx, cat, reqs, n, subnet_zones, n_subnet_zones, max_types, &plan);
  if (rc) return rc;
  rc = kp_launch_run_templates(plan, amis, n_amis, out, out_types, lt_out, out_type_config, out_configs, out_overrides, stats);
  kp_launch_plan_destroy(plan);
  return rc;
}

}  // extern "C"

// ---- The scheduler's inputs (kp_scheduler_inputs) -------------------------------------------------------------------
// The host does strings only: the templates' strict requirements merged per key (SReq), the nodes' label values as ids
// of per-key dictionaries (key-major, as DriftBuild's node_val), one bitset per (template, key), the distinct taint
// sets against the templates' tolerations, and the P x D template side with its relax loop. Every sum is the device's
// (kp_schedin.hip).
static_assert(sizeof(SiNodeOut) == sizeof(kp_sched_node_out) && sizeof(SiPoolOut) == sizeof(kp_sched_pool_out),
              "the device records mirror the ABI's");

namespace {
// Requirements.Compatible(q) on merged string requirements (oracle.cpp Compatible + Intersects)
bool SCompatible(const std::map<string, SReq>& r, const std::map<string, SReq>& q, bool allow_undefined_wellknown) {
  for (auto& kv : q) {
    auto it = r.find(kv.first);
    if (it == r.end()) {
      if (kv.second.NegOp() || (allow_undefined_wellknown && WellKnown().count(kv.first))) continue;
      return false;
    }
    const SReq m = SReqMerge(it->second, kv.second);
    if (!m.complement && m.values.empty() && !(kv.second.NegOp() && it->second.NegOp())) return false;
  }
  return true;
}
void AddLabel(std::map<string, SReq>& into, const kp_label& l) {
  SReq q;
  q.values.insert(l.value ? l.value : "");
  auto ins = into.emplace(Normalize(l.key), q);
  if (!ins.second) ins.first->second = SReqMerge(q, ins.first->second);
}
// strict(d, i): the node selector, the i-th required term (if any) and the volume requirements
void StrictReqs(const kp_pod_shape& d, uint32_t i, std::map<string, SReq>& out) {
  for (uint32_t j = 0; j < d.n_node_selector; j++) AddLabel(out, d.node_selector[j]);
  if (i < d.n_required_terms) MergeReqs(d.required_terms[i], out);
  MergeReqs(kp_requirements{d.volume_requirements, d.n_volume_requirements, 0}, out);
}
bool ToleratesTaintT(const kp_toleration& t, const TaintT& taint) {  // corev1 Toleration.ToleratesTaint
  if (t.effect != KP_EFFECT_ANY && t.effect != taint.effect) return false;
  if (t.key && *t.key && taint.key != t.key) return false;
  if (t.op == KP_TOL_EQUAL) return taint.value == (t.value ? t.value : "");
  return t.op == KP_TOL_EXISTS;
}
bool ToleratesAllT(const kp_pod_shape& d, const vector<TaintT>& taints, bool skip_pns) {
  for (const TaintT& taint : taints) {
    if (skip_pns && taint.effect == KP_EFFECT_PREFER_NO_SCHEDULE) continue;
    bool ok = false;
    for (uint32_t j = 0; j < d.n_tolerations && !ok; j++) ok = ToleratesTaintT(d.tolerations[j], taint);
    if (!ok) return false;
  }
  return true;
}
int32_t TaintsOf(const kp_taint* t, uint32_t n, const char* who, uint32_t i, vector<TaintT>& out) {
  if (n && !t) return fail(KP_E_INVAL, "%s %u: null taints", who, i);
  for (uint32_t j = 0; j < n; j++) {
    if (!t[j].key) return fail(KP_E_INVAL, "%s %u: null taint key", who, i);
    out.push_back({t[j].key, t[j].value ? t[j].value : "", t[j].effect});
  }
  std::sort(out.begin(), out.end());
  return KP_OK;
}
int32_t CheckLabels(const kp_label* l, uint32_t n, const char* who, uint32_t i) {
  if (n && !l) return fail(KP_E_INVAL, "%s %u: null labels", who, i);
  for (uint32_t j = 0; j < n; j++)
    if (!l[j].key) return fail(KP_E_INVAL, "%s %u: null label key", who, i);
  return KP_OK;
}
int32_t SchedInValidate(const kp_sched_state* st, const kp_sched_out* out) {
  if (!st || !out) return fail(KP_E_INVAL, "null state or out");
  if ((st->n_nodepools && !st->nodepools) || (st->n_daemonsets && !st->daemonsets) || (st->n_nodes && !st->nodes) ||
      (st->n_pods && !st->pods) || (st->n_request_rows && !st->request_rows) || (st->n_nodes && !st->pod_offsets))
    return fail(KP_E_INVAL, "null nodepools, daemonsets, nodes, pod_offsets, pods or request_rows");
  if ((st->n_nodes && !out->nodes) || (st->n_nodepools && !out->pools)) return fail(KP_E_INVAL, "null out->nodes or out->pools");
  if (st->n_nodepools >= 0xFFFF) return fail(KP_E_UNSUPPORTED, "%u NodePools (max 65534)", st->n_nodepools);
  if (st->n_request_rows >= (1u << 31)) return fail(KP_E_UNSUPPORTED, "%u request rows (max 2^31 - 1)", st->n_request_rows);
  if (st->n_nodes) {
    if (st->pod_offsets[0] != 0) return fail(KP_E_INVAL, "pod_offsets[0] = %u", st->pod_offsets[0]);
    for (uint32_t i = 0; i < st->n_nodes; i++)
      if (st->pod_offsets[i + 1] < st->pod_offsets[i]) return fail(KP_E_INVAL, "pod_offsets decrease at node %u", i);
    if (st->pod_offsets[st->n_nodes] != st->n_pods)
      return fail(KP_E_INVAL, "pod_offsets end at %u, n_pods = %u", st->pod_offsets[st->n_nodes], st->n_pods);
  } else if (st->n_pods) {
    return fail(KP_E_INVAL, "%u pods and no node", st->n_pods);
  }
  for (uint32_t i = 0; i < st->n_pods; i++)
    if (st->pods[i].requests >= st->n_request_rows)
      return fail(KP_E_INVAL, "pod %u: request row %u of %u", i, st->pods[i].requests, st->n_request_rows);
  for (uint32_t p = 0; p < st->n_nodepools; p++) {
    const kp_nodepool& np = st->nodepools[p];
    if (!np.name) return fail(KP_E_INVAL, "NodePool %u: null name", p);
    if (int32_t rc = CheckReqs(np.requirements, "NodePool", p, 0)) return rc;
    if (int32_t rc = CheckLabels(np.labels, np.n_labels, "NodePool", p)) return rc;
  }
  for (uint32_t d = 0; d < st->n_daemonsets; d++) {
    const kp_pod_shape& sh = st->daemonsets[d];
    if (int32_t rc = CheckLabels(sh.node_selector, sh.n_node_selector, "daemonset", d)) return rc;
    if ((sh.n_required_terms && !sh.required_terms) || (sh.n_tolerations && !sh.tolerations) ||
        (sh.n_volume_requirements && !sh.volume_requirements))
      return fail(KP_E_INVAL, "daemonset %u: null required terms, tolerations or volume requirements", d);
    for (uint32_t j = 0; j < sh.n_required_terms; j++)
      if (int32_t rc = CheckReqs(sh.required_terms[j], "daemonset", d, j)) return rc;
    if (int32_t rc = CheckReqs(kp_requirements{sh.volume_requirements, sh.n_volume_requirements, 0}, "daemonset volumes", d, 0))
      return rc;
    for (uint32_t j = 0; j < sh.n_tolerations; j++)
      if (sh.tolerations[j].op != KP_TOL_EQUAL && sh.tolerations[j].op != KP_TOL_EXISTS)
        return fail(KP_E_INVAL, "daemonset %u: toleration operator %d", d, sh.tolerations[j].op);
  }
  for (uint32_t i = 0; i < st->n_nodes; i++)
    if (int32_t rc = CheckLabels(st->nodes[i].labels, st->nodes[i].n_labels, "node", i)) return rc;
  return KP_OK;
}
}  // namespace

extern "C" {

int32_t kp_scheduler_inputs(kp_ctx* ctx, const kp_sched_state* st, kp_sched_out* out, kp_solve_stats* stats) {
  if (int32_t rc = SchedInValidate(st, out)) return rc;
  const uint32_t N = st->n_nodes, D = st->n_daemonsets, P = st->n_nodepools, R = st->n_request_rows;
  vector<vector<TaintT>> pool_taints(P), node_taints(N);
  for (uint32_t p = 0; p < P; p++)
    if (int32_t rc = TaintsOf(st->nodepools[p].taints, st->nodepools[p].n_taints, "NodePool", p, pool_taints[p])) return rc;
  for (uint32_t i = 0; i < N; i++)
    if (int32_t rc = TaintsOf(st->nodes[i].taints, st->nodes[i].n_taints, "node", i, node_taints[i])) return rc;
  if (!ctx) return KP_OK;  // host-only validation
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  if (stats) memset(stats, 0, sizeof *stats);
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t W = std::max<uint32_t>(1, (D + 63) / 64);
  // the templates' strict requirements, their keys, the nodes' values under those keys
  vector<std::map<string, SReq>> strict(D);
  std::unordered_map<string, uint32_t> key_id;
  for (uint32_t d = 0; d < D; d++) {
    StrictReqs(st->daemonsets[d], 0, strict[d]);
    for (auto& kv : strict[d]) key_id.emplace(kv.first, (uint32_t)key_id.size());
  }
  const uint32_t K = (uint32_t)key_id.size();
  vector<std::unordered_map<string, uint32_t>> val_id(K);
  vector<vector<string>> vals(K);
  vector<uint32_t> node_val((size_t)K * N, SI_NONE), node_pool(N, SI_NONE), node_tset(std::max<uint32_t>(N, 1), 0);
  vector<uint8_t> clash(K, 0);
  std::unordered_map<string, uint32_t> pool_by_name;
  for (uint32_t p = 0; p < P; p++) pool_by_name.emplace(st->nodepools[p].name, p);
  std::map<vector<TaintT>, uint32_t> tset_id;
  vector<const vector<TaintT>*> tsets;
  for (uint32_t i = 0; i < N; i++) {
    const kp_sched_node& n = st->nodes[i];
    std::fill(clash.begin(), clash.end(), 0);
    for (uint32_t j = 0; j < n.n_labels; j++) {
      const string key = Normalize(n.labels[j].key), v = n.labels[j].value ? n.labels[j].value : "";
      if (key == kNodePool) {
        auto f = pool_by_name.find(v);
        node_pool[i] = f == pool_by_name.end() ? SI_NONE : f->second;
      }
      auto f = key_id.find(key);
      if (f == key_id.end()) continue;
      const uint32_t k = f->second;
      auto ins = val_id[k].emplace(v, (uint32_t)val_id[k].size());
      if (ins.second) vals[k].push_back(v);
      // two labels that normalize to one key with different values leave DoesNotExist: as a missing label
      uint32_t& slot = node_val[(size_t)k * N + i];
      if (clash[k] || (slot != SI_NONE && slot != ins.first->second)) clash[k] = 1, slot = SI_NONE;
      else slot = ins.first->second;
    }
    auto ins = tset_id.emplace(node_taints[i], (uint32_t)tset_id.size());
    if (ins.second) tsets.push_back(&ins.first->first);
    node_tset[i] = ins.first->second;
  }
  // one bitset per (template, key) over the key's dictionary
  vector<uint32_t> tk_off(D + 1, 0), tk_key, tk_bits;
  vector<uint64_t> pass_bits;
  for (uint32_t d = 0; d < D; d++) {
    for (auto& kv : strict[d]) {
      const uint32_t k = key_id[kv.first];
      if (pass_bits.size() >= 0xFFFFFFFFull) return fail(KP_E_UNSUPPORTED, "the daemonsets' requirement bitsets are too large");
      tk_key.push_back(k | (kv.second.NegOp() ? SI_ABSENT_PASSES : 0));
      tk_bits.push_back((uint32_t)pass_bits.size());
      const size_t base = pass_bits.size();
      pass_bits.resize(base + std::max<size_t>(1, (vals[k].size() + 63) / 64), 0);
      for (size_t v = 0; v < vals[k].size(); v++)
        if (kv.second.Admits(vals[k][v])) pass_bits[base + (v >> 6)] |= 1ull << (v & 63);
    }
    tk_off[d + 1] = (uint32_t)tk_key.size();
  }
  // distinct taint set x template
  const uint32_t S = std::max<uint32_t>(1, (uint32_t)tsets.size());
  vector<uint64_t> tol_bits((size_t)S * W, 0);
  for (uint32_t s = 0; s < tsets.size(); s++)
    for (uint32_t d = 0; d < D; d++)
      if (ToleratesAllT(st->daemonsets[d], *tsets[s], false)) tol_bits[(size_t)s * W + (d >> 6)] |= 1ull << (d & 63);
  // the template side: P x D with the relax loop
  vector<uint64_t> pool_compat((size_t)std::max<uint32_t>(P, 1) * W, 0);
  for (uint32_t p = 0; p < P; p++) {
    const kp_nodepool& np = st->nodepools[p];
    std::map<string, SReq> tmpl;
    MergeReqs(np.requirements, tmpl);
    for (uint32_t j = 0; j < np.n_labels; j++) AddLabel(tmpl, np.labels[j]);
    AddLabel(tmpl, kp_label{kNodePool, np.name});
    for (uint32_t d = 0; d < D; d++) {
      const kp_pod_shape& sh = st->daemonsets[d];
      if (!ToleratesAllT(sh, pool_taints[p], true)) continue;
      bool ok = SCompatible(tmpl, strict[d], true);
      for (uint32_t i = 1; i < sh.n_required_terms && !ok; i++) {
        std::map<string, SReq> q;
        StrictReqs(sh, i, q);
        ok = SCompatible(tmpl, q, true);
      }
      if (ok) pool_compat[(size_t)p * W + (d >> 6)] |= 1ull << (d & 63);
    }
  }
  // the numbers
  vector<kp_resource_list> alloc(std::max<uint32_t>(N, 1)), cap(std::max<uint32_t>(N, 1)), tmpl_req(std::max<uint32_t>(D, 1)),
      limits(std::max<uint32_t>(P, 1));
  for (uint32_t i = 0; i < N; i++) alloc[i] = st->nodes[i].allocatable, cap[i] = st->nodes[i].capacity;
  for (uint32_t d = 0; d < D; d++) tmpl_req[d] = st->daemonsets[d].requests;
  for (uint32_t p = 0; p < P; p++) limits[p] = st->nodepools[p].limits;
  vector<uint32_t> pod(std::max<uint32_t>(st->n_pods, 1), 0), pod_off(N + 1, 0);
  for (uint32_t i = 0; i < st->n_pods; i++)
    pod[i] = st->pods[i].requests | ((st->pods[i].flags & KP_SCHED_POD_DAEMON) ? SI_POD_DAEMON : 0);
  for (uint32_t i = 0; i <= N && N; i++) pod_off[i] = st->pod_offsets[i];
  vector<uint32_t> pool_off(P + 1, 0), pool_nodes(std::max<uint32_t>(N, 1), 0);
  for (uint32_t i = 0; i < N; i++)
    if (node_pool[i] != SI_NONE) pool_off[node_pool[i] + 1]++;
  for (uint32_t p = 0; p < P; p++) pool_off[p + 1] += pool_off[p];
  {
    vector<uint32_t> at(pool_off.begin(), pool_off.end() - 1);
    for (uint32_t i = 0; i < N; i++)
      if (node_pool[i] != SI_NONE) pool_nodes[at[node_pool[i]]++] = i;
  }
  Blob blob;
  const size_t o_val = blob.put(node_val), o_tset = blob.put(node_tset), o_alloc = blob.put(alloc), o_cap = blob.put(cap),
               o_poff = blob.put(pod_off), o_pod = blob.put(pod), o_rows = blob.put(st->request_rows, R),
               o_tol = blob.put(tol_bits), o_tkoff = blob.put(tk_off), o_tkkey = blob.put(tk_key),
               o_tkbits = blob.put(tk_bits), o_pass = blob.put(pass_bits), o_tmpl = blob.put(tmpl_req),
               o_pooloff = blob.put(pool_off), o_poolnodes = blob.put(pool_nodes), o_pcompat = blob.put(pool_compat),
               o_limits = blob.put(limits);
  const size_t o_compat = blob.reserve_dev(sizeof(uint64_t) * std::max<size_t>((size_t)N * W, 1)),
               o_nout = blob.reserve_dev(sizeof(SiNodeOut) * std::max<uint32_t>(N, 1)),
               o_part = blob.reserve_dev(sizeof(int64_t) * KP_NUM_RESOURCES * SI_POOL_CHUNKS * std::max<uint32_t>(P, 1)),
               o_pout = blob.reserve_dev(sizeof(SiPoolOut) * std::max<uint32_t>(P, 1));
  if (blob.total() > ctx->schedin_bytes) {
    if (ctx->schedin) (void)hipFree(ctx->schedin);
    ctx->schedin = nullptr, ctx->schedin_bytes = 0;
    HIPCHK(hipMalloc(&ctx->schedin, blob.total()));
    ctx->schedin_bytes = blob.total();
  }
  uint8_t* base = (uint8_t*)ctx->schedin;
  SchedInArgs a{};
  a.n_nodes = (int)N, a.n_tmpl = (int)D, a.n_pools = (int)P, a.words = (int)W;
  a.node_val = (const uint32_t*)(base + o_val), a.node_tset = (const uint32_t*)(base + o_tset);
  a.alloc = (const kp_resource_list*)(base + o_alloc), a.cap = (const kp_resource_list*)(base + o_cap);
  a.pod_off = (const uint32_t*)(base + o_poff), a.pod = (const uint32_t*)(base + o_pod);
  a.rows = (const kp_resource_list*)(base + o_rows), a.tol_bits = (const uint64_t*)(base + o_tol);
  a.tk_off = (const uint32_t*)(base + o_tkoff), a.tk_key = (const uint32_t*)(base + o_tkkey);
  a.tk_bits = (const uint32_t*)(base + o_tkbits), a.pass_bits = (const uint64_t*)(base + o_pass);
  a.tmpl = (const kp_resource_list*)(base + o_tmpl), a.pool_off = (const uint32_t*)(base + o_pooloff);
  a.pool_nodes = (const uint32_t*)(base + o_poolnodes), a.pool_compat = (const uint64_t*)(base + o_pcompat);
  a.limits = (const kp_resource_list*)(base + o_limits);
  a.compat = (uint64_t*)(base + o_compat), a.node_out = (SiNodeOut*)(base + o_nout);
  a.part = (int64_t*)(base + o_part), a.pool_out = (SiPoolOut*)(base + o_pout);
  const double compile_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  hipStream_t s = ctx->stream;
  HIPCHK(hipMemcpyAsync(base, blob.host.data(), blob.host.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipEventRecord(ctx->ev0, s));
  HIPCHK(launch_scheduler_inputs(a, s));
  HIPCHK(hipEventRecord(ctx->ev1, s));
  if (N) HIPCHK(hipMemcpyAsync(out->nodes, a.node_out, sizeof(SiNodeOut) * N, hipMemcpyDeviceToHost, s));
  if (P) HIPCHK(hipMemcpyAsync(out->pools, a.pool_out, sizeof(SiPoolOut) * P, hipMemcpyDeviceToHost, s));
  if (N && out->compat) HIPCHK(hipMemcpyAsync(out->compat, a.compat, sizeof(uint64_t) * (size_t)N * W, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (stats) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    stats->device_ms = ms;
    stats->prepare_ms = compile_ms;
    stats->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return KP_OK;
}

}  // extern "C"

// ---- The catalogue compile (kp_catalog_compile) ---------------------------------------------------------------------
// The host does strings only: a type's architecture and GPU manufacturer become flags, zone names indices into
// all_zones, the unavailable offerings one bit row over the types per (capacity type, zone) plus the two wide masks,
// and every NodeClass one fixed-width record (CcNodeClass). Every number of the result is the device's
// (kp_catcomp.hip); kp_instance_type_resolve and kp_instance_type_overhead above are what the tests hold it to.
static_assert(sizeof(kp_reserved_offering) == 16, "the reserved record is written by the device as it stands");

namespace {
int CapacityTypeIndex(const char* ct) {
  if (ct && strcmp(ct, "on-demand") == 0) return KP_CT_ON_DEMAND;
  if (ct && strcmp(ct, "spot") == 0) return KP_CT_SPOT;
  return -1;
}
// Validation and the zone dictionary (zone name -> index into all_zones)
int32_t CatCompValidate(const kp_compile_in* in, const kp_compile_out* out, std::unordered_map<string, uint32_t>& zone_id) {
  if (!in || !out) return fail(KP_E_INVAL, "null in or out");
  if (!out->capacity && !out->overhead && !out->kube_reserved && !out->system_reserved && !out->eviction_threshold &&
      !out->it_zones && !out->price && !out->available && !out->reserved)
    return fail(KP_E_INVAL, "every output is NULL");
  const uint32_t T = in->n_types, N = in->n_nodeclasses, Z = in->n_all_zones;
  // the caps first: nothing is read before them
  if (Z > 64) return fail(KP_E_UNSUPPORTED, "%u zones (max 64)", Z);
  if ((uint64_t)N * T >= (1ull << 31)) return fail(KP_E_UNSUPPORTED, "%u NodeClasses x %u types (max 2^31 - 1 pairs)", N, T);
  if ((uint64_t)T * Z * 2 >= (1ull << 31)) return fail(KP_E_UNSUPPORTED, "%u types x %u zones (max 2^30 - 1 prices)", T, Z);
  if (N > 65535) return fail(KP_E_UNSUPPORTED, "%u NodeClasses (max 65535)", N);
  if ((T && !in->types) || (N && !in->nodeclasses) || (Z && !in->all_zones) || (T && !in->type_zones) ||
      (T && !in->od_price) || (T && Z && !in->spot_price) || (in->n_unavailable && !in->unavailable) ||
      (in->n_reservations && (!in->reservations || !in->reservation_offsets)))
    return fail(KP_E_INVAL, "null types, nodeclasses, all_zones, type_zones, od_price, spot_price, unavailable, "
                            "reservations or reservation_offsets");
  for (uint32_t z = 0; z < Z; z++) {
    if (!in->all_zones[z]) return fail(KP_E_INVAL, "all_zones[%u] is NULL", z);
    if (!zone_id.emplace(in->all_zones[z], z).second) return fail(KP_E_INVAL, "all_zones[%u] (%s) repeats", z, in->all_zones[z]);
  }
  const uint64_t zone_bits = Z == 64 ? ~0ull : (1ull << Z) - 1;
  for (uint32_t t = 0; t < T; t++) {
    if (in->type_zones[t] & ~zone_bits) return fail(KP_E_INVAL, "type %u: type_zones names a zone past n_all_zones = %u", t, Z);
    if (in->od_price[t] < 0) return fail(KP_E_INVAL, "type %u: on-demand price %g (a price is a number >= 0)", t, in->od_price[t]);
    for (uint32_t z = 0; z < Z; z++)
      if (in->spot_price[(size_t)t * Z + z] < 0)
        return fail(KP_E_INVAL, "type %u, zone %u: spot price %g (a price is a number >= 0)", t, z, in->spot_price[(size_t)t * Z + z]);
  }
  for (uint32_t n = 0; n < N; n++) {
    const kp_nodeclass& nc = in->nodeclasses[n];
    if (nc.n_zones && !nc.zones) return fail(KP_E_INVAL, "NodeClass %u: null zones", n);
    for (uint32_t j = 0; j < nc.n_zones; j++)
      if (!nc.zones[j]) return fail(KP_E_INVAL, "NodeClass %u: zone %u is NULL", n, j);
    if (nc.n_block_device_mappings && !nc.block_device_mappings) return fail(KP_E_INVAL, "NodeClass %u: null block_device_mappings", n);
  }
  if (in->discovered_memory)  // bytes become milli-units on the device
    for (size_t i = 0; i < (size_t)N * T; i++)
      if (in->discovered_memory[i] > std::numeric_limits<int64_t>::max() / 1000)
        return fail(KP_E_INVAL, "discovered_memory[%zu] = %lld bytes does not fit milli-units", i, (long long)in->discovered_memory[i]);
  for (uint32_t i = 0; i < in->n_unavailable; i++) {
    const kp_unavailable& u = in->unavailable[i];
    const bool triple = u.capacity_type && u.zone && u.type >= 0, ct_alone = u.capacity_type && !u.zone && u.type < 0,
               zone_alone = !u.capacity_type && u.zone && u.type < 0;
    if (!triple && !ct_alone && !zone_alone)
      return fail(KP_E_INVAL, "unavailable %u: not a (capacity type, type, zone) triple, a capacity type alone or a zone alone", i);
    if (u.capacity_type && CapacityTypeIndex(u.capacity_type) < 0)
      return fail(KP_E_INVAL, "unavailable %u: unknown capacity type %s", i, u.capacity_type);
    if (u.zone && !zone_id.count(u.zone)) return fail(KP_E_INVAL, "unavailable %u: zone %s is not in all_zones", i, u.zone);
    if (triple && (uint32_t)u.type >= T) return fail(KP_E_INVAL, "unavailable %u: type %d of %u", i, u.type, T);
  }
  if (in->n_reservations) {
    const uint32_t* off = in->reservation_offsets;
    if (off[0] != 0) return fail(KP_E_INVAL, "reservation_offsets[0] = %u", off[0]);
    for (uint32_t n = 0; n < N; n++)
      if (off[n + 1] < off[n]) return fail(KP_E_INVAL, "reservation_offsets decrease at NodeClass %u", n);
    if (off[N] != in->n_reservations)
      return fail(KP_E_INVAL, "reservation_offsets end at %u, n_reservations = %u", off[N], in->n_reservations);
    for (uint32_t r = 0; r < in->n_reservations; r++) {
      const kp_compile_reservation& cr = in->reservations[r];
      if (!cr.id) return fail(KP_E_INVAL, "reservation %u: null id", r);
      if (cr.type >= T) return fail(KP_E_INVAL, "reservation %u (%s): type %u of %u", r, cr.id, cr.type, T);
      if (!cr.zone || !zone_id.count(cr.zone))
        return fail(KP_E_INVAL, "reservation %u (%s): zone %s is not in all_zones", r, cr.id, cr.zone ? cr.zone : "(null)");
    }
  }
  return KP_OK;
}
}  // namespace

extern "C" {

int32_t kp_catalog_compile(kp_ctx* ctx, const kp_compile_in* in, const kp_compile_out* out, kp_solve_stats* stats) {
  std::unordered_map<string, uint32_t> zone_id;
  if (int32_t rc = CatCompValidate(in, out, zone_id)) return rc;
  if (!ctx) return KP_OK;  // host-only validation
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  HIPCHK(hipSetDevice(ctx->device));
  if (stats) memset(stats, 0, sizeof *stats);
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t T = in->n_types, N = in->n_nodeclasses, Z = in->n_all_zones;
  const uint32_t R = in->reserved_capacity ? in->n_reservations : 0;  // the ReservedCapacity feature gate
  const uint32_t W = std::max<uint32_t>(1, (T + 63) / 64);
  // the types as a structure of arrays
  const size_t T1 = std::max<uint32_t>(T, 1);
  vector<int32_t> vcpu(T1), gpu_count(T1), neuron_devices(T1), neuron_cores(T1), efa(T1), max_enis(T1), ipv4(T1), branch(T1);
  vector<int64_t> memory_mib(T1), storage_gb(T1);
  vector<uint32_t> type_flags(T1, 0);
  for (uint32_t t = 0; t < T; t++) {
    const kp_ec2_info& e = in->types[t];
    vcpu[t] = e.vcpu, memory_mib[t] = e.memory_mib, gpu_count[t] = e.gpu_count, neuron_devices[t] = e.neuron_devices;
    neuron_cores[t] = e.neuron_cores_per_device, efa[t] = e.efa, max_enis[t] = e.max_enis, ipv4[t] = e.ipv4_per_eni;
    branch[t] = e.branch_enis;
    storage_gb[t] = e.instance_storage_gb > 0 ? e.instance_storage_gb : e.local_nvme_gb;
    const char* gm = e.gpu_manufacturer ? e.gpu_manufacturer : "";
    const uint32_t gpu = strcmp(gm, "nvidia") == 0 ? CC_GPU_NVIDIA : strcmp(gm, "amd") == 0 ? CC_GPU_AMD
                         : strcmp(gm, "habana") == 0 ? CC_GPU_HABANA : CC_GPU_NONE;
    type_flags[t] = (e.arch && strcmp(e.arch, "arm64") == 0 ? CC_T_ARM64 : 0) | (e.arch && strcmp(e.arch, "amd64") == 0 ? CC_T_AMD64 : 0) |
                    (e.in_limits_table ? CC_T_IN_LIMITS : 0) | (e.trunking ? CC_T_TRUNKING : 0) | (gpu << CC_T_GPU_SHIFT);
  }
  // every NodeClass as one record
  vector<CcNodeClass> ncs(std::max<uint32_t>(N, 1));
  memset(ncs.data(), 0, ncs.size() * sizeof(CcNodeClass));
  const kp_ec2_info no_store{};
  for (uint32_t n = 0; n < N; n++) {
    const kp_nodeclass& nc = in->nodeclasses[n];
    CcNodeClass& c = ncs[n];
    const FamilyFlags fam = Family(&nc);
    c.flags = (fam.eni_memory ? CC_N_ENI_MEMORY : 0) | (fam.pods_per_core ? CC_N_PODS_PER_CORE : 0) |
              (fam.eni_density ? CC_N_ENI_DENSITY : 0) | (fam.windows ? CC_N_WINDOWS : 0) |
              (nc.instance_store_policy == KP_INSTANCE_STORE_RAID0 ? CC_N_RAID0 : 0);
    if (const kp_kubelet* kl = nc.kubelet) {
      c.flags |= CC_N_KUBELET | (kl->has_eviction_hard ? CC_N_EVICTION_HARD : 0) |
                 (kl->has_eviction_soft && fam.eviction_soft ? CC_N_EVICTION_SOFT : 0);
      c.kube_reserved = kl->kube_reserved, c.system_reserved = kl->system_reserved;
      c.hard_memory = kl->hard_memory_available, c.hard_nodefs = kl->hard_nodefs_available;
      c.soft_memory = kl->soft_memory_available, c.soft_nodefs = kl->soft_nodefs_available;
    }
    kp_nodeclass no_raid = nc;  // what EphemeralBytes returns without RAID0: the type plays no part in it
    no_raid.instance_store_policy = KP_INSTANCE_STORE_NONE;
    c.storage_bytes = EphemeralBytes(&no_store, &no_raid);
    c.max_pods = nc.max_pods, c.pods_per_core = nc.pods_per_core;
    for (uint32_t j = 0; j < nc.n_zones; j++) {
      auto f = zone_id.find(nc.zones[j]);
      if (f != zone_id.end()) c.zone_mask |= 1ull << f->second;
    }
  }
  // the unavailable offerings
  vector<uint64_t> ice_rows((size_t)2 * std::max<uint32_t>(Z, 1) * W, 0);
  uint64_t ice_zones = 0;
  uint32_t ice_cts = 0;
  for (uint32_t i = 0; i < in->n_unavailable; i++) {
    const kp_unavailable& u = in->unavailable[i];
    if (u.capacity_type && u.zone)
      ice_rows[((size_t)CapacityTypeIndex(u.capacity_type) * Z + zone_id[u.zone]) * W + ((uint32_t)u.type >> 6)] |= 1ull << (u.type & 63);
    else if (u.capacity_type)
      ice_cts |= 1u << CapacityTypeIndex(u.capacity_type);
    else
      ice_zones |= 1ull << zone_id[u.zone];
  }
  vector<CcReservation> res(std::max<uint32_t>(R, 1));
  for (uint32_t n = 0; n < N && R; n++)
    for (uint32_t r = in->reservation_offsets[n]; r < in->reservation_offsets[n + 1]; r++)
      res[r] = CcReservation{n, in->reservations[r].type, zone_id[in->reservations[r].zone], in->reservations[r].available_count};
  const size_t pairs = (size_t)N * T, P1 = std::max<size_t>(pairs, 1);
  Blob blob;
  const size_t o_vcpu = blob.put(vcpu), o_mem = blob.put(memory_mib), o_tf = blob.put(type_flags), o_gpu = blob.put(gpu_count),
               o_nd = blob.put(neuron_devices), o_ncore = blob.put(neuron_cores), o_efa = blob.put(efa), o_enis = blob.put(max_enis),
               o_ipv4 = blob.put(ipv4), o_branch = blob.put(branch), o_sgb = blob.put(storage_gb),
               o_tz = blob.put(in->type_zones, T), o_od = blob.put(in->od_price, T), o_spot = blob.put(in->spot_price, (size_t)T * Z),
               o_ncs = blob.put(ncs), o_ice = blob.put(ice_rows), o_res = blob.put(res),
               o_disc = in->discovered_memory ? blob.put(in->discovered_memory, pairs) : 0;
  const size_t o_lists = blob.reserve_dev(sizeof(kp_resource_list) * P1 * 5), o_itz = blob.reserve_dev(sizeof(uint64_t) * P1),
               o_avail = blob.reserve_dev(sizeof(uint64_t) * P1 * 2),
               o_price = blob.reserve_dev(sizeof(double) * std::max<size_t>((size_t)T * Z * 2, 1)),
               o_rout = blob.reserve_dev(sizeof(kp_reserved_offering) * std::max<uint32_t>(R, 1));
  if (blob.total() > ctx->catcomp_bytes) {
    if (ctx->catcomp) (void)hipFree(ctx->catcomp);
    ctx->catcomp = nullptr, ctx->catcomp_bytes = 0;
    HIPCHK(hipMalloc(&ctx->catcomp, blob.total()));
    ctx->catcomp_bytes = blob.total();
  }
  uint8_t* base = (uint8_t*)ctx->catcomp;
  CatCompArgs a{};
  a.n_types = (int)T, a.n_nodeclasses = (int)N, a.n_zones = (int)Z, a.n_reservations = (int)R, a.words = (int)W;
  a.vm_memory_overhead_percent = in->opts.vm_memory_overhead_percent, a.reserved_enis = in->opts.reserved_enis;
  a.vcpu = (const int32_t*)(base + o_vcpu), a.memory_mib = (const int64_t*)(base + o_mem);
  a.type_flags = (const uint32_t*)(base + o_tf), a.gpu_count = (const int32_t*)(base + o_gpu);
  a.neuron_devices = (const int32_t*)(base + o_nd), a.neuron_cores = (const int32_t*)(base + o_ncore);
  a.efa = (const int32_t*)(base + o_efa), a.max_enis = (const int32_t*)(base + o_enis);
  a.ipv4_per_eni = (const int32_t*)(base + o_ipv4), a.branch_enis = (const int32_t*)(base + o_branch);
  a.storage_gb = (const int64_t*)(base + o_sgb), a.type_zones = (const uint64_t*)(base + o_tz);
  a.od_price = (const double*)(base + o_od), a.spot_price = (const double*)(base + o_spot);
  a.nodeclasses = (const CcNodeClass*)(base + o_ncs);
  a.discovered = in->discovered_memory ? (const int64_t*)(base + o_disc) : nullptr;
  a.ice_rows = (const uint64_t*)(base + o_ice), a.ice_zones = ice_zones, a.ice_capacity_types = ice_cts;
  a.reservations = (const CcReservation*)(base + o_res);
  kp_resource_list* lists = (kp_resource_list*)(base + o_lists);
  a.capacity = lists, a.overhead = lists + P1, a.kube_reserved = lists + 2 * P1, a.system_reserved = lists + 3 * P1;
  a.eviction_threshold = lists + 4 * P1;
  a.it_zones = (uint64_t*)(base + o_itz), a.available = (uint64_t*)(base + o_avail), a.price = (double*)(base + o_price);
  a.reserved = (kp_reserved_offering*)(base + o_rout);
  const double compile_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  hipStream_t s = ctx->stream;
  HIPCHK(hipMemcpyAsync(base, blob.host.data(), blob.host.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipEventRecord(ctx->ev0, s));
  HIPCHK(launch_catalog_compile(a, s));
  HIPCHK(hipEventRecord(ctx->ev1, s));
  const struct {
    void* dst;
    const void* src;
    size_t bytes;
  } back[] = {{out->capacity, a.capacity, sizeof(kp_resource_list) * pairs},
              {out->overhead, a.overhead, sizeof(kp_resource_list) * pairs},
              {out->kube_reserved, a.kube_reserved, sizeof(kp_resource_list) * pairs},
              {out->system_reserved, a.system_reserved, sizeof(kp_resource_list) * pairs},
              {out->eviction_threshold, a.eviction_threshold, sizeof(kp_resource_list) * pairs},
              {out->it_zones, a.it_zones, sizeof(uint64_t) * pairs},
              {out->available, a.available, sizeof(uint64_t) * pairs * 2},
              {out->price, a.price, sizeof(double) * (size_t)T * Z * 2},
              {out->reserved, a.reserved, sizeof(kp_reserved_offering) * R}};
  for (auto& b : back)
    if (b.dst && b.bytes) HIPCHK(hipMemcpyAsync(b.dst, b.src, b.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (stats) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    stats->device_ms = ms;
    stats->prepare_ms = compile_ms;
    stats->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return KP_OK;
}

int32_t kp_simulate_batch(kp_ctx* ctx, const kp_cluster* cl, const uint32_t* offsets, const uint32_t* nodes,
                          uint32_t n_subsets, int32_t multi_node, kp_sim_result* out, kp_solve_stats* stats) {
  kp_cluster_plan* plan = nullptr;
  int32_t rc = kp_cluster_prepare(ctx, cl, &plan);
  if (rc) return rc;
  const double prep = plan->prepare_ms;
  rc = kp_cluster_simulate(plan, offsets, nodes, n_subsets, multi_node, out, stats);
  if (stats) stats->prepare_ms = prep;
  kp_cluster_plan_destroy(plan);
  return rc;
}

}  // extern "C"

// ==================================================================================================
// Multi-GPU consolidation: RCCL communicator + the sweep's argmin (kp_consolidate_argmin)
// ==================================================================================================
static_assert(sizeof(kp_choice) == sizeof(CommBest), "kp_choice mirrors CommBest (the all-gathered record)");


namespace {
int32_t nccl_fail(ncclResult_t r, const char* what) {
  return fail(KP_E_DEVICE, "%s: %s", what, ncclGetErrorString(r));
}
// (savings desc, global index asc) over the records holding a decision (index >= 0)
bool Better(const kp_choice& x, const kp_choice& best) {
  if (x.subset < 0) return false;
  if (best.subset < 0) return true;
  if (x.result.savings != best.result.savings) return x.result.savings > best.result.savings;
  return x.subset < best.subset;
}
}  // namespace

extern "C" {

int32_t kp_choice_reduce(const kp_choice* per_rank, uint32_t n, kp_choice* out) {
  if (!out || (!per_rank && n)) return fail(KP_E_INVAL, "null argument");
  kp_choice best;
  memset(&best, 0, sizeof best);
  best.subset = -1;
  uint64_t counts[3] = {0, 0, 0}, overflowed = 0;
  for (uint32_t i = 0; i < n; i++)
    if (per_rank[i].subset == KP_CHOICE_FAILED)
      return fail(KP_E_DEVICE, "rank %u failed its step of the sweep (error %lld)", i, (long long)per_rank[i].counts[0]);
  for (uint32_t i = 0; i < n; i++) {
    for (int k = 0; k < 3; k++) counts[k] += per_rank[i].counts[k];
    overflowed += per_rank[i].overflowed;
    if (Better(per_rank[i], best)) best = per_rank[i];
  }
  for (int k = 0; k < 3; k++) best.counts[k] = counts[k];
  best.overflowed = overflowed;
  if (best.subset < 0) memset(&best.result, 0, sizeof best.result);
  *out = best;
  return KP_OK;
}

int32_t kp_comm_unique_id(uint8_t* id) {
  if (!id) return fail(KP_E_INVAL, "null argument");
  ncclUniqueId u;
  ncclResult_t r = ncclGetUniqueId(&u);
  if (r != ncclSuccess) return nccl_fail(r, "ncclGetUniqueId");
  static_assert(sizeof(u) == KP_COMM_ID_BYTES, "ncclUniqueId size");
  memcpy(id, &u, sizeof u);
  return KP_OK;
}

int32_t kp_comm_init(kp_ctx* ctx, const uint8_t* id, int32_t n_ranks, int32_t rank, kp_comm** out) {
  if (!ctx || !id || !out) return fail(KP_E_INVAL, "null argument");
  if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(KP_E_INVAL, "rank %d of %d", rank, n_ranks);
  HIPCHK(hipSetDevice(ctx->device));
  auto c = std::make_unique<kp_comm>();
  c->ctx = ctx;
  c->n_ranks = n_ranks;
  c->rank = rank;
  ncclUniqueId u;
  memcpy(&u, id, sizeof u);
  ncclResult_t r = ncclCommInitRank(&c->comm, n_ranks, u, rank);
  if (r != ncclSuccess) return nccl_fail(r, "ncclCommInitRank");
  HIPCHK(c->buf.alloc(sizeof(CommBest) * (size_t)(n_ranks + 1)));
  CommReadSettings(c.get());
  *out = c.release();
  return KP_OK;
}

int32_t kp_comm_init_all(kp_ctx* const* ctxs, int32_t n, kp_comm** out) {
  if (!ctxs || !out || n < 1) return fail(KP_E_INVAL, "null argument");
  vector<int> devs(n);
  for (int i = 0; i < n; i++) {
    if (!ctxs[i]) return fail(KP_E_INVAL, "null context %d", i);
    devs[i] = ctxs[i]->device;
    for (int j = 0; j < i; j++)
      if (devs[j] == devs[i]) return fail(KP_E_INVAL, "contexts %d and %d share GPU %d (RCCL: one rank per GPU)", j, i, devs[i]);
  }
  vector<ncclComm_t> comms(n, nullptr);
  ncclResult_t r = ncclCommInitAll(comms.data(), n, devs.data());
  if (r != ncclSuccess) return nccl_fail(r, "ncclCommInitAll");
  vector<std::unique_ptr<kp_comm>> cs(n);
  for (int i = 0; i < n; i++) {
    cs[i] = std::make_unique<kp_comm>();
    cs[i]->ctx = ctxs[i];
    cs[i]->comm = comms[i];
    cs[i]->n_ranks = n;
    cs[i]->rank = i;
    CommReadSettings(cs[i].get());
  }
  for (int i = 0; i < n; i++) {
    if (hipSetDevice(devs[i]) != hipSuccess || cs[i]->buf.alloc(sizeof(CommBest) * (size_t)(n + 1)) != hipSuccess) {
      for (int j = 0; j < n; j++) (void)ncclCommDestroy(comms[j]);
      return fail(KP_E_NOMEM, "communicator buffer on GPU %d", devs[i]);
    }
  }
  for (int i = 0; i < n; i++) out[i] = cs[i].release();
  return KP_OK;
}

int32_t kp_comm_init_host(kp_ctx* ctx, int32_t n_ranks, int32_t rank, kp_allgather_fn fn, void* user, kp_comm** out) {
  if (!ctx || !fn || !out) return fail(KP_E_INVAL, "null argument");
  if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(KP_E_INVAL, "rank %d of %d", rank, n_ranks);
  auto c = std::make_unique<kp_comm>();
  c->ctx = ctx;
  c->host_fn = fn;
  c->host_user = user;
  c->n_ranks = n_ranks;
  c->rank = rank;
  CommReadSettings(c.get());
  *out = c.release();
  return KP_OK;
}

int32_t kp_comm_rank(const kp_comm* c, int32_t* rank, int32_t* n_ranks) {
  if (!c) return fail(KP_E_INVAL, "null argument");
  if (rank) *rank = c->rank;
  if (n_ranks) *n_ranks = c->n_ranks;
  return KP_OK;
}

void kp_comm_destroy(kp_comm* c) {
  if (!c) return;
  (void)hipSetDevice(c->ctx->device);
  if (c->comm) (void)ncclCommDestroy(c->comm);
  delete c;
}

int32_t kp_consolidate_argmin(kp_cluster_plan* plan, kp_comm* comm, const uint32_t* offsets, const uint32_t* nodes,
                              uint32_t n_subsets, uint64_t base_index, int32_t multi_node, kp_sim_result* out,
                              kp_choice* best, kp_solve_stats* stats) {
  return kp_consolidate_argmin_cancellable(plan, comm, nullptr, offsets, nodes, n_subsets, base_index, multi_node, out,
                                           best, stats);
}

static int32_t ArgminImpl(kp_cluster_plan* plan, kp_comm* comm, kp_cancel* cancel, const uint32_t* offsets,
                          const uint32_t* nodes, uint32_t n_subsets, uint64_t base_index, int32_t multi_node,
                          kp_sim_result* out, kp_choice* best, kp_solve_stats* stats, BudgetGate* bg);

int32_t kp_consolidate_argmin_cancellable(kp_cluster_plan* plan, kp_comm* comm, kp_cancel* cancel,
                                          const uint32_t* offsets, const uint32_t* nodes, uint32_t n_subsets,
                                          uint64_t base_index, int32_t multi_node, kp_sim_result* out, kp_choice* best,
                                          kp_solve_stats* stats) {
  return ArgminImpl(plan, comm, cancel, offsets, nodes, n_subsets, base_index, multi_node, out, best, stats, nullptr);
}

int32_t kp_consolidate_argmin_budgeted(kp_cluster_plan* plan, kp_comm* comm, kp_cancel* cancel, const uint32_t* offsets,
                                       const uint32_t* nodes, uint32_t n_subsets, uint64_t base_index, int32_t multi_node,
                                       const uint32_t* allowed, uint32_t n_allowed, kp_sim_result* out, kp_choice* best,
                                       uint64_t* n_blocked, kp_solve_stats* stats) {
  if (n_blocked) *n_blocked = 0;
  if (!allowed)
    return ArgminImpl(plan, comm, cancel, offsets, nodes, n_subsets, base_index, multi_node, out, best, stats, nullptr);
  BudgetGate bg{allowed, n_allowed};
  const int32_t rc = ArgminImpl(plan, comm, cancel, offsets, nodes, n_subsets, base_index, multi_node, out, best, stats, &bg);
  if (!rc && n_blocked) *n_blocked = bg.blocked;
  return rc;
}

// bg: the budget gate (a failure of it is a failure of the local step: a KP_CHOICE_FAILED record, no peer left waiting)
static int32_t ArgminImpl(kp_cluster_plan* plan, kp_comm* comm, kp_cancel* cancel, const uint32_t* offsets,
                          const uint32_t* nodes, uint32_t n_subsets, uint64_t base_index, int32_t multi_node,
                          kp_sim_result* out, kp_choice* best, kp_solve_stats* stats, BudgetGate* bg) {
  auto t0 = std::chrono::steady_clock::now();
  if (!plan || !best || (n_subsets && !offsets)) return fail(KP_E_INVAL, "null argument");
  if (cancel && cancel->ctx.p != plan->ctx.p) return fail(KP_E_INVAL, "the cancel token belongs to another context");
  if (comm && comm->ctx->device != plan->ctx->device) return fail(KP_E_INVAL, "comm and plan are on different GPUs");
  kp_ctx* ctx = plan->ctx;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  if (stats) memset(stats, 0, sizeof *stats);
  hipStream_t st = ctx->stream;
  float ms = 0;
  uint64_t kst[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  CommBest mine;  // this rank's record (host)
  memset(&mine, 0, sizeof mine);
  DevBuf rec, parts;
  // the local step: simulation + device argmax into one record; any failure becomes a KP_CHOICE_FAILED record so that
  // the collective below is still reached by every rank
  auto local = [&]() -> int32_t {
    HIPCHK(hipSetDevice(ctx->device));
    SimArgs a;
    memset(&a, 0, sizeof a);
    const int n_parts = (int)std::min<uint32_t>(std::max<uint32_t>((n_subsets + 4095) / 4096, 1), 1024);
    HIPCHK(parts.alloc(sizeof(ArgmaxPart) * n_parts));
    HIPCHK(rec.alloc(sizeof(CommBest)));
    if (bg)
      if (int32_t rc = CheckBudget(plan, bg)) return rc;
    if (n_subsets) {
      int32_t rc = SimLaunchLocked(plan, offsets, nodes, n_subsets, multi_node, a, cancel, bg);
      if (rc) return rc;
      if (out) HIPCHK(hipMemcpyAsync(out, a.out, sizeof(SimOut) * n_subsets, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(kst, a.stats, sizeof kst, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(launch_argmax(n_subsets ? a.out : nullptr, (int)n_subsets, (ArgmaxPart*)parts.p, n_parts,
                         (int64_t)base_index, (CommBest*)rec.p, st));
    HIPCHK(hipMemcpyAsync(&mine, rec.p, sizeof mine, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_subsets && !plan->general && kst[5])
      return fail(KP_E_CANCELED, "consolidation sweep cancelled (kp_cancel_set)");
    if (n_subsets && plan->general) ms = (float)plan->general_ms;
    else if (n_subsets) HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    return KP_OK;
  };
  const int32_t lrc = local();
  if (lrc) {
    memset(&mine, 0, sizeof mine);
    mine.index = KP_CHOICE_FAILED;
    mine.counts[0] = (uint64_t)(int64_t)lrc;
  }
  const int nr = comm ? comm->n_ranks : 1;
  vector<CommBest> recs(nr);
  if (comm && nr > 1) {  // one collective: every rank's 88-byte record to every rank (RCCL over xGMI)
    const string err = g_err;
    int32_t rc = CommExchange(comm, &mine, recs.data(), sizeof mine);
    if (rc) return rc;
    g_err = err;
  } else {
    recs[0] = mine;
  }
  if (lrc) return lrc;
  for (int i = 0; i < nr; i++)
    if (recs[i].index != KP_CHOICE_FAILED && recs[i].counts[3])
      return fail(KP_E_DEVICE, "rank %d: %llu subsets overflowed the pod queue", i, (unsigned long long)recs[i].counts[3]);
  vector<kp_choice> ch(nr);
  memcpy(ch.data(), recs.data(), sizeof(kp_choice) * nr);
  int32_t rc = kp_choice_reduce(ch.data(), (uint32_t)nr, best);
  if (rc) return rc;
  if (stats) {
    stats->device_ms = ms;
    stats->solve_kernel_ms = ms;
    stats->attempts = kst[0];
    stats->bytes_algorithmic = kst[1];
    stats->pops = kst[2];
    stats->phase_cycles[0] = kst[3];
    if (plan->general) {  // general path: simulations batched / compiled per subset, batched launches
      stats->phase_cycles[1] = kst[4];
      stats->phase_cycles[2] = kst[6];
      for (int k = 0; k < 8; k++) stats->attempt_cycles[k] = plan->general_phase[k];  // (timing diagnostics)
    } else {  // batched sweep: wave slots launched, most subsets any wave ran
      stats->phase_cycles[1] = plan->sim_waves[0];
      stats->phase_cycles[2] = plan->sim_waves[1];
    }
    stats->prepare_ms = plan->prepare_ms;
    stats->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return KP_OK;
}

}  // extern "C"
