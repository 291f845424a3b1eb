// dvm_slam_amd/csrc/bow_targets.cpp -- dvm_search_by_bow_targets: ORBmatcher::SearchByBoW(KF1, KF2) of one current keyframe against all
// the candidate and covisible keyframes of LoopClosing::DetectCommonRegionsFromBoW as one chain (include/dvmslam_hip.h; kernels in
// bow_targets_kernels.hip; the handle's stream, working set, packing cursor and kernel times: chain.h).  The working set: a device block
// [upload: keyframe table, current keyframe, targets, zeroed counters][results: nmatches, match rows][bins] and a page-locked block
// [upload][results].  A call validates everything, packs the upload, sends it with ONE copy, launches the search and the settle kernels,
// copies the results back with ONE copy and waits ONCE.
// dvm_search_by_bow_targets_resident names every keyframe as a keyframe-store slot plus its map points as map-store slots: the table's
// desc and FeatureVector pointers go into the slots, the upload is [keyframe table][prologue table][mp_slot lists], and k_bt_prologue
// writes the flags, the angles, the -1 rows and the zeroed counters into the device block before the same two kernels run.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/dvmslam_hip.h"
#include "bow_targets_kernels.h"
#include "chain.h"
#include "keyframe_store.h"
#include "map_store.h"
#include "match_kernels.h"
#include "orb_pipeline.h"

using namespace dvm;

struct dvm_bow_targets : Chain {
  // ws.d: [up_bytes][res_bytes][bin_bytes]; ws.hm (page-locked, not mapped): [up_bytes][res_bytes]
  size_t up_bytes = 0, res_bytes = 0, bin_bytes = 0;
  int max_cur = 0, max_targets = 0, max_total = 0;
  std::vector<uint8_t> seen, listed;            // [kFrameCap] each: the duplicate check of one keyframe; the current keyframe's listed features
  float last_ms[3] = {0, 0, 0};                 // search, settle, the resident call's prologue
  int64_t last_up = 0;                          // dvm_bow_targets_last_upload_bytes
  std::vector<KfSlotView> views;                // the resident call's keyframes: [0] the current one, [1 + t] target t
  std::vector<const dvm_map_store*> stores;     // the distinct map stores it names
};

namespace {
using Cursor64 = Cursor<64>;                    // every item of the upload and the results starts at a multiple of 64 bytes
constexpr int kMaxTargets = 65535;
constexpr int64_t kMaxEntries = (int64_t)1 << 27;   // target x current-keypoint entries of one call
// upload bytes of a keyframe of n keypoints whose FeatureVector has at most n nodes: angle, descriptor, use flag; node, offset, feature;
// the last offset and the rounding of its six arrays
constexpr size_t kUpPerKeypoint = 4 + 32 + 1 + 4 + 4 + 4, kUpFixed = 4 + 6 * 64;

int fail(const char* fn, int rc, const std::string& msg) { set_error(std::string(fn) + ": " + msg); return rc; }

size_t packed_bytes(const dvm_bt_keyframe& k) {
  const size_t n = (size_t)k.n, f = (size_t)k.fv_n, m = f ? (size_t)k.fv_off[f] : 0;
  return pad<64>(n * 4) + pad<64>(n * 32) + pad<64>(n) + pad<64>(f * 4) + pad<64>((f + 1) * 4) + pad<64>(m * 4);
}

// what the header lists under DVM_ERR_INVALID, for one keyframe; `seen` [>= n] is scratch and holds the listed features afterwards
int validate(const char* fn, const std::string& w, const dvm_bt_keyframe& k, uint8_t* seen) {
  if (k.n < 0 || k.n > kFrameCap) return fail(fn, DVM_ERR_INVALID, w + ": n outside [0, 8192]");
  if (k.fv_n < 0) return fail(fn, DVM_ERR_INVALID, w + ": negative node count");
  if (k.n > 0 && (!k.kps || !k.desc || !k.mp)) return fail(fn, DVM_ERR_INVALID, w + ": missing keypoint array");
  if (k.fv_n > 0 && (!k.fv_node || !k.fv_off || !k.fv_feat)) return fail(fn, DVM_ERR_INVALID, w + ": missing FeatureVector array");
  if (k.n > 0) std::memset(seen, 0, (size_t)k.n);
  if (k.fv_n == 0) return DVM_OK;
  if (k.fv_off[0] != 0) return fail(fn, DVM_ERR_INVALID, w + ": fv_off does not start at 0");
  for (int a = 0; a < k.fv_n; a++) {
    if (a > 0 && !((uint32_t)k.fv_node[a - 1] < (uint32_t)k.fv_node[a]))
      return fail(fn, DVM_ERR_INVALID, w + ": node ids not strictly ascending as unsigned");
    if (k.fv_off[a + 1] < k.fv_off[a]) return fail(fn, DVM_ERR_INVALID, w + ": fv_off decreases");
    if (k.fv_off[a + 1] > k.n) return fail(fn, DVM_ERR_INVALID, w + ": more listed features than keypoints (a feature is listed twice or lies outside [0, n))");
    for (int p = k.fv_off[a]; p < k.fv_off[a + 1]; p++) {
      const int32_t i = k.fv_feat[p];
      if (i < 0 || i >= k.n) return fail(fn, DVM_ERR_INVALID, w + ": a feature outside [0, n)");
      // a keypoint lies in ONE node: what the independence of the nodes, and with it the kernel, rests on
      if (seen[i]) return fail(fn, DVM_ERR_INVALID, w + ": feature " + std::to_string(i) + " listed twice");
      seen[i] = 1;
    }
  }
  return DVM_OK;
}

void pack(Cursor64& up, const dvm_bt_keyframe& k, BtKfDev& D) {
  const size_t n = (size_t)k.n, f = (size_t)k.fv_n, m = f ? (size_t)k.fv_off[f] : 0;
  float* angle = up.carve<float>(n);              // the search reads the angle alone: 4 of a keypoint's 28 bytes travel
  for (size_t i = 0; i < n; i++) angle[i] = k.kps[i].angle;
  D.angle = rebase(angle, up.base, up.twin);
  D.desc = up.put(k.desc, n * 32);
  uint8_t* use = up.carve<uint8_t>(n);
  for (size_t i = 0; i < n; i++) use[i] = k.mp[i] >= 0 && !(k.bad && k.bad[i]) ? 1 : 0;      // pMP && !pMP->isBad() (:742-748, :761-765)
  D.use = rebase(use, up.base, up.twin);
  D.fv_node = reinterpret_cast<const int32_t*>(up.put(k.fv_node, f * 4));
  if (f) D.fv_off = reinterpret_cast<const int32_t*>(up.put(k.fv_off, (f + 1) * 4));
  else { const int32_t zero = 0; D.fv_off = reinterpret_cast<const int32_t*>(up.put(&zero, 4)); }
  D.fv_feat = reinterpret_cast<const int32_t*>(up.put(k.fv_feat, m * 4));
  D.n = k.n; D.fv_n = k.fv_n;
}

// what the resident call adds in front of the search: the prologue's table and the stores its kernels read
struct Resident {
  const BtProKf* d_pro; int n_kf, n_max;
  const dvm_keyframe_store* kfs; const std::vector<const dvm_map_store*>* stores;
};
// the resident call behind its packing, as the uploaded call's second half runs (which keeps its own text): the upload region's first
// `copy` bytes sent with ONE copy, the prologue, the search and the settle kernels between the stores' read brackets, the results --
// [nmatches][match rows] in both blocks, the bins behind them on the device -- back with ONE copy behind ONE wait
int search_and_fetch(dvm_bow_targets* h, const char* fn, int T, int n1, int fv_n1, size_t copy, float nnratio, int check_ori, int32_t* d_cnt,
                     const Resident* R, int32_t* match_idx2, int32_t* nmatches) {
  const WorkingSet& ws = h->ws;
  const size_t E = (size_t)T * (size_t)n1;
  Cursor64 res{ws.d + h->up_bytes};
  int32_t* d_nm = res.carve<int32_t>((size_t)T);
  int32_t* d_match = res.carve<int32_t>(E);
  int8_t* d_bin = reinterpret_cast<int8_t*>(ws.d + h->up_bytes + h->res_bytes);
  uint8_t* h_res = ws.hm + h->up_bytes;
  const size_t back = pad<64>((size_t)T * 4) + E * 4;
  const BtKfDev* d_tab = reinterpret_cast<const BtKfDev*>(ws.d);
  const EventTimer& tm = h->timer;
  // a put or an update queued before this call is seen
  { const int rc = kfs_read_begin(R->kfs, h->s); if (rc != DVM_OK) return rc; }
  for (const dvm_map_store* st : *R->stores) { const int rc = store_read_begin(st, h->s); if (rc != DVM_OK) return rc; }
  DVM_HIP(hipMemcpyAsync(ws.d, ws.hm, copy, hipMemcpyHostToDevice, h->s));
  h->last_up = (int64_t)copy;
  DVM_HIP(tm.mark(3, h->s));
  launch_bt_prologue(h->s, d_tab, R->d_pro, R->n_kf, R->n_max, d_match, (int64_t)E, d_cnt, T * kBtCnt);
  DVM_HIP(tm.mark(0, h->s));
  launch_bt_search(h->s, d_tab, T, n1, fv_n1, nnratio, d_match, d_bin, d_cnt);
  DVM_HIP(tm.mark(1, h->s));
  launch_bt_settle(h->s, d_tab, T, n1, check_ori != 0, d_match, d_bin, d_cnt, d_nm);
  DVM_HIP(tm.mark(2, h->s));
  int rc = hip_check(hipGetLastError(), fn);
  // and one queued after never overtakes it (recorded whatever the launches returned)
  const int re = kfs_read_end(R->kfs, h->s);
  if (rc == DVM_OK) rc = re;
  for (const dvm_map_store* st : *R->stores) { const int rm = store_read_end(st, h->s); if (rc == DVM_OK) rc = rm; }
  if (rc == DVM_OK) rc = hip_check(hipMemcpyAsync(h_res, d_nm, back, hipMemcpyDeviceToHost, h->s), fn);
  const int rs = hip_check(hipStreamSynchronize(h->s), fn);
  if (rc != DVM_OK) return rc;
  if (rs != DVM_OK) return rs;
  if (tm.on) { DVM_HIP(tm.elapsed(0, 1, &h->last_ms[0])); DVM_HIP(tm.elapsed(1, 2, &h->last_ms[1])); DVM_HIP(tm.elapsed(3, 0, &h->last_ms[2])); }
  std::memcpy(nmatches, h_res, (size_t)T * 4);
  std::memcpy(match_idx2, h_res + pad<64>((size_t)T * 4), E * 4);
  return DVM_OK;
}
}  // namespace

extern "C" {

int dvm_bow_targets_create(int device, dvm_bow_targets** out) {
  const int rc = chain_create(device, out);
  if (rc == DVM_OK) { (*out)->seen.assign(kFrameCap, 0); (*out)->listed.assign(kFrameCap, 0); }
  return rc;
}
void dvm_bow_targets_destroy(dvm_bow_targets* h) { chain_destroy(h); }

int dvm_bow_targets_reserve(dvm_bow_targets* h, int max_cur, int max_targets, int max_total) {
  const char* fn = "dvm_bow_targets_reserve";
  if (!h || max_cur < 0 || max_cur > kFrameCap || max_targets < 0 || max_targets > kMaxTargets || max_total < 0 ||
      (int64_t)max_total > (int64_t)max_targets * kFrameCap)
    return fail(fn, DVM_ERR_INVALID, "bad sizes");
  if (max_cur <= h->max_cur && max_targets <= h->max_targets && max_total <= h->max_total) return DVM_OK;
  const int n1 = std::max(max_cur, h->max_cur), nt = std::max(max_targets, h->max_targets), tot = std::max(max_total, h->max_total);
  if ((int64_t)n1 * nt > kMaxEntries) return fail(fn, DVM_ERR_INVALID, "bad sizes");
  DVM_HIP(hipSetDevice(h->device));
  DVM_HIP(hipStreamSynchronize(h->s));
  h->up_bytes = h->res_bytes = h->bin_bytes = 0; h->max_cur = h->max_targets = h->max_total = 0;   // (a failed allocation leaves the handle holding nothing)
  const size_t up = pad<64>((size_t)(nt + 1) * sizeof(BtKfDev)) + ((size_t)n1 + (size_t)tot) * kUpPerKeypoint + (size_t)(nt + 1) * kUpFixed +
                    pad<64>((size_t)nt * kBtCnt * 4);
  const size_t res = pad<64>((size_t)nt * 4) + pad<64>((size_t)n1 * nt * 4);
  const size_t bin = pad<64>((size_t)n1 * nt);
  if (const char* what = h->ws.alloc(up + res + bin, up + res, up, /*mapped*/ false, /*zeroed*/ false))
    return fail(fn, DVM_ERR_HIP, std::string(what) + " failed");
  h->up_bytes = up; h->res_bytes = res; h->bin_bytes = bin;
  h->max_cur = n1; h->max_targets = nt; h->max_total = tot;
  return DVM_OK;
}

int dvm_bow_targets_profiling(dvm_bow_targets* h, int enable) {
  if (!h) return DVM_ERR_INVALID;
  DVM_HIP(hipSetDevice(h->device));
  return h->timer.enable(enable != 0);
}
int dvm_bow_targets_last_kernel_ms(dvm_bow_targets* h, float* ms) {
  if (!h || !ms) return DVM_ERR_INVALID;
  ms[0] = h->last_ms[0]; ms[1] = h->last_ms[1];
  return DVM_OK;
}
int dvm_bow_targets_last_prologue_ms(dvm_bow_targets* h, float* ms) {
  if (!h || !ms) return DVM_ERR_INVALID;
  *ms = h->last_ms[2];
  return DVM_OK;
}
int dvm_bow_targets_last_upload_bytes(const dvm_bow_targets* h, int64_t* bytes) {
  if (!h || !bytes) return DVM_ERR_INVALID;
  *bytes = h->last_up;
  return DVM_OK;
}

int dvm_search_by_bow_targets(dvm_bow_targets* h, const dvm_bt_keyframe* cur, int n_targets, const dvm_bt_keyframe* targets, float nnratio,
                              int check_ori, int32_t* match_idx2, int32_t* nmatches) {
  const char* fn = "dvm_search_by_bow_targets";
  if (!h || !cur || n_targets < 0 || (n_targets > 0 && (!targets || !nmatches))) return fail(fn, DVM_ERR_INVALID, "missing argument");
  // ---- every check before anything runs
  int64_t total = 0;
  size_t need = pad<64>((size_t)(n_targets + 1) * sizeof(BtKfDev)) + pad<64>((size_t)n_targets * kBtCnt * 4);
  for (int t = 0; t < n_targets; t++) {
    const int rc = validate(fn, "target " + std::to_string(t), targets[t], h->seen.data());
    if (rc != DVM_OK) return rc;
    total += targets[t].n;
    need += packed_bytes(targets[t]);
  }
  { const int rc = validate(fn, "the current keyframe", *cur, h->listed.data()); if (rc != DVM_OK) return rc; }
  need += packed_bytes(*cur);
  if (n_targets > 0 && cur->n > 0 && !match_idx2) return fail(fn, DVM_ERR_INVALID, "missing result array");
  if (cur->n > h->max_cur || n_targets > h->max_targets || total > h->max_total || need > h->up_bytes)
    return fail(fn, DVM_ERR_CAPACITY, "beyond the reservation (dvm_bow_targets_reserve): " + std::to_string(cur->n) + " keypoints against " +
                                          std::to_string(n_targets) + " targets with " + std::to_string(total) + " keypoints");
  const int T = n_targets, n1 = cur->n;
  const size_t E = (size_t)T * (size_t)n1;
  if (T == 0) return DVM_OK;
  if (n1 == 0 || cur->fv_n == 0) {              // no node to walk: every search returns 0 and leaves no match
    for (size_t e = 0; e < E; e++) match_idx2[e] = -1;
    for (int t = 0; t < T; t++) nmatches[t] = 0;
    return DVM_OK;
  }
  DVM_HIP(hipSetDevice(h->device));

  // ---- the upload: [table][current keyframe][targets][counters = 0]
  const WorkingSet& ws = h->ws;
  Cursor64 up{ws.hm, ws.d};
  BtKfDev* tab = up.carve<BtKfDev>((size_t)T + 1);
  std::memset(tab, 0, ((size_t)T + 1) * sizeof(BtKfDev));
  pack(up, *cur, tab[0]);
  for (int t = 0; t < T; t++) pack(up, targets[t], tab[1 + t]);
  int32_t* h_cnt = up.carve<int32_t>((size_t)T * kBtCnt);
  std::memset(h_cnt, 0, (size_t)T * kBtCnt * 4);
  int32_t* d_cnt = rebase(h_cnt, ws.hm, ws.d);
  if (up.used() > h->up_bytes) return fail(fn, DVM_ERR_STATE, "the packed keyframes exceed the reserved region");   // (an internal error: `need` is this sum)
  // ---- the results: [nmatches][match rows] in both blocks, the bins behind them on the device
  Cursor64 res{ws.d + h->up_bytes};
  int32_t* d_nm = res.carve<int32_t>((size_t)T);
  int32_t* d_match = res.carve<int32_t>(E);
  int8_t* d_bin = reinterpret_cast<int8_t*>(ws.d + h->up_bytes + h->res_bytes);
  uint8_t* h_res = ws.hm + h->up_bytes;
  const size_t back = pad<64>((size_t)T * 4) + E * 4;
  const BtKfDev* d_tab = reinterpret_cast<const BtKfDev*>(ws.d);

  DVM_HIP(hipMemcpyAsync(ws.d, ws.hm, up.used(), hipMemcpyHostToDevice, h->s));
  h->last_up = (int64_t)up.used();
  const EventTimer& tm = h->timer;
  DVM_HIP(tm.mark(0, h->s));
  launch_bt_search(h->s, d_tab, T, n1, cur->fv_n, nnratio, d_match, d_bin, d_cnt);
  DVM_HIP(tm.mark(1, h->s));
  launch_bt_settle(h->s, d_tab, T, n1, check_ori != 0, d_match, d_bin, d_cnt, d_nm);
  DVM_HIP(tm.mark(2, h->s));
  int rc = hip_check(hipGetLastError(), "dvm_search_by_bow_targets launch");
  if (rc == DVM_OK) rc = hip_check(hipMemcpyAsync(h_res, d_nm, back, hipMemcpyDeviceToHost, h->s), "dvm_search_by_bow_targets copy");
  const int rs = hip_check(hipStreamSynchronize(h->s), "dvm_search_by_bow_targets sync");
  if (rc != DVM_OK) return rc;
  if (rs != DVM_OK) return rs;
  if (tm.on) { DVM_HIP(tm.elapsed(0, 1, &h->last_ms[0])); DVM_HIP(tm.elapsed(1, 2, &h->last_ms[1])); h->last_ms[2] = 0; }
  std::memcpy(nmatches, h_res, (size_t)T * 4);
  std::memcpy(match_idx2, h_res + pad<64>((size_t)T * 4), E * 4);
  if (cur->fv_off[cur->fv_n] < n1) {            // a keypoint that no node lists (a stopped word) is never a query
    const uint8_t* listed = h->listed.data();
    for (int i = 0; i < n1; i++)
      if (!listed[i])
        for (int t = 0; t < T; t++) match_idx2[(size_t)t * n1 + i] = -1;
  }
  return DVM_OK;
}

int dvm_search_by_bow_targets_resident(dvm_bow_targets* h, const dvm_keyframe_store* kfs, const dvm_kf_resident* cur, int n_targets,
                                       const dvm_kf_resident* targets, float nnratio, int check_ori, int32_t* match_idx2, int32_t* nmatches) {
  const char* fn = "dvm_search_by_bow_targets_resident";
  if (!h || !kfs || !cur || n_targets < 0 || (n_targets > 0 && (!targets || !nmatches))) return fail(fn, DVM_ERR_INVALID, "missing argument");
  if (kfs_device(kfs) != h->device) return fail(fn, DVM_ERR_INVALID, "the keyframe store lives on another device");
  // ---- every check before anything is queued
  const int T = n_targets;
  h->views.resize((size_t)T + 1);
  h->stores.clear();
  int64_t total = 0;
  int n_max = 0;
  size_t copy = pad<64>(((size_t)T + 1) * sizeof(BtKfDev)) + pad<64>(((size_t)T + 1) * sizeof(BtProKf));   // the header's upload formula
  size_t derived = pad<64>((size_t)T * kBtCnt * 4);                                                         // what the prologue writes
  for (int k = 0; k <= T; k++) {
    const dvm_kf_resident& r = k ? targets[k - 1] : *cur;
    const std::string w = (k ? "target " + std::to_string(k - 1) : std::string("the current keyframe")) + " (slot " + std::to_string(r.slot) + ")";
    KfSlotView& v = h->views[k];
    if (!kfs_slot_view(kfs, r.slot, &v)) return fail(fn, DVM_ERR_INVALID, w + ": slot outside the store, never written or removed");
    if (v.n > 0 && !r.mp_slot) return fail(fn, DVM_ERR_INVALID, w + ": missing mp_slot");
    if (r.points && store_device(r.points) != h->device) return fail(fn, DVM_ERR_INVALID, w + ": its map store lives on another device");
    bool any = false;
    const int bad = store_kf_slots_check(r.points, r.mp_slot, v.n, &any);
    if (bad == 1) return fail(fn, DVM_ERR_INVALID, w + ": an mp_slot below -1, outside its map store or never written");
    if (bad == 2) return fail(fn, DVM_ERR_INVALID, w + ": an mp_slot names a point and points is NULL");
    // a keypoint lies in ONE node: what the independence of the nodes, and with it the kernel, rests on (put records it, fv_once.h)
    if (!v.fv_once) return fail(fn, DVM_ERR_INVALID, w + ": its FeatureVector lists a feature twice");
    if (any && std::find(h->stores.begin(), h->stores.end(), r.points) == h->stores.end()) h->stores.push_back(r.points);
    if (k) total += v.n;
    n_max = std::max(n_max, v.n);
    copy += pad<64>((size_t)v.n * 4);
    derived += pad<64>((size_t)v.n * 4) + pad<64>((size_t)v.n);
  }
  const int n1 = h->views[0].n, fv_n1 = h->views[0].fv_n;
  if (T > 0 && n1 > 0 && !match_idx2) return fail(fn, DVM_ERR_INVALID, "missing result array");
  if (n1 > h->max_cur || T > h->max_targets || total > h->max_total || copy + derived > h->up_bytes)
    return fail(fn, DVM_ERR_CAPACITY, "beyond the reservation (dvm_bow_targets_reserve): " + std::to_string(n1) + " keypoints against " +
                                          std::to_string(T) + " targets with " + std::to_string(total) + " keypoints");
  const size_t E = (size_t)T * (size_t)n1;
  if (T == 0) return DVM_OK;
  if (n1 == 0 || fv_n1 == 0) {                  // no node to walk: every search returns 0 and leaves no match
    for (size_t e = 0; e < E; e++) match_idx2[e] = -1;
    for (int t = 0; t < T; t++) nmatches[t] = 0;
    return DVM_OK;
  }
  DVM_HIP(hipSetDevice(h->device));

  // ---- the upload: [table][prologue table][mp_slot lists]; behind it, device only: [angle, use of every keyframe][counters]
  const WorkingSet& ws = h->ws;
  Cursor64 up{ws.hm, ws.d};
  BtKfDev* tab = up.carve<BtKfDev>((size_t)T + 1);
  BtProKf* pro = up.carve<BtProKf>((size_t)T + 1);
  for (int k = 0; k <= T; k++) {
    const dvm_kf_resident& r = k ? targets[k - 1] : *cur;
    const KfSlotView& v = h->views[k];
    pro[k].recs = r.points ? reinterpret_cast<const uint8_t*>(store_records(r.points)) : nullptr;
    pro[k].mp_slot = reinterpret_cast<const int32_t*>(up.put(r.mp_slot, (size_t)v.n * 4));
    pro[k].kps = reinterpret_cast<const uint8_t*>(v.kps);
    pro[k].reserved = 0;
  }
  if (up.used() != copy) return fail(fn, DVM_ERR_STATE, "the upload differs from its formula");   // (an internal error)
  for (int k = 0; k <= T; k++) {
    const KfSlotView& v = h->views[k];
    BtKfDev& D = tab[k];
    D.angle = rebase(up.carve<float>((size_t)v.n), ws.hm, ws.d);
    D.use = rebase(up.carve<uint8_t>((size_t)v.n), ws.hm, ws.d);
    D.desc = v.desc; D.fv_node = v.fv_node; D.fv_off = v.fv_off; D.fv_feat = v.fv_feat;
    D.n = v.n; D.fv_n = v.fv_n;
  }
  int32_t* d_cnt = rebase(up.carve<int32_t>((size_t)T * kBtCnt), ws.hm, ws.d);
  if (up.used() > h->up_bytes) return fail(fn, DVM_ERR_STATE, "the call's block exceeds the reserved region");   // (an internal error: copy + derived is this sum)
  const Resident R{rebase(pro, ws.hm, ws.d), T + 1, n_max, kfs, &h->stores};
  return search_and_fetch(h, fn, T, n1, fv_n1, copy, nnratio, check_ori, d_cnt, &R, match_idx2, nmatches);
}

}  // extern "C"
