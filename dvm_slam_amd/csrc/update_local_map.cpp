// dvm_slam_amd/csrc/update_local_map.cpp -- dvm_update_local_map (include/dvmslam_hip.h): Tracking::UpdateLocalMap's two graph walks on the
// rows a dvm_keyframe_store keeps beside its keyframes and the records of a dvm_map_store, for the frames of one tick.
//   dvm_update_local_map_keyframes   the vote loop of UpdateLocalKeyFrames (reference src/Tracking.cc:3145-3181)
//   dvm_update_local_map_points      UpdateLocalPoints (:3117-3141) and the frame_mp the second half of the tracked frame takes
// Each call: every check on the host (update_local_map_lists.h), ONE upload -- a 64-byte parameter block per frame and the frames' lists,
// nothing per keyframe of a store or per entry of a row --, ONE chain of launches batched over the frames (update_local_map_kernels.hip)
// on the handle's stream, ONE synchronisation; the results lie in a mapped page-locked block behind it.  The call reads its stores
// between store_read_begin / kfs_read_begin and _read_end: it sees every update, commit, put and row edit queued before it, and none
// overtakes it.
// The per-frame tables (mult, first, pos: map_capacity words each) are idle between calls: the kernels put back what they touched, and a
// call refused on the host has queued nothing.  A call that fails on the device (DVM_ERR_HIP behind its first launch) closes the stores'
// read brackets, and the next call on the handle writes the tables idle again before it runs.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dvmslam_hip.h"
#include "chain.h"
#include "keyframe_store.h"
#include "map_store.h"
#include "update_local_map_kernels.h"
#include "update_local_map_lists.h"

using namespace dvm;

namespace {
// the two blocks of a reservation, each walked by one layout (a null base measures)
struct UlmDevBlock { uint8_t* up; int32_t *mult, *first, *pos, *cnt, *off; size_t bytes; };
struct UlmHostBlock { uint8_t* up; int32_t* votes; uint8_t* frame_bad; int32_t *local, *frame_mp, *counts; size_t bytes; };
size_t up_capacity(const UlmReserve& R) {
  return (size_t)R.max_frames * (kUlmParamBytes + 4 * (ulm_pad16((size_t)R.max_frame_keypoints) + ulm_pad16((size_t)R.max_local_keyframes)));
}
size_t blocks_max(const UlmReserve& R) { return (size_t)R.max_local_keyframes * (size_t)ulm_row_blocks(R.slot_keypoints); }
UlmDevBlock dev_layout(uint8_t* base, const UlmReserve& R) {
  Cursor<64> c{base};
  const size_t F = (size_t)R.max_frames, M = (size_t)R.map_capacity;
  UlmDevBlock D{};
  D.up = c.carve<uint8_t>(up_capacity(R));
  D.mult = c.carve<int32_t>(F * M); D.first = c.carve<int32_t>(F * M); D.pos = c.carve<int32_t>(F * M);
  D.cnt = c.carve<int32_t>(F * (blocks_max(R) + 1)); D.off = c.carve<int32_t>(F * (blocks_max(R) + 1));
  D.bytes = c.used();
  return D;
}
UlmHostBlock host_layout(uint8_t* base, const UlmReserve& R) {
  Cursor<64> c{base};
  const size_t F = (size_t)R.max_frames, np = ulm_pad16((size_t)R.max_frame_keypoints);
  UlmHostBlock H{};
  H.up = c.carve<uint8_t>(up_capacity(R));
  H.votes = c.carve<int32_t>(F * (size_t)R.kf_capacity); H.frame_bad = c.carve<uint8_t>(F * np);
  H.local = c.carve<int32_t>(F * (size_t)R.map_capacity); H.frame_mp = c.carve<int32_t>(F * np); H.counts = c.carve<int32_t>(F * 2);
  H.bytes = c.used();
  return H;
}
int fail(const char* fn, int rc, const std::string& msg) { set_error(std::string(fn) + ": " + msg); return rc; }
}  // namespace

struct dvm_update_local_map : dvm::Chain {
  UlmReserve R{0, 0, 0, 0, 0, 1};
  bool reserved = false;
  std::vector<uint32_t> stamp; uint32_t call = 0;   // [kf_capacity] a keyframe slot named twice in one frame
  std::vector<uint8_t> kf_state;                    // [max_local_keyframes] what the store knows of a frame's named slots
  int64_t last_h2d = 0, last_d2h = 0;
  float last_ms = 0.f;
  bool dirty = false;                               // a call failed after its first launch was queued: the tables may hold its entries
};

namespace {
std::string refusal(const UlmVerdict& v, const int32_t* list_entry) {
  const std::string f = v.frame >= 0 ? "frame " + std::to_string(v.frame) : std::string("the call");
  const std::string e = v.at >= 0 ? ", entry " + std::to_string(v.at) + (list_entry ? " (slot " + std::to_string(*list_entry) + ")" : std::string()) : std::string();
  switch (v.fault) {
    case kUlmNull: return f + ": a NULL argument with a non-zero count";
    case kUlmCount: return f + ": a negative count";
    case kUlmNoReserve: return "nothing reserved (dvm_update_local_map_reserve)";
    case kUlmFrames: return "more frames than max_frames of the reservation";
    case kUlmKeypoints: return f + ": more keypoints than max_frame_keypoints of the reservation";
    case kUlmLocalKfs: return f + ": more keyframes named than max_local_keyframes of the reservation";
    case kUlmMapTable: return f + ": the map store holds more slots than map_capacity of the reservation";
    case kUlmKfTable: return f + ": the keyframe store holds more slots than kf_capacity of the reservation";
    case kUlmSlotKeypoints: return f + ": the keyframe store's slot_keypoints beyond the reservation's";
    case kUlmDevice: return f + ": a store lives on another device";
    case kUlmFrameSlot: return f + e + ": a frame slot below -1, outside its map store or never written";
    case kUlmKfSlot: return f + e + ": kf_slot outside the store, never put or removed";
    case kUlmKfNoRow: return f + e + ": kf_slot without a MATCHES row";
    case kUlmKfTwice: return f + e + ": kf_slot named twice in one frame";
    case kUlmRowStore: return f + e + ": the slot's MATCHES row names another map store than the frame's";
    case kUlmObservedStore: return f + ": an OBSERVED row of the keyframe store names another map store than the frame's";
    default: return "bad sizes";
  }
}
UlmFacts facts_of(const dvm_update_local_map* h, const dvm_keyframe_store* kfs, const dvm_map_store* points) {
  UlmFacts F{};
  F.same_device = kfs_device(kfs) == h->device && store_device(points) == h->device;
  F.map_capacity = dvm_map_store_capacity(points); F.written = store_written(points);
  F.kf_capacity = kfs_capacity(kfs); F.slot_keypoints = dvm_keyframe_store_slot_keypoints(kfs);
  F.observed_same = true; F.kf_state = nullptr;
  return F;
}
// the frames' stores, each once: a reader's bracket
template <class In> int read_begin(const In* in, int count, hipStream_t s) {
  for (int b = 0; b < count; b++) {
    bool kf_seen = false, mp_seen = false;
    for (int a = 0; a < b; a++) { kf_seen |= in[a].kfs == in[b].kfs; mp_seen |= in[a].points == in[b].points; }
    if (!kf_seen) { const int rc = kfs_read_begin(in[b].kfs, s); if (rc != DVM_OK) return rc; }
    if (!mp_seen) { const int rc = store_read_begin(in[b].points, s); if (rc != DVM_OK) return rc; }
  }
  return DVM_OK;
}
template <class In> int read_end(const In* in, int count, hipStream_t s) {
  for (int b = 0; b < count; b++) {
    bool kf_seen = false, mp_seen = false;
    for (int a = 0; a < b; a++) { kf_seen |= in[a].kfs == in[b].kfs; mp_seen |= in[a].points == in[b].points; }
    if (!kf_seen) { const int rc = kfs_read_end(in[b].kfs, s); if (rc != DVM_OK) return rc; }
    if (!mp_seen) { const int rc = store_read_end(in[b].points, s); if (rc != DVM_OK) return rc; }
  }
  return DVM_OK;
}
// mult, first and pos idle (reserve; and the next call behind one that failed on the device)
int idle_tables(dvm_update_local_map* h, const UlmReserve& R) {
  const UlmDevBlock D = dev_layout(h->ws.d, R);
  const size_t words = (size_t)R.max_frames * (size_t)R.map_capacity;
  if (words) {
    DVM_HIP(hipMemsetAsync(D.mult, 0, words * 4, h->s));
    DVM_HIP(hipMemsetAsync(D.first, 0x7f, words * 4, h->s));
    DVM_HIP(hipMemsetAsync(D.pos, 0xff, words * 4, h->s));
  }
  DVM_HIP(hipStreamSynchronize(h->s));
  return DVM_OK;
}
// in front of a call's upload: a handle whose last call failed on the device gets its tables back first
int make_clean(dvm_update_local_map* h) {
  if (!h->dirty) return DVM_OK;
  (void)hipGetLastError();
  const int rc = idle_tables(h, h->R);
  if (rc == DVM_OK) h->dirty = false;
  return rc;
}
// a HIP call failed between read_begin and the call's synchronisation: the stores' read brackets are closed as far as the stream allows
// (their next writers wait for whatever the stream still holds), and the handle's tables count as touched
template <class In> int run_failed(dvm_update_local_map* h, const In* in, int count, int rc) {
  h->dirty = true;
  (void)read_end(in, count, h->s);
  (void)hipGetLastError();
  return rc;
}
// the part of UlmArgs that does not depend on the call
UlmArgs args_of(const dvm_update_local_map* h, size_t up_lists_off) {
  const UlmDevBlock D = dev_layout(h->ws.d, h->R);
  const UlmHostBlock H = host_layout(h->ws.hm_dev, h->R);
  UlmArgs A{};
  A.frames = reinterpret_cast<const UlmFrameDev*>(D.up);
  A.lists = reinterpret_cast<const int32_t*>(D.up + up_lists_off);
  A.mult = D.mult; A.first = D.first; A.pos = D.pos; A.map_capacity = h->R.map_capacity;
  A.cnt = D.cnt; A.off = D.off; A.blocks_max = (int32_t)blocks_max(h->R); A.row_blocks = ulm_row_blocks(h->R.slot_keypoints);
  A.votes = H.votes; A.frame_bad = H.frame_bad; A.local = H.local; A.frame_mp = H.frame_mp; A.counts = H.counts;
  A.kf_capacity_res = h->R.kf_capacity; A.n_pad = (int32_t)ulm_pad16((size_t)h->R.max_frame_keypoints);
  return A;
}
}  // namespace

extern "C" {

int dvm_update_local_map_create(int device, dvm_update_local_map** out) { return chain_create(device, out); }
void dvm_update_local_map_destroy(dvm_update_local_map* h) { chain_destroy(h); }

int dvm_update_local_map_reserve(dvm_update_local_map* h, int max_frames, int max_frame_keypoints, int max_local_keyframes, int map_capacity,
                                 int kf_capacity, int slot_keypoints) {
  const char* fn = "dvm_update_local_map_reserve";
  if (!h) return DVM_ERR_INVALID;
  UlmReserve R{max_frames, max_frame_keypoints, max_local_keyframes, map_capacity, kf_capacity, slot_keypoints};
  if (ulm_check_reserve(R).fault != kUlmOk)
    return fail(fn, DVM_ERR_INVALID, "a negative size, slot_keypoints outside [1, 8192], or tables beyond 2^31 words");
  if (h->reserved) {                                               // grow-only
    const UlmReserve& O = h->R;
    if (R.max_frames <= O.max_frames && R.max_frame_keypoints <= O.max_frame_keypoints && R.max_local_keyframes <= O.max_local_keyframes &&
        R.map_capacity <= O.map_capacity && R.kf_capacity <= O.kf_capacity && R.slot_keypoints <= O.slot_keypoints)
      return DVM_OK;
    R = UlmReserve{std::max(R.max_frames, O.max_frames), std::max(R.max_frame_keypoints, O.max_frame_keypoints),
                   std::max(R.max_local_keyframes, O.max_local_keyframes), std::max(R.map_capacity, O.map_capacity),
                   std::max(R.kf_capacity, O.kf_capacity), std::max(R.slot_keypoints, O.slot_keypoints)};
    if (ulm_check_reserve(R).fault != kUlmOk) return fail(fn, DVM_ERR_INVALID, "tables beyond 2^31 words");
  }
  DVM_HIP(hipSetDevice(h->device));
  DVM_HIP(hipStreamSynchronize(h->s));
  h->reserved = false;                                             // (a failed allocation leaves the handle holding nothing)
  const UlmDevBlock Dm = dev_layout(nullptr, R);
  const UlmHostBlock Hm = host_layout(nullptr, R);
  if (const char* what = h->ws.alloc(std::max(Dm.bytes, (size_t)64), std::max(Hm.bytes, (size_t)64), up_capacity(R), true, true)) {
    (void)hipGetLastError();
    return fail(fn, DVM_ERR_CAPACITY, std::string(what) + " (" + std::to_string(Dm.bytes) + " device bytes, " + std::to_string(Hm.bytes) + " page-locked)");
  }
  // the tables idle, once: every call puts back what it touched
  { const int rc = idle_tables(h, R); if (rc != DVM_OK) { h->ws.free(); return rc; } }
  h->dirty = false;
  h->R = R; h->reserved = true;
  h->stamp.assign((size_t)R.kf_capacity, 0u); h->call = 0;
  h->kf_state.assign((size_t)R.max_local_keyframes, 0);
  return DVM_OK;
}

int dvm_update_local_map_keyframes(dvm_update_local_map* h, int count, const dvm_ulm_keyframes_in* in, const dvm_ulm_keyframes_out* out) {
  static_assert(sizeof(UlmFrameDev) == kUlmParamBytes, "the parameter block");
  const char* fn = "dvm_update_local_map_keyframes";
  if (!h) return DVM_ERR_INVALID;
  if (count < 0) return fail(fn, DVM_ERR_INVALID, "a negative count");
  if (count == 0) return DVM_OK;
  if (!in || !out) return fail(fn, DVM_ERR_INVALID, "a NULL argument with a non-zero count");
  if (!h->reserved) return fail(fn, DVM_ERR_CAPACITY, refusal(ulm_fail(kUlmNoReserve), nullptr));
  if (count > h->R.max_frames) return fail(fn, DVM_ERR_CAPACITY, refusal(ulm_fail(kUlmFrames), nullptr));
  // every frame is decided before anything is queued
  for (int b = 0; b < count; b++) {
    if (!in[b].kfs || !in[b].points) return fail(fn, DVM_ERR_INVALID, refusal(ulm_fail(kUlmNull, b), nullptr));
    UlmFacts F = facts_of(h, in[b].kfs, in[b].points);
    F.observed_same = kfs_rows_all_name(in[b].kfs, DVM_KFS_ROW_OBSERVED, in[b].points);
    const UlmVerdict v = ulm_check_keyframes_frame(h->R, F, b, in[b], out[b]);
    if (v.fault != kUlmOk) return fail(fn, v.rc(), refusal(v, v.fault == kUlmFrameSlot ? &in[b].mp_slot[v.at] : nullptr));
  }
  DVM_HIP(hipSetDevice(h->device));
  { const int rc = make_clean(h); if (rc != DVM_OK) return rc; }
  // the one upload: the parameter blocks, then the frames' lists
  const size_t lists_off = (size_t)count * kUlmParamBytes;
  UlmFrameDev* P = reinterpret_cast<UlmFrameDev*>(h->ws.hm);
  int32_t* lists = reinterpret_cast<int32_t*>(h->ws.hm + lists_off);
  size_t w = 0;
  int n_max = 0, c_max = 0;
  for (int b = 0; b < count; b++) {
    const KfsRowsView V = kfs_rows_view(in[b].kfs, DVM_KFS_ROW_OBSERVED);
    UlmFrameDev& p = P[b];
    std::memset(&p, 0, sizeof(p));
    p.records = reinterpret_cast<const uint32_t*>(store_records(in[b].points));
    p.rows = V.rows; p.len = V.len; p.row_words = (int32_t)V.row_words;
    p.n = in[b].n; p.kf_capacity = kfs_capacity(in[b].kfs);
    p.mp_off = (int32_t)w;
    if (in[b].n > 0) std::memcpy(lists + w, in[b].mp_slot, (size_t)in[b].n * 4);
    w += ulm_pad16((size_t)in[b].n);
    n_max = std::max(n_max, in[b].n); c_max = std::max(c_max, p.kf_capacity);
  }
  const size_t up = lists_off + 4 * w;                             // == ulm_keyframes_upload_bytes(count, in)
  hipStream_t s = h->s;
  const UlmArgs A = args_of(h, lists_off);
  auto queued = [&]() -> int {
    { const int rc = read_begin(in, count, s); if (rc != DVM_OK) return rc; }
    DVM_HIP(hipMemcpyAsync(h->ws.d, h->ws.hm, up, hipMemcpyHostToDevice, s));
    DVM_HIP(h->timer.mark(0, s));
    launch_ulm_keyframes(s, A, count, n_max, c_max);
    { const int rc = hip_check(hipGetLastError(), "the vote kernels"); if (rc != DVM_OK) return rc; }
    DVM_HIP(h->timer.mark(1, s));
    { const int rc = read_end(in, count, s); if (rc != DVM_OK) return rc; }
    DVM_HIP(hipStreamSynchronize(s));                              // the ONE synchronisation: the results lie in mapped memory behind it
    return DVM_OK;
  };
  { const int rc = queued(); if (rc != DVM_OK) return run_failed(h, in, count, rc); }
  if (h->timer.on) DVM_HIP(h->timer.elapsed(0, 1, &h->last_ms));
  const UlmHostBlock H = host_layout(h->ws.hm, h->R);
  h->last_h2d = (int64_t)up; h->last_d2h = 0;
  for (int b = 0; b < count; b++) {
    const size_t C = (size_t)kfs_capacity(in[b].kfs);
    std::memcpy(out[b].votes, H.votes + (size_t)b * (size_t)h->R.kf_capacity, C * 4);
    if (in[b].n > 0) std::memcpy(out[b].frame_bad, H.frame_bad + (size_t)b * (size_t)A.n_pad, (size_t)in[b].n);
    h->last_d2h += (int64_t)(C * 4 + (size_t)in[b].n);
  }
  return DVM_OK;
}

int dvm_update_local_map_points(dvm_update_local_map* h, int count, const dvm_ulm_points_in* in, dvm_ulm_points_out* out) {
  const char* fn = "dvm_update_local_map_points";
  if (!h) return DVM_ERR_INVALID;
  if (count < 0) return fail(fn, DVM_ERR_INVALID, "a negative count");
  if (count == 0) return DVM_OK;
  if (!in || !out) return fail(fn, DVM_ERR_INVALID, "a NULL argument with a non-zero count");
  if (!h->reserved) return fail(fn, DVM_ERR_CAPACITY, refusal(ulm_fail(kUlmNoReserve), nullptr));
  if (count > h->R.max_frames) return fail(fn, DVM_ERR_CAPACITY, refusal(ulm_fail(kUlmFrames), nullptr));
  for (int b = 0; b < count; b++) {
    if (!in[b].kfs || !in[b].points) return fail(fn, DVM_ERR_INVALID, refusal(ulm_fail(kUlmNull, b), nullptr));
    UlmFacts F = facts_of(h, in[b].kfs, in[b].points);
    if (in[b].n_kfs > 0 && in[b].n_kfs <= h->R.max_local_keyframes && in[b].kf_slot) {
      for (int k = 0; k < in[b].n_kfs; k++) {
        KfSlotView v;
        int32_t len = 0;
        const dvm_map_store* names = nullptr;
        const int32_t sl = in[b].kf_slot[k];
        h->kf_state[k] = !kfs_slot_view(in[b].kfs, sl, &v)                                ? kUlmKfAbsent
                         : !kfs_row_info(in[b].kfs, DVM_KFS_ROW_MATCHES, sl, &len, &names) ? kUlmKfRowless
                         : names != in[b].points                                           ? kUlmKfOtherStore
                                                                                           : kUlmKfGood;
      }
    }
    F.kf_state = h->kf_state.data();
    if (++h->call == 0) { std::fill(h->stamp.begin(), h->stamp.end(), 0u); h->call = 1; }
    const UlmVerdict v = ulm_check_points_frame(h->R, F, b, in[b], out[b], h->stamp.data(), h->call);
    if (v.fault != kUlmOk)
      return fail(fn, v.rc(), refusal(v, v.fault == kUlmFrameSlot ? &in[b].mp_slot[v.at] : v.at >= 0 ? &in[b].kf_slot[v.at] : nullptr));
  }
  DVM_HIP(hipSetDevice(h->device));
  { const int rc = make_clean(h); if (rc != DVM_OK) return rc; }
  const size_t lists_off = (size_t)count * kUlmParamBytes;
  UlmFrameDev* P = reinterpret_cast<UlmFrameDev*>(h->ws.hm);
  int32_t* lists = reinterpret_cast<int32_t*>(h->ws.hm + lists_off);
  size_t w = 0;
  int kfs_max = 0;
  for (int b = 0; b < count; b++) {
    const KfsRowsView V = kfs_rows_view(in[b].kfs, DVM_KFS_ROW_MATCHES);
    UlmFrameDev& p = P[b];
    std::memset(&p, 0, sizeof(p));
    p.records = reinterpret_cast<const uint32_t*>(store_records(in[b].points));
    p.rows = V.rows; p.len = V.len; p.row_words = (int32_t)V.row_words;
    p.n = in[b].n; p.n_kfs = in[b].n_kfs; p.kf_capacity = kfs_capacity(in[b].kfs);
    p.local_cap = std::min(out[b].local_cap, h->R.map_capacity);
    p.mp_off = (int32_t)w;
    if (in[b].n > 0) std::memcpy(lists + w, in[b].mp_slot, (size_t)in[b].n * 4);
    w += ulm_pad16((size_t)in[b].n);
    p.kf_off = (int32_t)w;
    if (in[b].n_kfs > 0) std::memcpy(lists + w, in[b].kf_slot, (size_t)in[b].n_kfs * 4);
    w += ulm_pad16((size_t)in[b].n_kfs);
    kfs_max = std::max(kfs_max, in[b].n_kfs);
  }
  const size_t up = lists_off + 4 * w;                             // == ulm_points_upload_bytes(count, in)
  hipStream_t s = h->s;
  const UlmArgs A = args_of(h, lists_off);
  auto queued = [&]() -> int {
    { const int rc = read_begin(in, count, s); if (rc != DVM_OK) return rc; }
    DVM_HIP(hipMemcpyAsync(h->ws.d, h->ws.hm, up, hipMemcpyHostToDevice, s));
    DVM_HIP(h->timer.mark(0, s));
    launch_ulm_points(s, A, count, kfs_max);
    { const int rc = hip_check(hipGetLastError(), "the local-point kernels"); if (rc != DVM_OK) return rc; }
    DVM_HIP(h->timer.mark(1, s));
    { const int rc = read_end(in, count, s); if (rc != DVM_OK) return rc; }
    DVM_HIP(hipStreamSynchronize(s));                              // the ONE synchronisation
    return DVM_OK;
  };
  { const int rc = queued(); if (rc != DVM_OK) return run_failed(h, in, count, rc); }
  if (h->timer.on) DVM_HIP(h->timer.elapsed(0, 1, &h->last_ms));
  const UlmHostBlock H = host_layout(h->ws.hm, h->R);
  h->last_h2d = (int64_t)up; h->last_d2h = 0;
  int over = -1;
  for (int b = 0; b < count; b++) {
    const int32_t n_local = H.counts[2 * b], got = std::min(n_local, out[b].local_cap);
    out[b].n_local = n_local; out[b].n_outside = H.counts[2 * b + 1];
    if (got > 0) std::memcpy(out[b].local_slot, H.local + (size_t)b * (size_t)h->R.map_capacity, (size_t)got * 4);
    if (in[b].n > 0) std::memcpy(out[b].frame_mp, H.frame_mp + (size_t)b * (size_t)A.n_pad, (size_t)in[b].n * 4);
    h->last_d2h += (int64_t)(((size_t)got + (size_t)in[b].n + 2) * 4);
    if (n_local > out[b].local_cap && over < 0) over = b;
  }
  if (over >= 0)
    return fail(fn, DVM_ERR_CAPACITY, "frame " + std::to_string(over) + ": " + std::to_string(out[over].n_local) + " local points beyond local_cap " +
                                          std::to_string(out[over].local_cap) + " (n_local holds the count; frame_mp is complete)");
  return DVM_OK;
}

int dvm_update_local_map_last_bytes(const dvm_update_local_map* h, int64_t* host_to_device, int64_t* device_to_host) {
  if (!h || !host_to_device || !device_to_host) return DVM_ERR_INVALID;
  *host_to_device = h->last_h2d; *device_to_host = h->last_d2h;
  return DVM_OK;
}

int dvm_update_local_map_profile(dvm_update_local_map* h, int enable) {
  if (!h) return DVM_ERR_INVALID;
  DVM_HIP(hipSetDevice(h->device));
  return h->timer.enable(enable != 0);
}

int dvm_update_local_map_last_ms(const dvm_update_local_map* h, float* kernel_ms) {
  if (!h || !kernel_ms) return DVM_ERR_INVALID;
  *kernel_ms = h->last_ms;
  return DVM_OK;
}

}  // extern "C"
