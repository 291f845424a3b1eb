// dvm_slam_amd/csrc/keyframe_store.cpp -- dvm_keyframe_store (include/dvmslam_hip.h): an agent's keyframes resident on the device.
//
// What a KeyFrame holds once ComputeBoW has run -- mvKeysUn, mDescriptors, the level tables, mFeatVec, the image bounds and the feature
// grid -- lives in one device block of `capacity` slots (kf_store_layout.h) that never moves.  LocalMapping puts a keyframe once; the
// Fuse chain and the CreateNewMapPoints chain read it step after step (fuse_targets.cpp: dvm_fuse_targets_set_resident; new_points.cpp:
// dvm_create_new_map_points_resident) and send only what changes, the pose and mvpMapPoints.
//
// Ordering is map_store.cpp's -- the store's own stream plus two events:
//   put      validates the whole batch, then in rounds: packs keyframes into the page-locked staging block ([items][arrays]), makes the
//            store's stream wait for `read_ev` (the last kernel a chain queued to read the store), sends ONE copy to the staging block's
//            device twin, launches k_kfs_put there and records `write_ev`.  It returns without waiting; the next round (or put) waits on
//            the host for `write_ev` before it touches the staging block again.
//   a chain  kfs_read_begin: its stream waits for `write_ev`; kfs_read_end: `read_ev` recorded behind its reading kernels.
// Safety: per slot the host keeps a written flag, a generation and the counts the kernels index with; every slot a call names is checked
// BEFORE anything is queued, and every count of a put is bounded by slot_keypoints, so no kernel runs on an unchecked value.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/dvmslam_hip.h"
#include "chain.h"
#include "fv_once.h"
#include "keyframe_store.h"

using namespace dvm;

namespace {
constexpr int kStageKeyframes = 32;              // keyframes of the largest size one round holds (smaller ones: more)
struct SlotMeta {
  uint8_t written = 0;
  uint8_t fv_once = 0;                             // the FeatureVector lists every feature at most once (fv_once.h): what the BoW-targets search needs
  uint32_t gen = 0;
  int32_t n = 0, fv_n = 0, n_feat = 0, n_levels = 0;
  float fx = 0, fy = 0, cx = 0, cy = 0, min_x = 0, max_x = 0, min_y = 0, max_y = 0, log_scale_factor = 0;
};
int fail(const char* fn, int rc, const std::string& msg) { set_error(std::string(fn) + ": " + msg); return rc; }
}  // namespace

struct dvm_keyframe_store {
  int device = 0, capacity = 0, K = 0;
  KfSlotLayout L{};
  uint8_t* d = nullptr;                            // [capacity] slots of L.stride bytes
  uint8_t *hs = nullptr, *ds = nullptr;            // staging: page-locked, and its device twin; [items: capacity][arrays]
  size_t item_bytes = 0, stage_bytes = 0;
  hipStream_t s = nullptr;
  hipEvent_t write_ev = nullptr, read_ev = nullptr;
  bool write_pending = false, read_pending = false;
  std::vector<SlotMeta> meta;
  std::vector<uint32_t> stamp; uint32_t call = 0;  // per slot: the put call that named it last (a slot named twice in one call)
  std::vector<uint8_t> seen;                       // [K] scratch of the listed-once scan
  uint8_t* slot_base(int32_t sl) const { return d + (size_t)sl * L.stride; }
  // the staging block is the host's again: the last round's copy has read it
  int staging_free() {
    if (write_pending) { DVM_HIP(hipEventSynchronize(write_ev)); write_pending = false; }
    return DVM_OK;
  }
};

namespace dvm {
int kfs_device(const dvm_keyframe_store* st) { return st->device; }
bool kfs_slot_view(const dvm_keyframe_store* st, int32_t slot, KfSlotView* v) {
  if ((uint32_t)slot >= (uint32_t)st->capacity || !st->meta[slot].written) return false;
  const SlotMeta& m = st->meta[slot];
  const KfSlotLayout& L = st->L;
  uint8_t* b = st->slot_base(slot);
  v->kps = reinterpret_cast<const dvm_keypoint_pod*>(b + L.kps);
  v->desc = b + L.desc;
  v->fv_node = reinterpret_cast<const int32_t*>(b + L.fv_node);
  v->fv_off = reinterpret_cast<const int32_t*>(b + L.fv_off);
  v->fv_feat = reinterpret_cast<const int32_t*>(b + L.fv_feat);
  v->sf = reinterpret_cast<const float*>(b + L.sf);
  v->sigma2 = reinterpret_cast<const float*>(b + L.sigma2);
  v->inv_sigma2 = reinterpret_cast<const float*>(b + L.inv_sigma2);
  FrameView& F = v->F;
  F.skp = reinterpret_cast<float4*>(b + L.skp);
  F.sidx = reinterpret_cast<int32_t*>(b + L.sidx);
  F.sdesc = b + L.sdesc;
  F.cell_start = reinterpret_cast<int32_t*>(b + L.cell_start);
  F.n_sorted = reinterpret_cast<int32_t*>(b + L.counters);
  F.n_total = F.n_sorted + 1;
  F.n_overflow = F.n_sorted + 2;
  F.cap = m.n;
  F.minX = m.min_x; F.minY = m.min_y;
  F.wInv = static_cast<float>(64) / static_cast<float>(m.max_x - m.min_x);   // Frame.cc:443-444, as dvm_frame_build
  F.hInv = static_cast<float>(48) / static_cast<float>(m.max_y - m.min_y);
  v->n = m.n; v->fv_n = m.fv_n; v->n_feat = m.n_feat; v->n_levels = m.n_levels;
  v->fx = m.fx; v->fy = m.fy; v->cx = m.cx; v->cy = m.cy;
  v->min_x = m.min_x; v->max_x = m.max_x; v->min_y = m.min_y; v->max_y = m.max_y; v->log_scale_factor = m.log_scale_factor;
  v->gen = m.gen; v->fv_once = m.fv_once != 0;
  return true;
}
uint32_t kfs_generation(const dvm_keyframe_store* st, int32_t slot) { return (uint32_t)slot < (uint32_t)st->capacity ? st->meta[slot].gen : 0u; }
int kfs_read_begin(const dvm_keyframe_store* cst, hipStream_t s) {
  dvm_keyframe_store* st = const_cast<dvm_keyframe_store*>(cst);
  if (!st->write_pending) return DVM_OK;
  if (hipEventQuery(st->write_ev) == hipSuccess) { st->write_pending = false; return DVM_OK; }   // (a put that has run needs no wait, now or later)
  (void)hipGetLastError();     // hipErrorNotReady is no error
  DVM_HIP(hipStreamWaitEvent(s, st->write_ev, 0));
  return DVM_OK;
}
int kfs_read_end(const dvm_keyframe_store* cst, hipStream_t s) {
  dvm_keyframe_store* st = const_cast<dvm_keyframe_store*>(cst);
  DVM_HIP(hipEventRecord(st->read_ev, s));
  st->read_pending = true;
  return DVM_OK;
}
}  // namespace dvm

namespace {
// everything dvm_fuse_targets_set and dvm_create_new_map_points check of a keyframe per call, once
int check_keyframe(const char* fn, const dvm_kfs_keyframe& k, const std::string& w, int K) {
  if (k.n < 0) return fail(fn, DVM_ERR_INVALID, w + ": negative n");
  if (k.n > K) return fail(fn, DVM_ERR_CAPACITY, w + ": " + std::to_string(k.n) + " keypoints beyond slot_keypoints " + std::to_string(K));
  if (k.n_levels < 1 || k.n_levels > 64) return fail(fn, DVM_ERR_INVALID, w + ": n_levels outside [1, 64]");
  if (!k.scale_factors || !k.level_sigma2 || !k.inv_level_sigma2) return fail(fn, DVM_ERR_INVALID, w + ": missing level table");
  if (!(k.max_x > k.min_x) || !(k.max_y > k.min_y)) return fail(fn, DVM_ERR_INVALID, w + ": image bounds empty");
  if (k.n > 0 && (!k.kps || !k.desc)) return fail(fn, DVM_ERR_INVALID, w + ": missing keypoint array");
  for (int i = 0; i < k.n; i++)
    if ((uint32_t)k.kps[i].octave >= (uint32_t)k.n_levels) return fail(fn, DVM_ERR_INVALID, w + ": a keypoint's octave outside the level tables");
  if (k.fv_n < 0) return fail(fn, DVM_ERR_INVALID, w + ": negative fv_n");
  if (k.fv_n > K) return fail(fn, DVM_ERR_CAPACITY, w + ": " + std::to_string(k.fv_n) + " FeatureVector nodes beyond slot_keypoints " + std::to_string(K));
  if (k.fv_n > k.n) return fail(fn, DVM_ERR_INVALID, w + ": more FeatureVector nodes than keypoints");
  if (k.fv_n > 0) {
    if (!k.fv_node || !k.fv_off || !k.fv_feat) return fail(fn, DVM_ERR_INVALID, w + ": missing FeatureVector array");
    if (k.fv_off[0] != 0) return fail(fn, DVM_ERR_INVALID, w + ": FeatureVector offsets do not start at 0");
    for (int a = 0; a < k.fv_n; a++) {
      if (k.fv_off[a + 1] < k.fv_off[a]) return fail(fn, DVM_ERR_INVALID, w + ": FeatureVector offsets not monotone");
      if (a > 0 && (uint32_t)k.fv_node[a] <= (uint32_t)k.fv_node[a - 1])
        return fail(fn, DVM_ERR_INVALID, w + ": FeatureVector nodes not ascending (as unsigned: node -1 is last)");
    }
    const int nf = k.fv_off[k.fv_n];
    if (nf > k.n) return fail(fn, DVM_ERR_INVALID, w + ": more FeatureVector features than keypoints");
    for (int f = 0; f < nf; f++)
      if (k.fv_feat[f] < 0 || k.fv_feat[f] >= k.n) return fail(fn, DVM_ERR_INVALID, w + ": FeatureVector feature index out of range");
  }
  return DVM_OK;
}
}  // namespace

extern "C" {

int dvm_keyframe_store_create(int device, int capacity, int slot_keypoints, dvm_keyframe_store** out) {
  static_assert(sizeof(dvm_keypoint) == kKfsKeypointBytes && sizeof(dvm_keypoint_pod) == kKfsKeypointBytes, "layout");
  static_assert(kCellStartStride == (int)kKfsCellStart, "layout");
  const char* fn = "dvm_keyframe_store_create";
  if (!out) return DVM_ERR_INVALID;
  *out = nullptr;
  if (capacity < 1 || slot_keypoints < 1 || slot_keypoints > kFrameCap) return fail(fn, DVM_ERR_INVALID, "capacity < 1 or slot_keypoints outside [1, 8192]");
  { const int rc = need_device(device); if (rc != DVM_OK) return rc; }
  dvm_keyframe_store* st = new (std::nothrow) dvm_keyframe_store();
  if (!st) return DVM_ERR_INVALID;
  st->device = device; st->capacity = capacity; st->K = slot_keypoints;
  st->L = kf_slot_layout((size_t)slot_keypoints);
  const size_t C = (size_t)capacity, block = C * st->L.stride;
  st->item_bytes = pad<256>(C * sizeof(KfsPutItem));
  st->stage_bytes = st->item_bytes + (size_t)std::min(capacity, kStageKeyframes) * kf_stage_bytes_max((size_t)slot_keypoints);
  const char* what = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&st->d), block) != hipSuccess) { st->d = nullptr; what = "hipMalloc"; }
  else if (hipMalloc(reinterpret_cast<void**>(&st->ds), st->stage_bytes) != hipSuccess) { st->ds = nullptr; what = "hipMalloc of the staging twin"; }
  else if (hipHostMalloc(reinterpret_cast<void**>(&st->hs), st->stage_bytes, hipHostMallocDefault) != hipSuccess) { st->hs = nullptr; what = "page-locked staging"; }
  if (what) {
    (void)hipGetLastError();
    dvm_keyframe_store_destroy(st);
    return fail(fn, DVM_ERR_CAPACITY, std::string(what) + " (capacity " + std::to_string(capacity) + ", slot_keypoints " + std::to_string(slot_keypoints) + ")");
  }
  if (hipStreamCreateWithFlags(&st->s, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&st->write_ev, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&st->read_ev, hipEventDisableTiming) != hipSuccess || hipMemsetAsync(st->d, 0, block, st->s) != hipSuccess ||
      hipStreamSynchronize(st->s) != hipSuccess) {
    dvm_keyframe_store_destroy(st);
    return fail(fn, DVM_ERR_HIP, "stream, events or clearing the slots");
  }
  st->meta.assign(C, SlotMeta()); st->stamp.assign(C, 0); st->seen.assign((size_t)slot_keypoints, 0);
  *out = st;
  return DVM_OK;
}

void dvm_keyframe_store_destroy(dvm_keyframe_store* st) {
  if (!st) return;
  (void)hipSetDevice(st->device);
  if (st->s) (void)hipStreamSynchronize(st->s);
  if (st->read_pending && st->read_ev) (void)hipEventSynchronize(st->read_ev);   // a chain still reading the slots
  if (st->s) (void)hipStreamDestroy(st->s);
  if (st->write_ev) (void)hipEventDestroy(st->write_ev);
  if (st->read_ev) (void)hipEventDestroy(st->read_ev);
  if (st->d) (void)hipFree(st->d);
  if (st->ds) (void)hipFree(st->ds);
  if (st->hs) (void)hipHostFree(st->hs);
  delete st;
}

int dvm_keyframe_store_capacity(const dvm_keyframe_store* st) { return st ? st->capacity : DVM_ERR_INVALID; }
int dvm_keyframe_store_slot_keypoints(const dvm_keyframe_store* st) { return st ? st->K : DVM_ERR_INVALID; }

int dvm_keyframe_store_put(dvm_keyframe_store* st, int n, const int32_t* slots, const dvm_kfs_keyframe* kfs) {
  const char* fn = "dvm_keyframe_store_put";
  if (!st || n < 0 || (n && (!slots || !kfs))) return fail(fn, DVM_ERR_INVALID, "missing argument");
  if (n == 0) return DVM_OK;
  // the whole batch is decided before anything is staged or queued
  if (++st->call == 0) { std::fill(st->stamp.begin(), st->stamp.end(), 0u); st->call = 1; }
  for (int k = 0; k < n; k++) {
    const int32_t sl = slots[k];
    const std::string w = "keyframe " + std::to_string(k) + " (slot " + std::to_string(sl) + ")";
    if (sl < 0 || sl >= st->capacity) return fail(fn, DVM_ERR_INVALID, w + ": slot outside [0, capacity)");
    if (st->stamp[sl] == st->call) return fail(fn, DVM_ERR_INVALID, w + ": slot named twice in one call");
    st->stamp[sl] = st->call;
    const int rc = check_keyframe(fn, kfs[k], w, st->K);
    if (rc != DVM_OK) return rc;
  }
  DVM_HIP(hipSetDevice(st->device));
  KfsPutItem* items = reinterpret_cast<KfsPutItem*>(st->hs);
  for (int done = 0; done < n;) {
    { const int rc = st->staging_free(); if (rc != DVM_OK) return rc; }
    Cursor<kKfsAlign> c{st->hs, st->ds, st->item_bytes};
    int m = 0;
    for (; done + m < n; m++) {
      const dvm_kfs_keyframe& k = kfs[done + m];
      const size_t nf = k.fv_n > 0 ? (size_t)k.fv_off[k.fv_n] : 0, nl = (size_t)k.n_levels;
      if (c.used() + kf_stage_bytes((size_t)k.n, (size_t)k.fv_n, nf, nl) > st->stage_bytes) break;   // (the first of a round always fits)
      KfsPutItem& it = items[m];
      it.src = c.put(k.kps, (size_t)k.n * kKfsKeypointBytes);
      c.put(k.desc, (size_t)k.n * 32);
      c.put(k.fv_node, (size_t)k.fv_n * 4);
      c.put(k.fv_off, k.fv_n > 0 ? ((size_t)k.fv_n + 1) * 4 : 0);
      c.put(k.fv_feat, nf * 4);
      c.put(k.scale_factors, nl * 4);
      c.put(k.level_sigma2, nl * 4);
      c.put(k.inv_level_sigma2, nl * 4);
      it.slot = st->slot_base(slots[done + m]);
      it.n = k.n; it.fv_n = k.fv_n; it.n_feat = (int32_t)nf; it.n_levels = k.n_levels;
      it.minX = k.min_x; it.minY = k.min_y;
      it.wInv = static_cast<float>(64) / static_cast<float>(k.max_x - k.min_x);   // Frame.cc:443-444, as dvm_frame_build
      it.hInv = static_cast<float>(48) / static_cast<float>(k.max_y - k.min_y);
    }
    if (m == 0) return fail(fn, DVM_ERR_STATE, "a keyframe exceeds the staging block");   // (an internal error: kf_stage_bytes_max bounds every keyframe)
    if (st->read_pending) {                                        // behind the chain kernels that read the slots
      DVM_HIP(hipStreamWaitEvent(st->s, st->read_ev, 0));
      st->read_pending = false;
    }
    // the items and the arrays in one copy (the gap between them, when the batch is smaller than the capacity, travels too: at most 48 B per slot)
    DVM_HIP(hipMemcpyAsync(st->ds, st->hs, c.used(), hipMemcpyHostToDevice, st->s));
    launch_kfs_put(st->s, reinterpret_cast<const KfsPutItem*>(st->ds), m, st->L);
    { const int rc = hip_check(hipGetLastError(), "k_kfs_put"); if (rc != DVM_OK) return rc; }
    DVM_HIP(hipEventRecord(st->write_ev, st->s));
    st->write_pending = true;
    for (int k = done; k < done + m; k++) {
      const dvm_kfs_keyframe& f = kfs[k];
      SlotMeta& M = st->meta[slots[k]];
      M.written = 1; M.gen++;
      M.n = f.n; M.fv_n = f.fv_n; M.n_feat = f.fv_n > 0 ? f.fv_off[f.fv_n] : 0; M.n_levels = f.n_levels;
      // put accepts a feature listed in two nodes (Fuse and CreateNewMapPoints do not mind); the slot remembers it for the chain that does
      M.fv_once = fv_first_repeat(f.fv_feat, M.n_feat, f.n, st->seen.data()) < 0;
      M.fx = f.fx; M.fy = f.fy; M.cx = f.cx; M.cy = f.cy;
      M.min_x = f.min_x; M.max_x = f.max_x; M.min_y = f.min_y; M.max_y = f.max_y; M.log_scale_factor = f.log_scale_factor;
    }
    done += m;
  }
  return DVM_OK;
}

int dvm_keyframe_store_remove(dvm_keyframe_store* st, int n, const int32_t* slots) {
  const char* fn = "dvm_keyframe_store_remove";
  if (!st || n < 0 || (n && !slots)) return fail(fn, DVM_ERR_INVALID, "missing argument");
  for (int k = 0; k < n; k++)
    if ((uint32_t)slots[k] >= (uint32_t)st->capacity || !st->meta[slots[k]].written)
      return fail(fn, DVM_ERR_INVALID, "slot " + std::to_string(slots[k]) + " outside [0, capacity) or not written");
  for (int k = 0; k < n; k++) {
    SlotMeta& M = st->meta[slots[k]];
    if (M.written) { M.written = 0; M.gen++; }
  }
  return DVM_OK;
}

int dvm_keyframe_store_debug_read(dvm_keyframe_store* st, int slot, dvm_kfs_readback* out) {
  const char* fn = "dvm_keyframe_store_debug_read";
  if (!st || !out) return fail(fn, DVM_ERR_INVALID, "missing argument");
  if ((uint32_t)slot >= (uint32_t)st->capacity || !st->meta[slot].written)
    return fail(fn, DVM_ERR_INVALID, "slot " + std::to_string(slot) + " outside [0, capacity) or not written");
  DVM_HIP(hipSetDevice(st->device));
  DVM_HIP(hipStreamSynchronize(st->s));
  st->write_pending = false;
  std::vector<uint8_t> h(st->L.stride);
  DVM_HIP(hipMemcpy(h.data(), st->slot_base(slot), st->L.stride, hipMemcpyDeviceToHost));
  const SlotMeta& M = st->meta[slot];
  const KfSlotLayout& L = st->L;
  const int32_t* cnt = reinterpret_cast<const int32_t*>(h.data() + L.counters);
  out->n = M.n; out->fv_n = M.fv_n; out->n_feat = M.n_feat; out->n_levels = M.n_levels;
  out->n_sorted = cnt[0]; out->n_total = cnt[1];
  out->fx = M.fx; out->fy = M.fy; out->cx = M.cx; out->cy = M.cy;
  out->min_x = M.min_x; out->max_x = M.max_x; out->min_y = M.min_y; out->max_y = M.max_y; out->log_scale_factor = M.log_scale_factor;
  out->generation = M.gen;
  if (cnt[0] < 0 || cnt[0] > M.n) return fail(fn, DVM_ERR_STATE, "the slot's grid counter lies outside [0, n]");
  const size_t n = (size_t)M.n, ns = (size_t)cnt[0];
  auto give = [&](void* dst, size_t at, size_t bytes) { if (dst && bytes) std::memcpy(dst, h.data() + at, bytes); };
  give(out->kps, L.kps, n * kKfsKeypointBytes);
  give(out->desc, L.desc, n * 32);
  give(out->fv_node, L.fv_node, (size_t)M.fv_n * 4);
  give(out->fv_off, L.fv_off, M.fv_n > 0 ? ((size_t)M.fv_n + 1) * 4 : 0);
  give(out->fv_feat, L.fv_feat, (size_t)M.n_feat * 4);
  give(out->scale_factors, L.sf, (size_t)M.n_levels * 4);
  give(out->level_sigma2, L.sigma2, (size_t)M.n_levels * 4);
  give(out->inv_level_sigma2, L.inv_sigma2, (size_t)M.n_levels * 4);
  give(out->skp, L.skp, ns * 16);
  give(out->sidx, L.sidx, ns * 4);
  give(out->sdesc, L.sdesc, ns * 32);
  give(out->cell_start, L.cell_start, kKfsCellStart * 4);
  return DVM_OK;
}

}  // extern "C"
