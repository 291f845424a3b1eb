// dvm_slam_amd/csrc/map_store.cpp -- dvm_map_store (include/dvmslam_hip.h): an agent's map points resident on the device.
//
// The records (dvm_local_point, 72 B) live in one device block of `capacity` slots that never moves.  LocalMapping writes a point after
// a local BA, a fuse or a culling step (the reference holds Map::mMutexMapUpdate around those writes); the tracked frame reads it at
// camera rate (dvm_track_finish_batch_resident, dvm_track_local_map_batch_resident in track.cpp).
//
// Ordering -- the store's own stream plus two events:
//   update   copies slots and records into the store's page-locked staging block (mapped: k_store_scatter reads it in place), makes the
//            store's stream wait for `read_ev` (the last kernel a chain queued to read the store), launches the scatter there and records
//            `write_ev`.  It returns without waiting; the next update (or read) waits on the host for `write_ev` before it touches the
//            staging block again.
//   a chain  store_read_begin: its stream waits for `write_ev`; store_read_end: `read_ev` recorded behind its reading kernels.
// So a reader always sees every update queued before it, and an update never overtakes a reader in flight.
//   refresh  (dvm_map_store_refresh) writes records in place from the keyframe store's descriptors: on the calling thread's staging stream
//            (host_stage.h), which waits for `read_ev` AND `write_ev` -- it is a writer behind every reader and every earlier writer --,
//            bracketed as a reader of the keyframe store; it records `write_ev` behind its launch and synchronises once, so whatever
//            follows it, on any stream, sees its records.
// Safety: the host keeps a written flag per slot; every slot a call names is checked against capacity and that flag BEFORE anything is
// queued, so no kernel indexes the store with an unchecked value.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/dvmslam_hip.h"
#include "chain.h"
#include "fuse_points_lists.h"
#include "host_stage.h"
#include "keyframe_store.h"
#include "map_refresh_lists.h"
#include "map_store.h"

using namespace dvm;

struct dvm_map_store {
  int device = 0, capacity = 0;
  LocalPointPod* d = nullptr;                      // [capacity]
  uint8_t *hm = nullptr, *hm_dev = nullptr;        // staging, page-locked and mapped: [capacity] slots, [capacity] records
  hipStream_t s = nullptr;
  hipEvent_t write_ev = nullptr, read_ev = nullptr;
  bool write_pending = false, read_pending = false;
  std::vector<uint8_t> written;                    // per slot: an update has named it
  std::vector<uint32_t> stamp; uint32_t gen = 0;   // per slot: the update call that named it last (a slot named twice in one call)
  int32_t* stage_slots() const { return reinterpret_cast<int32_t*>(hm); }
  LocalPointPod* stage_recs() const { return reinterpret_cast<LocalPointPod*>(hm + pad<256>((size_t)capacity * 4)); }
  template <class T> T* dev(T* p) const { return rebase(p, hm, hm_dev); }
  // the staging block is the host's again: the last scatter has read it
  int staging_free() {
    if (write_pending) { DVM_HIP(hipEventSynchronize(write_ev)); write_pending = false; }
    return DVM_OK;
  }
  // dvm_map_store_refresh: what the last one moved, its kernel's time when profiling, the call's keyframe table as the kernel takes it
  int64_t refresh_h2d = 0, refresh_d2h = 0;
  EventTimer timer; float refresh_ms = 0.f;
  std::vector<MprKfMeta> kf_meta; std::vector<MprKfDev> kf_dev;
};

namespace dvm {
const LocalPointPod* store_records(const dvm_map_store* st) { return st->d; }
int store_device(const dvm_map_store* st) { return st->device; }
const uint8_t* store_written(const dvm_map_store* st) { return st->written.data(); }
bool store_slots_ok(const dvm_map_store* st, const int32_t* slots, int n) {
  const uint32_t cap = (uint32_t)st->capacity;
  const uint8_t* w = st->written.data();
  for (int k = 0; k < n; k++)
    if ((uint32_t)slots[k] >= cap || !w[slots[k]]) return false;
  return true;
}
int store_kf_slots_check(const dvm_map_store* st, const int32_t* slots, int n, bool* any) {
  return fpl_slots_check(FplStore{st ? st->capacity : -1, st ? st->written.data() : nullptr}, slots, n, any);
}
int store_read_begin(const dvm_map_store* cst, hipStream_t s) {
  dvm_map_store* st = const_cast<dvm_map_store*>(cst);
  if (!st->write_pending) return DVM_OK;
  // (an update that has run needs no wait, now or later: a map point is written rarely and read at camera rate)
  if (hipEventQuery(st->write_ev) == hipSuccess) { st->write_pending = false; return DVM_OK; }
  (void)hipGetLastError();     // hipErrorNotReady is no error
  DVM_HIP(hipStreamWaitEvent(s, st->write_ev, 0));
  return DVM_OK;
}
int store_read_end(const dvm_map_store* cst, hipStream_t s) {
  dvm_map_store* st = const_cast<dvm_map_store*>(cst);
  DVM_HIP(hipEventRecord(st->read_ev, s));
  st->read_pending = true;
  return DVM_OK;
}
int store_commit_geometry(dvm_map_store* st, const StoreCommitRange* ranges, int n, hipEvent_t done) {
  DVM_HIP(hipSetDevice(st->device));
  if (st->read_pending) {                                        // behind the chain kernels that read the records, as an update
    DVM_HIP(hipStreamWaitEvent(st->s, st->read_ev, 0));
    st->read_pending = false;
  }
  for (int first = 0; first < n; first += kStoreCommitRanges) {
    const int m = std::min(kStoreCommitRanges, n - first);
    StoreCommit C;
    std::memset(&C, 0, sizeof(C));
    int span = 0;
    for (int i = 0; i < m; i++) { C.r[i] = ranges[first + i]; span = std::max(span, (int)ranges[first + i].n); }
    launch_store_commit(st->s, st->d, C, m, span);
    { const int rc = hip_check(hipGetLastError(), "k_store_commit"); if (rc != DVM_OK) return rc; }
  }
  DVM_HIP(hipEventRecord(st->write_ev, st->s));
  st->write_pending = true;
  DVM_HIP(hipEventRecord(done, st->s));
  return DVM_OK;
}
}  // namespace dvm

extern "C" {

int dvm_map_store_create(int device, int capacity, dvm_map_store** out) {
  if (!out) return DVM_ERR_INVALID;
  *out = nullptr;
  if (capacity < 1) return DVM_ERR_INVALID;
  { const int rc = need_device(device); if (rc != DVM_OK) return rc; }
  dvm_map_store* st = new (std::nothrow) dvm_map_store();
  if (!st) return DVM_ERR_INVALID;
  st->device = device; st->capacity = capacity;
  const size_t C = (size_t)capacity;
  const size_t hbytes = pad<256>(C * 4) + pad<256>(C * sizeof(LocalPointPod));
  const char* what = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&st->d), C * sizeof(LocalPointPod)) != hipSuccess) { st->d = nullptr; what = "hipMalloc"; }
  else if (hipHostMalloc(reinterpret_cast<void**>(&st->hm), hbytes, hipHostMallocMapped) != hipSuccess) { st->hm = nullptr; what = "page-locked staging"; }
  else if (hipHostGetDevicePointer(reinterpret_cast<void**>(&st->hm_dev), st->hm, 0) != hipSuccess) what = "page-locked staging";
  if (what) {
    (void)hipGetLastError();
    dvm_map_store_destroy(st);
    set_error(std::string("dvm_map_store_create: ") + what + " (capacity " + std::to_string(capacity) + ")");
    return DVM_ERR_CAPACITY;
  }
  if (hipStreamCreateWithFlags(&st->s, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&st->write_ev, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&st->read_ev, hipEventDisableTiming) != hipSuccess || hipMemsetAsync(st->d, 0, C * sizeof(LocalPointPod), st->s) != hipSuccess ||
      hipStreamSynchronize(st->s) != hipSuccess) {
    dvm_map_store_destroy(st); set_error("dvm_map_store_create: stream, events or clearing the records"); return DVM_ERR_HIP;
  }
  st->written.assign(C, 0); st->stamp.assign(C, 0);
  *out = st;
  return DVM_OK;
}

void dvm_map_store_destroy(dvm_map_store* st) {
  if (!st) return;
  (void)hipSetDevice(st->device);
  if (st->s) { (void)hipStreamSynchronize(st->s); }
  if (st->read_pending && st->read_ev) (void)hipEventSynchronize(st->read_ev);   // a chain still reading the records
  if (st->s) (void)hipStreamDestroy(st->s);
  if (st->write_ev) (void)hipEventDestroy(st->write_ev);
  if (st->read_ev) (void)hipEventDestroy(st->read_ev);
  st->timer.destroy();
  if (st->d) (void)hipFree(st->d);
  if (st->hm) (void)hipHostFree(st->hm);
  delete st;
}

int dvm_map_store_capacity(const dvm_map_store* st) { return st ? st->capacity : DVM_ERR_INVALID; }

int dvm_map_store_update(dvm_map_store* st, int n, const int32_t* slots, const dvm_local_point* records) {
  if (!st || n < 0 || (n && (!slots || !records))) return DVM_ERR_INVALID;
  if (n == 0) return DVM_OK;
  // every slot in range and named once: decided before anything is staged or queued
  if (++st->gen == 0) { std::fill(st->stamp.begin(), st->stamp.end(), 0u); st->gen = 1; }
  for (int k = 0; k < n; k++) {
    const int32_t sl = slots[k];
    if (sl < 0 || sl >= st->capacity) { set_error("dvm_map_store_update: slot " + std::to_string(sl) + " outside [0, capacity)"); return DVM_ERR_INVALID; }
    if (st->stamp[sl] == st->gen) { set_error("dvm_map_store_update: slot " + std::to_string(sl) + " named twice in one call"); return DVM_ERR_INVALID; }
    st->stamp[sl] = st->gen;
  }
  DVM_HIP(hipSetDevice(st->device));
  { const int rc = st->staging_free(); if (rc != DVM_OK) return rc; }
  std::memcpy(st->stage_slots(), slots, (size_t)n * 4);          // (n <= capacity: every slot once)
  std::memcpy(st->stage_recs(), records, (size_t)n * sizeof(LocalPointPod));
  if (st->read_pending) {                                        // behind the chain kernels that read the records
    DVM_HIP(hipStreamWaitEvent(st->s, st->read_ev, 0));
    st->read_pending = false;
  }
  launch_store_scatter(st->s, st->d, st->dev(st->stage_slots()), st->dev(st->stage_recs()), n);
  { const int rc = hip_check(hipGetLastError(), "k_store_scatter"); if (rc != DVM_OK) return rc; }
  DVM_HIP(hipEventRecord(st->write_ev, st->s));
  st->write_pending = true;
  for (int k = 0; k < n; k++) st->written[slots[k]] = 1;
  return DVM_OK;
}

int dvm_map_store_read(dvm_map_store* st, int n, const int32_t* slots, dvm_local_point* out) {
  if (!st || n < 0 || (n && (!slots || !out))) return DVM_ERR_INVALID;
  if (n == 0) return DVM_OK;
  if (!store_slots_ok(st, slots, n)) { set_error("dvm_map_store_read: a slot outside [0, capacity) or never written"); return DVM_ERR_INVALID; }
  DVM_HIP(hipSetDevice(st->device));
  { const int rc = st->staging_free(); if (rc != DVM_OK) return rc; }
  // through the staging block, `capacity` slots at a time (a slot may repeat: n is not bounded by the capacity)
  for (int done = 0; done < n; done += st->capacity) {
    const int m = std::min(st->capacity, n - done);
    std::memcpy(st->stage_slots(), slots + done, (size_t)m * 4);
    launch_store_read(st->s, st->d, st->dev(st->stage_slots()), st->dev(st->stage_recs()), m);
    { const int rc = hip_check(hipGetLastError(), "k_store_read"); if (rc != DVM_OK) return rc; }
    DVM_HIP(hipStreamSynchronize(st->s));
    std::memcpy(out + done, st->stage_recs(), (size_t)m * sizeof(LocalPointPod));
  }
  return DVM_OK;
}

int dvm_map_store_refresh(dvm_map_store* st, const dvm_keyframe_store* ks, const dvm_mp_refresh* in) {
  static const char* fn = "dvm_map_store_refresh: ";
  auto refuse = [&](int rc, const std::string& msg) { set_error(fn + msg); return rc; };
  if (!st || !ks || !in) return refuse(DVM_ERR_INVALID, "missing argument");
  {
    const MprVerdict v = mpr_check_args(*in);
    if (v.fault == kMprCounts) return refuse(DVM_ERR_INVALID, "a negative count");
    if (v.fault == kMprWhat) return refuse(DVM_ERR_INVALID, "what = " + std::to_string(in->what) + ": not DESCRIPTOR, GEOMETRY or both");
    if (v.fault != kMprOk) return refuse(DVM_ERR_INVALID, "a required array is NULL (ref_obs with GEOMETRY; is_new and new_pos come together)");
  }
  if (kfs_device(ks) != st->device) return refuse(DVM_ERR_INVALID, "the keyframe store lives on another device");
  const int L = in->n_points, K = in->n_kfs;
  // what the keyframe store knows of every entry, then every list: decided before anything is queued
  st->kf_meta.assign((size_t)K, MprKfMeta{-1, 0});
  st->kf_dev.resize((size_t)K);
  for (int k = 0; k < K; k++) {
    const dvm_mp_refresh_kf& f = in->kfs[k];
    KfSlotView v;
    if (f.slot >= 0 && kfs_slot_view(ks, f.slot, &v)) st->kf_meta[k] = MprKfMeta{v.n, v.n_levels};
    MprKfDev& d = st->kf_dev[k];
    d.slot = f.slot; d.fl = (f.flags & DVM_MPR_KF_BAD) | ((uint32_t)st->kf_meta[k].n_levels << 8);
    d.ow[0] = f.ow[0]; d.ow[1] = f.ow[1]; d.ow[2] = f.ow[2];
  }
  if (++st->gen == 0) { std::fill(st->stamp.begin(), st->stamp.end(), 0u); st->gen = 1; }
  const MprVerdict v = mpr_check_lists(*in, st->capacity, st->written.data(), st->stamp.data(), st->gen, st->kf_meta.data());
  if (v.fault != kMprOk) {
    const std::string pt = v.point >= 0 ? "point " + std::to_string(v.point) + (v.point < L ? " (slot " + std::to_string(in->mp_slot[v.point]) + ")" : std::string()) : std::string();
    const std::string kf = v.kf >= 0 ? "keyframe " + std::to_string(v.kf) + " (slot " + std::to_string(in->kfs[v.kf].slot) + ")" : std::string();
    const std::string ob = v.obs >= 0 ? ", observation " + std::to_string(v.obs - in->obs_off[v.point]) : std::string();
    switch (v.fault) {
      case kMprOff: return refuse(v.rc(), "obs_off not monotone from 0 to n_obs at entry " + std::to_string(v.point));
      case kMprKfFlags: return refuse(v.rc(), kf + ": unknown flags");
      case kMprKfSlot: return refuse(v.rc(), kf + ": slot outside the keyframe store, never written or removed");
      case kMprMapSlot: return refuse(v.rc(), pt + ": slot outside [0, capacity)");
      case kMprMapTwice: return refuse(v.rc(), pt + ": slot named twice in one call");
      case kMprUnwritten: return refuse(v.rc(), pt + ": an old point whose slot was never written");
      case kMprNewEmpty: return refuse(v.rc(), pt + ": a new point without observations");
      case kMprNewWhat: return refuse(v.rc(), pt + ": a new point needs what = DESCRIPTOR | GEOMETRY");
      case kMprTooMany: return refuse(v.rc(), pt + ": more than " + std::to_string(kMprMaxObs) + " observations");
      case kMprObsKf: return refuse(v.rc(), pt + ob + ": kf outside [0, n_kfs)");
      case kMprKp: return refuse(v.rc(), pt + ob + ": kp outside [0, n) of " + kf);
      case kMprRef: return refuse(v.rc(), pt + ": ref_obs outside [0, N)");
      default: return refuse(v.rc(), pt + ": the ref observation lies on " + kf + ", a bad keyframe without a slot");
    }
  }
  st->refresh_h2d = st->refresh_d2h = 0; st->refresh_ms = 0.f;
  if (L == 0) return DVM_OK;
  DVM_HIP(hipSetDevice(st->device));
  // one upload; the outputs are written by the kernel into page-locked memory (each entry once: nothing but the results comes down)
  Stage stg;
  const size_t l = (size_t)L;
  const int i_slot = stg.in(in->mp_slot, 4 * l), i_off = stg.in(in->obs_off, 4 * (l + 1)), i_obs = stg.in(in->obs, sizeof(dvm_mp_obs) * (size_t)in->n_obs);
  const int i_ref = stg.in(in->ref_obs, 4 * l), i_kf = stg.in(K ? st->kf_dev.data() : nullptr, sizeof(MprKfDev) * (size_t)K);
  const int i_new = stg.in(in->is_new, l), i_pos = stg.in(in->new_pos, 12 * l);
  const int o_best = stg.out_mapped(in->best_obs_out, 4 * l), o_med = stg.out_mapped(in->best_median_out, 4 * l), o_geo = stg.out_mapped(in->geometry_out, 32 * l);
  { const int rc = stg.upload(); if (rc != DVM_OK) return rc; }
  hipStream_t s = stg.stream();
  if (st->read_pending) {                                          // a writer: behind the chain kernels that read the records ...
    DVM_HIP(hipStreamWaitEvent(s, st->read_ev, 0));
    st->read_pending = false;
  }
  { const int rc = store_read_begin(st, s); if (rc != DVM_OK) return rc; }     // ... and behind the last update or commit
  { const int rc = kfs_read_begin(ks, s); if (rc != DVM_OK) return rc; }       // a reader of the keyframe slots
  const KfsBlockView B = kfs_block_view(ks);
  MprArgs A;
  std::memset(&A, 0, sizeof(A));
  A.records = st->d;
  A.kf_base = B.base; A.kf_stride = B.stride; A.kf_kps = B.kps; A.kf_desc = B.desc; A.kf_sf = B.sf;
  A.mp_slot = stg.ptr<int32_t>(i_slot); A.obs_off = stg.ptr<int32_t>(i_off); A.obs = stg.ptr<dvm_mp_obs>(i_obs); A.ref_obs = stg.ptr<int32_t>(i_ref);
  A.kfs = stg.ptr<MprKfDev>(i_kf); A.is_new = stg.ptr<uint8_t>(i_new); A.new_pos = stg.ptr<float>(i_pos);
  A.best_obs_out = stg.ptr<int32_t>(o_best); A.best_median_out = stg.ptr<int32_t>(o_med); A.geometry_out = stg.ptr<float>(o_geo);
  A.n_points = L; A.what = in->what;
  DVM_HIP(st->timer.mark(0, s));
  launch_mp_refresh(s, A, v.max_obs > 64);
  { const int rc = hip_check(hipGetLastError(), "k_mp_refresh"); if (rc != DVM_OK) return rc; }
  DVM_HIP(st->timer.mark(1, s));
  { const int rc = kfs_read_end(ks, s); if (rc != DVM_OK) return rc; }
  DVM_HIP(hipEventRecord(st->write_ev, s));
  st->write_pending = true;
  // the ONE synchronisation: the outputs lie in page-locked memory behind it
  { const int rc = stg.download(); if (rc != DVM_OK) return rc; }
  st->write_pending = false;
  if (in->is_new)
    for (int p = 0; p < L; p++) if (in->is_new[p]) st->written[in->mp_slot[p]] = 1;
  st->refresh_h2d = (int64_t)stg.in_bytes;
  st->refresh_d2h = (int64_t)(4 * l) * (1 + (in->best_median_out ? 1 : 0) + (in->geometry_out ? 8 : 0));
  if (st->timer.on) DVM_HIP(st->timer.elapsed(0, 1, &st->refresh_ms));
  return DVM_OK;
}

int dvm_map_store_last_refresh_bytes(const dvm_map_store* st, int64_t* host_to_device, int64_t* device_to_host) {
  if (!st || !host_to_device || !device_to_host) return DVM_ERR_INVALID;
  *host_to_device = st->refresh_h2d; *device_to_host = st->refresh_d2h;
  return DVM_OK;
}

int dvm_map_store_profile(dvm_map_store* st, int enable) {
  if (!st) return DVM_ERR_INVALID;
  DVM_HIP(hipSetDevice(st->device));
  return st->timer.enable(enable != 0);
}

int dvm_map_store_last_refresh_ms(const dvm_map_store* st, float* kernel_ms) {
  if (!st || !kernel_ms) return DVM_ERR_INVALID;
  *kernel_ms = st->refresh_ms;
  return DVM_OK;
}

}  // extern "C"
