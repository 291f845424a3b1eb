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
// Safety: the host keeps a written flag per slot; every slot a call names is checked against capacity and that flag BEFORE anything is
// queued, so no kernel indexes the store with an unchecked value.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/dvmslam_hip.h"
#include "chain.h"
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
};

namespace dvm {
const LocalPointPod* store_records(const dvm_map_store* st) { return st->d; }
int store_device(const dvm_map_store* st) { return st->device; }
bool store_slots_ok(const dvm_map_store* st, const int32_t* slots, int n) {
  const uint32_t cap = (uint32_t)st->capacity;
  const uint8_t* w = st->written.data();
  for (int k = 0; k < n; k++)
    if ((uint32_t)slots[k] >= cap || !w[slots[k]]) return false;
  return true;
}
int store_kf_slots_check(const dvm_map_store* st, const int32_t* slots, int n, bool* any) {
  bool some = false;
  int rc = 0;
  for (int k = 0; k < n && !rc; k++) {
    const int32_t sl = slots[k];
    if (sl == -1) continue;
    some = true;
    if (sl < 0) rc = 1;
    else if (!st) rc = 2;
    else if (sl >= st->capacity || !st->written[sl]) rc = 1;
  }
  if (any) *any = some;
  return rc;
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

}  // extern "C"
