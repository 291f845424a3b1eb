// dvm_slam_amd/csrc/fuse_points_lists.h -- host side of the Fuse runs on points named as map-store slots (fuse_targets.cpp:
// dvm_fuse_targets_run[_hits]_resident, dvm_fuse_targets_run_hits_candidates): every check of the call's arguments and slot lists, decided
// before anything is queued, so that k_ft_gather and the k_ft_cand_* kernels (fuse_targets_kernels.hip) index with checked values only.
// Pure host code, no HIP: tools/check_fuse_points_lists.cpp walks it under the sanitizers (tests/test_fuse_points_lists.py).
//   fpl_slots_check       a slot list: every entry -1 or a written slot of the store (store_kf_slots_check of map_store.h is this function)
//   fpl_check_points      a dvm_ft_points_resident against the handle's reservation and the store
//   fpl_check_candidates  a dvm_ft_candidates against the two reservations and the store; the flat length of its lists
//   fpl_flatten           the lists back to back, in (list, keypoint) order: what travels up
// The first offence in the order of the code below is the one reported.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/dvmslam_hip.h"

namespace dvm {

// what a check knows of the map store a call names: capacity = -1 for a NULL store (written is then not read)
struct FplStore { int32_t capacity; const uint8_t* written; };

enum FplFault {
  kFplOk = 0,
  kFplNull,          // a required array is NULL
  kFplCount,         // a negative count
  kFplPoints,        // more rows than max_points of dvm_fuse_targets_reserve: DVM_ERR_CAPACITY
  kFplEntries,       // more entries than max_entries of dvm_fuse_targets_reserve_candidates: DVM_ERR_CAPACITY
  kFplTable,         // the store holds more slots than map_capacity of dvm_fuse_targets_reserve_candidates: DVM_ERR_CAPACITY
  kFplSlot,          // a slot below -1, outside [0, capacity) or never written         (list, at)
  kFplNoStore,       // a NULL store where a slot names a point                          (list, at)
};
struct FplVerdict {
  int fault = kFplOk;
  int list = -1, at = -1;        // what the fault names: the list (n_lists: the exclude list) and the entry inside it
  int64_t total = 0;             // the flat length of a candidates call's lists (valid when fault == kFplOk)
  int rc() const { return fault == kFplOk ? DVM_OK : fault == kFplPoints || fault == kFplEntries || fault == kFplTable ? DVM_ERR_CAPACITY : DVM_ERR_INVALID; }
};
inline FplVerdict fpl_fail(int fault, int list = -1, int at = -1) {
  FplVerdict v;
  v.fault = fault; v.list = list; v.at = at;
  return v;
}

// 0: every one of slots[0 .. n) is -1 or a written slot; 1: a slot below -1, outside [0, capacity) or never written; 2: no store and a
// slot names a point.  *any (may be NULL): a slot >= 0 seen; *at (may be NULL): the offending entry
inline int fpl_slots_check(const FplStore& st, const int32_t* slots, int n, bool* any, int* at = nullptr) {
  bool some = false;
  int rc = 0, k = 0;
  for (; k < n && !rc; k++) {
    const int32_t sl = slots[k];
    if (sl == -1) continue;
    some = true;
    if (sl < 0) rc = 1;
    else if (st.capacity < 0) rc = 2;
    else if (sl >= st.capacity || !st.written[sl]) rc = 1;
  }
  if (any) *any = some;
  if (at && rc) *at = k - 1;
  return rc;
}

inline FplVerdict fpl_slot_list(const FplStore& st, const int32_t* slots, int n, int list) {
  int at = -1;
  const int rc = fpl_slots_check(st, slots, n, nullptr, &at);
  return rc == 0 ? FplVerdict{} : fpl_fail(rc == 2 ? kFplNoStore : kFplSlot, list, at);
}

inline FplVerdict fpl_check_points(const dvm_ft_points_resident& P, const FplStore& st, int max_points) {
  if (P.n < 0) return fpl_fail(kFplCount);
  if (P.n > max_points) return fpl_fail(kFplPoints);
  if (P.n > 0 && !P.slot) return fpl_fail(kFplNull);
  return fpl_slot_list(st, P.slot, P.n, 0);
}

// table_capacity: map_capacity of dvm_fuse_targets_reserve_candidates (the first-index table and the exclude marks are indexed by slot)
inline FplVerdict fpl_check_candidates(const dvm_ft_candidates& C, const FplStore& st, int max_points, int max_entries, int table_capacity) {
  if (C.n_lists < 0 || C.n_exclude < 0) return fpl_fail(kFplCount);
  if ((C.n_lists > 0 && (!C.mp_slot || !C.n)) || (C.n_exclude > 0 && !C.exclude)) return fpl_fail(kFplNull);
  int64_t total = 0;
  for (int l = 0; l < C.n_lists; l++) {
    if (C.n[l] < 0) return fpl_fail(kFplCount, l);
    if (C.n[l] > 0 && !C.mp_slot[l]) return fpl_fail(kFplNull, l);
    total += C.n[l];
  }
  if (total > max_points) return fpl_fail(kFplPoints);
  if (total > max_entries || C.n_exclude > max_entries) return fpl_fail(kFplEntries);
  if (st.capacity > table_capacity) return fpl_fail(kFplTable);
  for (int l = 0; l < C.n_lists; l++) {
    const FplVerdict v = fpl_slot_list(st, C.mp_slot[l], C.n[l], l);
    if (v.fault != kFplOk) return v;
  }
  FplVerdict v = fpl_slot_list(st, C.exclude, C.n_exclude, C.n_lists);
  v.total = total;
  return v;
}

// dst [total]: entry (l, k) at n[0] + .. + n[l - 1] + k (C passed fpl_check_candidates)
inline void fpl_flatten(const dvm_ft_candidates& C, int32_t* dst) {
  for (int l = 0; l < C.n_lists; l++) {
    if (C.n[l] > 0) std::memcpy(dst, C.mp_slot[l], (size_t)C.n[l] * 4);
    dst += C.n[l];
  }
}

}  // namespace dvm
