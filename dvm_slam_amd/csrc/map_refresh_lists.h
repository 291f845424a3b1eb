// dvm_slam_amd/csrc/map_refresh_lists.h -- host side of dvm_map_store_refresh (map_store.cpp): every check of the call's lists, decided
// before anything is queued, so that k_mp_refresh (map_refresh_kernels.hip) indexes with checked values only.  Pure host code, no HIP:
// tools/check_map_refresh_lists.cpp walks it under the sanitizers (tests/test_map_refresh_lists.py).
//   mpr_check_args    the call's own fields: required arrays, `what`, the counts
//   mpr_check_lists   the CSR, every map slot, every observation, every ref -- against what the entry knows of the two stores
// The first offence in the order of the code below is the one reported.
#pragma once
#include <cstdint>

#include "../../include/dvmslam_hip.h"

namespace dvm {

constexpr int kMprMaxObs = 512;                    // kDistinctMaxN (match_device.h): the LDS form's descriptor table

// what the entry knows of the call's keyframe entry k (kfs_slot_view): the slot's keypoint count and level count; n = -1 for a slot
// outside the store, never written or removed
struct MprKfMeta { int32_t n, n_levels; };

enum MprFault {
  kMprOk = 0,
  kMprNull,          // a required array is NULL, or exactly one of is_new / new_pos
  kMprWhat,          // what is 0 or has unknown bits
  kMprCounts,        // a negative count
  kMprOff,           // obs_off not monotone from 0 to n_obs                           (point: the first offending entry)
  kMprKfFlags,       // a keyframe entry with unknown flag bits                          (kf)
  kMprKfSlot,        // a keyframe slot outside the store, never written or removed      (kf)
  kMprMapSlot,       // a map slot outside [0, capacity)                                 (point)
  kMprMapTwice,      // a map slot named twice                                           (point)
  kMprUnwritten,     // an old point's slot never written                                (point)
  kMprNewEmpty,      // a new point without observations                                 (point)
  kMprNewWhat,       // a new point in a call that does not ask for both groups          (point)
  kMprTooMany,       // more than kMprMaxObs observations: DVM_ERR_CAPACITY              (point)
  kMprObsKf,         // an observation's kf outside [0, n_kfs)                           (point, obs)
  kMprKp,            // an observation's kp outside [0, n) of its slot                   (point, obs)
  kMprRef,           // ref_obs outside [0, N) on a point whose geometry is asked for    (point)
  kMprRefBad,        // the ref observation lies on a bad keyframe without a slot        (point)
};
struct MprVerdict {
  int fault = kMprOk;
  int point = -1, kf = -1, obs = -1;               // what the fault names (obs: the index in the call's obs array)
  int max_obs = 0;                                 // the longest list (valid when fault == kMprOk)
  int rc() const { return fault == kMprOk ? DVM_OK : fault == kMprTooMany ? DVM_ERR_CAPACITY : DVM_ERR_INVALID; }
};

inline MprVerdict mpr_fail(int fault, int point = -1, int kf = -1, int obs = -1) {
  MprVerdict v;
  v.fault = fault; v.point = point; v.kf = kf; v.obs = obs;
  return v;
}

inline MprVerdict mpr_check_args(const dvm_mp_refresh& in) {
  if (in.n_points < 0 || in.n_kfs < 0 || in.n_obs < 0) return mpr_fail(kMprCounts);
  if (in.what == 0u || (in.what & ~(uint32_t)(DVM_MPR_DESCRIPTOR | DVM_MPR_GEOMETRY)) != 0u) return mpr_fail(kMprWhat);
  if (!in.obs_off) return mpr_fail(kMprNull);
  if ((in.is_new == nullptr) != (in.new_pos == nullptr)) return mpr_fail(kMprNull);
  if (in.n_points > 0 && (!in.mp_slot || !in.best_obs_out || ((in.what & DVM_MPR_GEOMETRY) && !in.ref_obs))) return mpr_fail(kMprNull);
  if (in.n_obs > 0 && !in.obs) return mpr_fail(kMprNull);
  if (in.n_kfs > 0 && !in.kfs) return mpr_fail(kMprNull);
  return MprVerdict{};
}

// in: passed mpr_check_args.  written [map_capacity]: the map store's per-slot flags.  stamp [map_capacity] with `gen` a value no entry
// holds: scratch of the named-twice check (entries of named slots become gen).  meta [n_kfs].
inline MprVerdict mpr_check_lists(const dvm_mp_refresh& in, int map_capacity, const uint8_t* written, uint32_t* stamp, uint32_t gen, const MprKfMeta* meta) {
  const int L = in.n_points, E = in.n_obs, K = in.n_kfs;
  if (in.obs_off[0] != 0) return mpr_fail(kMprOff, 0);
  for (int p = 0; p < L; p++)
    if (in.obs_off[p + 1] < in.obs_off[p] || in.obs_off[p + 1] > E) return mpr_fail(kMprOff, p);
  if (in.obs_off[L] != E) return mpr_fail(kMprOff, L);
  for (int k = 0; k < K; k++) {
    const dvm_mp_refresh_kf& f = in.kfs[k];
    if (f.flags & ~(uint32_t)DVM_MPR_KF_BAD) return mpr_fail(kMprKfFlags, -1, k);
    if ((f.flags & DVM_MPR_KF_BAD) && f.slot == -1) continue;          // a bad keyframe that has left the store
    if (meta[k].n < 0) return mpr_fail(kMprKfSlot, -1, k);
  }
  const bool both = in.what == (DVM_MPR_DESCRIPTOR | DVM_MPR_GEOMETRY);
  int max_obs = 0;
  for (int p = 0; p < L; p++) {
    const int32_t sl = in.mp_slot[p];
    const int o0 = in.obs_off[p], N = in.obs_off[p + 1] - o0;
    const bool fresh = in.is_new && in.is_new[p];
    if (sl < 0 || sl >= map_capacity) return mpr_fail(kMprMapSlot, p);
    if (stamp[sl] == gen) return mpr_fail(kMprMapTwice, p);
    stamp[sl] = gen;
    if (!fresh && !written[sl]) return mpr_fail(kMprUnwritten, p);
    if (fresh && N == 0) return mpr_fail(kMprNewEmpty, p);
    if (fresh && !both) return mpr_fail(kMprNewWhat, p);
    if (N > kMprMaxObs) return mpr_fail(kMprTooMany, p);
    for (int j = 0; j < N; j++) {
      const dvm_mp_obs& ob = in.obs[o0 + j];
      if (ob.kf < 0 || ob.kf >= K) return mpr_fail(kMprObsKf, p, -1, o0 + j);
      const dvm_mp_refresh_kf& f = in.kfs[ob.kf];
      if ((f.flags & DVM_MPR_KF_BAD) && f.slot == -1) continue;        // no slot to check kp against
      if (ob.kp < 0 || ob.kp >= meta[ob.kf].n) return mpr_fail(kMprKp, p, ob.kf, o0 + j);
    }
    if ((in.what & DVM_MPR_GEOMETRY) && N >= 1) {
      const int32_t r = in.ref_obs[p];
      if (r < 0 || r >= N) return mpr_fail(kMprRef, p);
      const dvm_mp_refresh_kf& f = in.kfs[in.obs[o0 + r].kf];       // (its level table is read from its slot)
      if ((f.flags & DVM_MPR_KF_BAD) && f.slot == -1) return mpr_fail(kMprRefBad, p, in.obs[o0 + r].kf, o0 + r);
    }
    if (N > max_obs) max_obs = N;
  }
  MprVerdict ok;
  ok.max_obs = max_obs;
  return ok;
}

}  // namespace dvm
