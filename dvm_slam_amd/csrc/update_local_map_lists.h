// dvm_slam_amd/csrc/update_local_map_lists.h -- host side of dvm_update_local_map (update_local_map.cpp): the sizes of a reservation, the
// upload's layout and every check of a call's lists, decided before anything is queued, so that the k_ulm_* kernels
// (update_local_map_kernels.hip) index with checked values only.  Pure host code, no HIP.
//   ulm_check_reserve     the six sizes of dvm_update_local_map_reserve
//   ulm_check_keyframes   a dvm_update_local_map_keyframes call against the reservation and what the stores know
//   ulm_check_points      a dvm_update_local_map_points call, likewise
//   ulm_*_upload_bytes    the exact length of a call's one upload (include/dvmslam_hip.h states the formula)
// What the stores know of a frame travels in UlmFacts, filled by the entry from map_store.h / keyframe_store.h: the checks themselves read
// plain arrays.  The first offence in the order of the code below is the one reported.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/dvmslam_hip.h"

namespace dvm {

constexpr int kUlmBlock = 256;                    // entries of a row one workgroup of the mark / count / write kernels takes
constexpr int32_t kUlmFirstIdle = 0x7f7f7f7f;     // an idle word of `first` (what a byte-wise memset writes; above every key)
constexpr size_t kUlmParamBytes = 64;             // the per-frame parameter block (UlmFrameDev)

struct UlmReserve { int32_t max_frames, max_frame_keypoints, max_local_keyframes, map_capacity, kf_capacity, slot_keypoints; };
// words of a list of n entries in the upload: rounded up to 64 bytes
inline size_t ulm_pad16(size_t n) { return (n + 15) & ~(size_t)15; }
// workgroups per row: a key is (k * row_blocks + block) * 256 + lane = k * (padded row length) + kp
inline int32_t ulm_row_blocks(int32_t slot_keypoints) { return (slot_keypoints + kUlmBlock - 1) / kUlmBlock; }
inline int32_t ulm_key(int32_t k, int32_t kp, int32_t row_blocks) { return k * row_blocks * kUlmBlock + kp; }

enum UlmFault {
  kUlmOk = 0,
  kUlmNull,            // a NULL argument with a non-zero count                                   (frame)
  kUlmCount,           // a negative count                                                         (frame)
  kUlmNoReserve,       // no reservation yet: DVM_ERR_CAPACITY
  kUlmFrames,          // more frames than max_frames: DVM_ERR_CAPACITY
  kUlmKeypoints,       // a frame's n beyond max_frame_keypoints: DVM_ERR_CAPACITY                 (frame)
  kUlmLocalKfs,        // a frame's n_kfs beyond max_local_keyframes: DVM_ERR_CAPACITY             (frame)
  kUlmMapTable,        // the map store holds more slots than map_capacity: DVM_ERR_CAPACITY       (frame)
  kUlmKfTable,         // the keyframe store holds more slots than kf_capacity: DVM_ERR_CAPACITY   (frame)
  kUlmSlotKeypoints,   // the keyframe store's slot_keypoints beyond the reservation's: DVM_ERR_CAPACITY (frame)
  kUlmDevice,          // a store on another device                                                (frame)
  kUlmFrameSlot,       // a frame slot below -1, outside its map store or never written            (frame, at)
  kUlmKfSlot,          // a kf_slot outside the store, never put or removed                        (frame, at)
  kUlmKfNoRow,         // a kf_slot without a MATCHES row                                          (frame, at)
  kUlmKfTwice,         // a kf_slot named twice in one frame                                       (frame, at)
  kUlmRowStore,        // a named row names another map store than the frame's                     (frame, at)
  kUlmObservedStore,   // an OBSERVED row of the frame's keyframe store names another map store    (frame)
  kUlmSizes,           // reserve: a size below 0, slot_keypoints outside [1, 8192], or keys that would pass kUlmFirstIdle
};
struct UlmVerdict {
  int fault = kUlmOk;
  int frame = -1, at = -1;
  int rc() const {
    return fault == kUlmOk ? DVM_OK : (fault >= kUlmNoReserve && fault <= kUlmSlotKeypoints) ? DVM_ERR_CAPACITY : DVM_ERR_INVALID;
  }
};
inline UlmVerdict ulm_fail(int fault, int frame = -1, int at = -1) {
  UlmVerdict v;
  v.fault = fault; v.frame = frame; v.at = at;
  return v;
}

inline UlmVerdict ulm_check_reserve(const UlmReserve& R) {
  if (R.max_frames < 0 || R.max_frame_keypoints < 0 || R.max_local_keyframes < 0 || R.map_capacity < 0 || R.kf_capacity < 0) return ulm_fail(kUlmSizes);
  if (R.slot_keypoints < 1 || R.slot_keypoints > 8192) return ulm_fail(kUlmSizes);
  // the largest key plus one, and the largest flat table, stay below what an int32 and an idle word can tell apart
  const int64_t keys = (int64_t)R.max_local_keyframes * ulm_row_blocks(R.slot_keypoints) * kUlmBlock;
  if (keys >= kUlmFirstIdle || (int64_t)R.max_frames * R.map_capacity >= ((int64_t)1 << 31) || (int64_t)R.max_frames * R.kf_capacity >= ((int64_t)1 << 31))
    return ulm_fail(kUlmSizes);
  return UlmVerdict{};
}

// what the stores know of one frame of a call
enum UlmKfState : uint8_t { kUlmKfGood = 0, kUlmKfAbsent, kUlmKfRowless, kUlmKfOtherStore };
struct UlmFacts {
  bool same_device;               // both stores live on the handle's device
  int32_t map_capacity;           // of in[b].points
  const uint8_t* written;         // [map_capacity] of in[b].points
  int32_t kf_capacity, slot_keypoints;   // of in[b].kfs
  bool observed_same;             // every OBSERVED row that is set names in[b].points (keyframes call)
  const uint8_t* kf_state;        // [n_kfs] UlmKfState of each named slot (points call; slots outside the store are kUlmKfAbsent)
};

// a frame's list: every entry -1 or a written slot
inline int ulm_first_bad_slot(const int32_t* slots, int n, int32_t capacity, const uint8_t* written) {
  for (int i = 0; i < n; i++) {
    const int32_t sl = slots[i];
    if (sl == -1) continue;
    if (sl < 0 || sl >= capacity || !written[sl]) return i;
  }
  return -1;
}
inline UlmVerdict ulm_check_frame_common(const UlmReserve& R, const UlmFacts& F, int b, int32_t n, const int32_t* mp_slot) {
  if (n < 0) return ulm_fail(kUlmCount, b);
  if (n > 0 && !mp_slot) return ulm_fail(kUlmNull, b);
  if (!F.same_device) return ulm_fail(kUlmDevice, b);
  if (n > R.max_frame_keypoints) return ulm_fail(kUlmKeypoints, b);
  if (F.map_capacity > R.map_capacity) return ulm_fail(kUlmMapTable, b);
  if (F.kf_capacity > R.kf_capacity) return ulm_fail(kUlmKfTable, b);
  if (F.slot_keypoints > R.slot_keypoints) return ulm_fail(kUlmSlotKeypoints, b);
  const int at = ulm_first_bad_slot(mp_slot, n, F.map_capacity, F.written);
  if (at >= 0) return ulm_fail(kUlmFrameSlot, b, at);
  return UlmVerdict{};
}

inline UlmVerdict ulm_check_keyframes_frame(const UlmReserve& R, const UlmFacts& F, int b, const dvm_ulm_keyframes_in& in, const dvm_ulm_keyframes_out& out) {
  if (!in.kfs || !in.points || !out.votes || (in.n > 0 && !out.frame_bad)) return ulm_fail(kUlmNull, b);
  const UlmVerdict v = ulm_check_frame_common(R, F, b, in.n, in.mp_slot);
  if (v.fault != kUlmOk) return v;
  if (!F.observed_same) return ulm_fail(kUlmObservedStore, b);
  return UlmVerdict{};
}

// stamp [kf_capacity of the reservation], call: the handle's named-once scratch (a slot's stamp equals `call` once the frame named it);
// the caller takes a fresh `call` per frame
inline UlmVerdict ulm_check_points_frame(const UlmReserve& R, const UlmFacts& F, int b, const dvm_ulm_points_in& in, const dvm_ulm_points_out& out,
                                         uint32_t* stamp, uint32_t call) {
  if (!in.kfs || !in.points || (in.n > 0 && !out.frame_mp) || (out.local_cap > 0 && !out.local_slot)) return ulm_fail(kUlmNull, b);
  if (in.n_kfs < 0 || out.local_cap < 0) return ulm_fail(kUlmCount, b);
  if (in.n_kfs > 0 && !in.kf_slot) return ulm_fail(kUlmNull, b);
  if (in.n_kfs > R.max_local_keyframes) return ulm_fail(kUlmLocalKfs, b);
  const UlmVerdict v = ulm_check_frame_common(R, F, b, in.n, in.mp_slot);
  if (v.fault != kUlmOk) return v;
  for (int k = 0; k < in.n_kfs; k++) {
    const int32_t sl = in.kf_slot[k];
    if (sl < 0 || sl >= F.kf_capacity || F.kf_state[k] == kUlmKfAbsent) return ulm_fail(kUlmKfSlot, b, k);
    if (F.kf_state[k] == kUlmKfRowless) return ulm_fail(kUlmKfNoRow, b, k);
    if (stamp[sl] == call) return ulm_fail(kUlmKfTwice, b, k);
    stamp[sl] = call;
    if (F.kf_state[k] == kUlmKfOtherStore) return ulm_fail(kUlmRowStore, b, k);
  }
  return UlmVerdict{};
}

// ---- the one upload: [count parameter blocks of 64 B][frame 0's mp_slot, rounded up to 64 B][frame 0's kf_slot, likewise][frame 1's ...]
inline size_t ulm_keyframes_upload_bytes(int count, const dvm_ulm_keyframes_in* in) {
  size_t b = (size_t)count * kUlmParamBytes;
  for (int f = 0; f < count; f++) b += 4 * ulm_pad16((size_t)in[f].n);
  return b;
}
inline size_t ulm_points_upload_bytes(int count, const dvm_ulm_points_in* in) {
  size_t b = (size_t)count * kUlmParamBytes;
  for (int f = 0; f < count; f++) b += 4 * (ulm_pad16((size_t)in[f].n) + ulm_pad16((size_t)in[f].n_kfs));
  return b;
}

}  // namespace dvm
