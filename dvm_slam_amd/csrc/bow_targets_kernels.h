// dvm_slam_amd/csrc/bow_targets_kernels.h -- launchers of the KeyFrame -> KeyFrame SearchByBoW against many targets (bow_targets_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dvm {

// one keyframe inside the handle's device block: the arrays the search reads, as uploaded (entry 0 of the table is the current keyframe,
// entry 1 + t target t)
struct BtKfDev {
  const float* angle;            // [n] mvKeysUn[i].angle
  const uint8_t* desc;           // [n][32]
  const uint8_t* use;            // [n] 1: the keypoint has a map point that is not bad
  const int32_t* fv_node;        // [fv_n] ascending as unsigned
  const int32_t* fv_off;         // [fv_n + 1]
  const int32_t* fv_feat;        // [fv_off[fv_n]]
  int32_t n, fv_n;
};
constexpr int kBtCnt = 32;       // counters of one target: [0, 30) the rotation histogram, [30] the matches before the rotation check
// match [T][n1], bin [T][n1] (written where match >= 0), cnt [T][kBtCnt] zeroed by the upload
void launch_bt_search(hipStream_t s, const BtKfDev* tab, int n_targets, int n1, int fv_n1, float nnratio, int32_t* match, int8_t* bin, int32_t* cnt);
void launch_bt_settle(hipStream_t s, const BtKfDev* tab, int n_targets, int n1, int check_ori, int32_t* match, const int8_t* bin, const int32_t* cnt,
                      int32_t* nmatches);

// ---- the resident call (dvm_search_by_bow_targets_resident): desc and the FeatureVector of a table entry point into a keyframe-store
// slot; angle and use point into the handle's device block, which nothing uploads -- k_bt_prologue writes them.  What it reads per entry:
struct BtProKf {
  const uint8_t* recs;           // the keyframe's map store: [capacity] records of 72 bytes (dvm_local_point); not read when every mp_slot < 0
  const int32_t* mp_slot;        // [n] uploaded, the list rounded up to 64 bytes: GetMapPointMatches() as slots of recs, -1 = none
  const uint8_t* kps;            // the slot's keypoint records, [n] of 28 bytes (dvm_keypoint)
  uint64_t reserved;
};                               // 32 bytes
constexpr int kBtProThreads = 256;                   // k_bt_prologue's workgroup
constexpr int kBtProSpan = kBtProThreads * 4;        // keypoints of one workgroup, four per thread
// ONE launch: for every entry k of tab [n_kf] (the current keyframe and the targets) use[i] = mp_slot[i] >= 0 && !record.bad and
// angle[i] = kps[i].angle, written through tab[k].use / tab[k].angle; match [n_match] = -1; cnt [n_cnt] = 0.  n_max: the largest n of tab.
// match and cnt at multiples of 16 bytes, n_cnt a multiple of 4; the host has checked every slot of every list.
void launch_bt_prologue(hipStream_t s, const BtKfDev* tab, const BtProKf* pro, int n_kf, int n_max, int32_t* match, int64_t n_match, int32_t* cnt,
                        int n_cnt);

}  // namespace dvm
