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

}  // namespace dvm
