// dvm_slam_amd/csrc/fuse_targets_kernels.h -- launchers of the Fuse searches of LocalMapping::SearchInNeighbors (fuse_targets_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.h"

namespace dvm {

// one target keyframe inside the handle's device block: its uploaded arrays, its grid span and what k_project_search takes as arguments
struct FtTargetDev {
  const dvm_keypoint_pod* kps;   // [n] as uploaded
  const uint8_t* desc;           // [n][32]
  const float* sf;               // mvScaleFactors [n_levels]
  const float* inv_sigma2;       // mvInvLevelSigma2 [n_levels]; null: the ungated form (DVM_FT_FORM_SCW)
  FrameView F;                   // the target's span of the packed grid arrays (cap = n)
  ProjectCam C;                  // (th is a run argument: C.th is not read)
  int32_t n, model;              // model: dvm_cam::kPinhole (C.fx .. cy) / kKannalaBrandt8 (kb8)
  float kb8[8];                  // mvParameters of a KannalaBrandt8 target
};
struct FtHit { int32_t point, idx, dist; };   // == dvm_ft_hit
struct FtPoints {   // the point table of one run (device pointers)
  const float *pos, *normal, *min_dist, *max_dist;
  const uint8_t *desc, *valid, *skip;   // valid [n] / skip [T * n] may be null
  int32_t n;
};
void launch_ft_build(hipStream_t s, const FtTargetDev* targets, int n_targets);
// order [n_pinhole + n_kb8]: the targets' indices, the pinhole targets first: one launch per model type present, blockIdx.y walks its part
// of the list (rows are independent, so a mixed call is two launches over disjoint rows)
void launch_ft_search(hipStream_t s, const FtTargetDev* targets, const int32_t* order, int n_pinhole, int n_kb8, const FtPoints& P, float th,
                      int32_t* best_idx, int32_t* best_dist);
// the hits of dense rows [n_targets][n], stable, in three launches (count per target, scan over the targets, write): off [n_targets + 1]
// goes to device memory and to off_out, the hits below position cap to hits_out (both may be mapped host memory: plain vector stores)
void launch_ft_hits(hipStream_t s, const int32_t* best_idx, const int32_t* best_dist, int n_targets, int n, int32_t* cnt, int32_t* off,
                    int32_t* off_out, FtHit* hits_out, int cap);

}  // namespace dvm
