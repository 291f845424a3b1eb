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
  const float* inv_sigma2;       // mvInvLevelSigma2 [n_levels]
  FrameView F;                   // the target's span of the packed grid arrays (cap = n)
  ProjectCam C;                  // (th is a run argument: C.th is not read)
  int32_t n, pad_;
};
struct FtPoints {   // the point table of one run (device pointers)
  const float *pos, *normal, *min_dist, *max_dist;
  const uint8_t *desc, *valid, *skip;   // valid [n] / skip [T * n] may be null
  int32_t n;
};
void launch_ft_build(hipStream_t s, const FtTargetDev* targets, int n_targets);
void launch_ft_search(hipStream_t s, const FtTargetDev* targets, int n_targets, const FtPoints& P, float th, int32_t* best_idx, int32_t* best_dist);

}  // namespace dvm
