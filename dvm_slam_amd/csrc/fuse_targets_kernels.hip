// dvm_slam_amd/csrc/fuse_targets_kernels.hip -- the search part of ORBmatcher::Fuse(pKF, vpMapPoints, th) (reference src/ORBmatcher.cc:
// 1089-1210) for ALL target keyframes of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:812-821) at once (dvm_fuse_targets,
// include/dvmslam_hip.h):
//   k_ft_build    the feature grids of all targets in one launch, one workgroup per target, into back-to-back spans
//   k_ft_search   one DPP row (16 lanes) per (target, map point): the projection gates and the window search of k_project_search with the
//                 5.99 gate, then Fuse's acceptance (best distance <= TH_LOW)
// Both kernels call the device functions the single calls run (proj_device.h), so entry (t, i) is dvm_project_search on target t alone.
// What the sequential loop of the reference changes between two targets -- isBad(), IsInKeyFrame(), a survivor's descriptor -- never
// reaches these kernels: the caller masks or repeats rows (the skip array of a run).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fuse_targets_kernels.h"
#include "proj_device.h"

namespace dvm {

__global__ void __launch_bounds__(1024) k_ft_build(const FtTargetDev* __restrict__ targets) {
  const FtTargetDev& T = targets[blockIdx.x];
  frame_build_block(T.kps, T.desc, T.n, T.F);
}

// blockIdx.y = target.  A row whose point is masked (valid[i] == 0 or skip[t * n + i] != 0) writes "none" and leaves before anything is read.
__global__ void __launch_bounds__(256) k_ft_search(const FtTargetDev* __restrict__ targets, FtPoints P, float th,
                                                   int32_t* __restrict__ best_idx, int32_t* __restrict__ best_dist) {
  const int lane = threadIdx.x & 15;
  const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
  if (i >= P.n) return;
  const int t = blockIdx.y;
  const size_t e = (size_t)t * P.n + i;
  if ((P.valid && P.valid[i] == 0) || (P.skip && P.skip[e] != 0)) {   // uniform inside the row
    if (lane == 0) { best_idx[e] = -1; best_dist[e] = 256; }
    return;
  }
  const FtTargetDev& T = targets[t];
  const ProjectRow R = project_row(T.F, nullptr, T.C, th, P.pos, P.normal, P.min_dist, P.max_dist, P.desc, true, i, T.sf, T.inv_sigma2, 5.99, lane);
  if (lane == 0) {
    const int d = (int)(R.k1 >> 16);
    best_dist[e] = d;
    best_idx[e] = d <= 50 ? T.F.sidx[R.k1 & 0xFFFFu] : -1;   // ORBmatcher::TH_LOW (:1213); d = 256: no candidate
  }
}

void launch_ft_build(hipStream_t s, const FtTargetDev* targets, int n_targets) {
  if (n_targets > 0) hipLaunchKernelGGL(k_ft_build, dim3(n_targets), dim3(1024), 0, s, targets);
}
void launch_ft_search(hipStream_t s, const FtTargetDev* targets, int n_targets, const FtPoints& P, float th, int32_t* best_idx, int32_t* best_dist) {
  if (n_targets > 0 && P.n > 0)
    hipLaunchKernelGGL(k_ft_search, dim3((P.n + 15) / 16, n_targets), dim3(256), 0, s, targets, P, th, best_idx, best_dist);
}

}  // namespace dvm
