// dvm_slam_amd/csrc/new_points_kernels.h -- launchers of the LocalMapping::CreateNewMapPoints chain (new_points_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.h"

namespace dvm {

// one keyframe inside the packed upload (device pointers)
struct NpKfDev {
  const dvm_keypoint_pod* kps;
  const uint8_t* desc;
  const int32_t* mp;
  const int32_t *fv_node, *fv_off, *fv_feat;
  const float *sf, *sigma2;
  int32_t n, fv_n;
};
// one neighbour that passed the baseline test: its arrays, the search's geometry (F12, epipole) and the triangulation's (K, T, Ow of both)
struct NpNbDev {
  NpKfDev kf;
  TriPair P;
  TriGeom G;
  int32_t pad_;
};
struct NpArgs {
  NpKfDev cur;
  const NpNbDev* nb;              // [nrun]
  int32_t nrun, n1, n1p, nfeat1;  // neighbours that run; cur's keypoints, that rounded up to 64 (row stride of the speculative arrays), its FeatureVector's features
  int32_t n_levels, check_ori;
  // speculative results, [nrun][n1p]: best KF2 index of KF1 keypoint i (-1 none; preset by the caller), its status and point
  int32_t* best;
  int32_t* st;
  float* X;
  // results (mapped host memory): per running neighbour, then the flat records
  int32_t *h_matches, *h_pair_off, *h_pairs, *h_status, *h_new_point;
  float* h_x3D;
};
// the chain on KannalaBrandt8 keyframes (dvm_create_new_map_points_cam, model 1): beside NpArgs, per running neighbour the search's
// geometry on such a pair (the cameras' parameters, the relative pose, the epipole)
struct NpArgsKB8 {
  NpArgs A;
  const TriGeomKB8* G;            // [nrun]
};
void launch_np_search_kb8(hipStream_t s, const NpArgsKB8& K);
void launch_np_geometry_kb8(hipStream_t s, const NpArgsKB8& K);
void launch_np_search(hipStream_t s, const NpArgs& A);
void launch_np_geometry(hipStream_t s, const NpArgs& A);
void launch_np_settle(hipStream_t s, const NpArgs& A);

}  // namespace dvm
