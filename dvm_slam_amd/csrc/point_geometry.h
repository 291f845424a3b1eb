// dvm_slam_amd/csrc/point_geometry.h -- MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:473-540) for one map point, written
// ONCE for the two kernels that produce a record's normal and distances: k_ba_res_points (ba_window_resident.hip, a lane per point, the
// terms one after another) and k_mp_refresh (map_refresh_kernels.hip, a wavefront per point, the terms across the lanes).  Both SUM the
// terms in the list's order, so both leave the same bits.  Float arithmetic: one rounding per operation (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include "pose_f32.h"

namespace dvm {

// Vector3f::norm(): sqrt(a0 + (a1 + a2))
__device__ __forceinline__ float res_norm3(const float* d) { return sqrtf(dvm_pose::sum3(d[0] * d[0], d[1] * d[1], d[2] * d[2])); }

// one observation's term (:506-512): normali = Pos - Owi;  t = normali / normali.norm()
__device__ __forceinline__ void geo_term(const float* pos, const float* ow, float* t) {
  const float d[3] = {pos[0] - ow[0], pos[1] - ow[1], pos[2] - ow[2]};
  const float n = res_norm3(d);
  t[0] = d[0] / n; t[1] = d[1] / n; t[2] = d[2] / n;
}
// normal = normal + t, the terms in the list's order from normal = 0
__device__ __forceinline__ void geo_add(float* normal, float t0, float t1, float t2) {
  normal[0] = normal[0] + t0; normal[1] = normal[1] + t1; normal[2] = normal[2] + t2;
}
// g[0 .. 5]: the position and mNormalVector = normal / n (:535)
__device__ __forceinline__ void geo_mean(const float* pos, const float* normal, int n, float* g) {
  const float cnt = (float)n;
  g[0] = pos[0]; g[1] = pos[1]; g[2] = pos[2];
  g[3] = normal[0] / cnt; g[4] = normal[1] / cnt; g[5] = normal[2] / cnt;
}
// g[6], g[7]: mfMinDistance and mfMaxDistance (:515-534) from the reference keyframe's centre and level table (sf [n_levels]; octave:
// the level of the reference observation's keypoint)
__device__ __forceinline__ void geo_distances(const float* pos, const float* ow_ref, const float* sf, int octave, int n_levels, float* g) {
  const float d[3] = {pos[0] - ow_ref[0], pos[1] - ow_ref[1], pos[2] - ow_ref[2]};
  const float max_dist = res_norm3(d) * sf[octave];
  g[7] = max_dist;
  g[6] = max_dist / sf[n_levels - 1];
}

}  // namespace dvm
