// dvm_slam_amd/csrc/frustum_point.h -- Frame::isInFrustum of ONE map point, mono branch (reference src/Frame.cc:575-636) +
// MapPoint::PredictScale (src/MapPoint.cc:573-587), float arithmetic in the reference's order.  Shared by k_is_in_frustum
// (match_kernels.hip, dvm_is_in_frustum) and the second half of the tracked frame (track_kernels.hip, dvm_track_local_map).
#pragma once
#include <hip/hip_runtime.h>

#include "camera_model.h"
#include "match_kernels.h"   // FrustumFrame, TrackPoint
#include "pose_f32.h"

namespace dvm {

// p = GetWorldPos(), n = GetNormal(), min_dist / max_dist = mfMinDistance / mfMaxDistance
// MODEL: the camera behind mpCamera->project (Frame.cc:594).  The pinhole instantiation is what every chain calls; KannalaBrandt8
// (k_is_in_frustum_kb8 only) reads mvParameters from kb8 (camera_model.h) and none of F.fx, fy, cx, cy.
template <int MODEL = dvm_cam::kPinhole>
__device__ __forceinline__ TrackPoint frustum_point(const FrustumFrame& F, float p0, float p1, float p2, float n0, float n1, float n2,
                                                    float min_dist, float max_dist, float cos_limit, const float* kb8 = nullptr) {
  TrackPoint o;
  o.in_view = 0; o.proj_x = -1; o.proj_y = -1; o.proj_xr = 0; o.depth = 0; o.level = -1; o.view_cos = 0;
  // Pc = mRcw * P + mtcw (Frame.cc:585): Eigen's 3x3 * 3x1 coefficient is a0 + (a1 + a2)
  const float X = dvm_pose::sum3(F.Rcw[0] * p0, F.Rcw[1] * p1, F.Rcw[2] * p2) + F.tcw[0];
  const float Y = dvm_pose::sum3(F.Rcw[3] * p0, F.Rcw[4] * p1, F.Rcw[5] * p2) + F.tcw[1];
  const float Z = dvm_pose::sum3(F.Rcw[6] * p0, F.Rcw[7] * p1, F.Rcw[8] * p2) + F.tcw[2];
  const float Pc_dist = sqrtf(dvm_pose::sum3(X * X, Y * Y, Z * Z));
  const float invz = 1.0f / Z;
  bool ok = !(Z < 0.0f);
  float u, v;
  if constexpr (MODEL == dvm_cam::kKannalaBrandt8) dvm_cam::kb8_project(kb8, X, Y, Z, u, v);
  else { u = F.fx * X / Z + F.cx; v = F.fy * Y / Z + F.cy; }
  ok = ok && !(u < F.min_x || u > F.max_x) && !(v < F.min_y || v > F.max_y);
  if (ok) {
    o.proj_x = u; o.proj_y = v;
    const float maxDistance = 1.2f * max_dist, minDistance = 0.8f * min_dist;
    const float q0 = p0 - F.Ow[0], q1 = p1 - F.Ow[1], q2 = p2 - F.Ow[2];
    const float dist = sqrtf(dvm_pose::sum3(q0 * q0, q1 * q1, q2 * q2));
    if (!(dist < minDistance || dist > maxDistance)) {
      const float viewCos = dvm_pose::sum3(q0 * n0, q1 * n1, q2 * n2) / dist;
      if (!(viewCos < cos_limit)) {
        const int nScale = dvm_pose::predict_scale(max_dist, dist, F.log_scale_factor, F.n_levels);
        o.in_view = 1; o.proj_xr = u - F.bf * invz; o.depth = Pc_dist; o.level = nScale; o.view_cos = viewCos;
      }
    }
  }
  return o;
}

}  // namespace dvm
