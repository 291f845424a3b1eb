// dvm_slam_amd/csrc/tri_model.h -- the per-item arithmetic of LocalMapping::CreateNewMapPoints' device path for either camera model of
// camera_model.h, written once for the kernels (tri_device.h) and for the host (tests/test_kb8_tri_model.py builds it with g++):
//   unproject / project<MODEL>   pCamera->unprojectEig(kp.pt), pCamera->project(Point3f) (Pinhole.cpp, KannalaBrandt8.cpp)
//   null_vector                  the homogeneous point of a 4x4 system: eigenvector of the smallest eigenvalue of A^T A (jacobi4.h, double)
//   pair_geometry<MODEL>         the per-match body of CreateNewMapPoints (src/LocalMapping.cc:598-741, GeometricTools.cc:48-67)
//   kb8_triangulate_matches      KannalaBrandt8::TriangulateMatches (CameraModels/KannalaBrandt8.cpp:304-374, :392-403), whose value
//                                > 0.0001f is KannalaBrandt8::epipolarConstrain (:216-220), SearchForTriangulation's test on such a camera
//   pair_pose                    R21 = R12^T and -R21 t12, once per pair on the host
// The structs are template parameters (PAIR: dvm_tri_pair or its device twin, KP: dvm_keypoint or its device twin), so this header needs
// neither the HIP runtime nor the public header.  -ffp-contract=off on the translation unit, as for camera_model.h.
#pragma once
#include <math.h>
#include <stdint.h>

#include "camera_model.h"
#include "jacobi4.h"
#include "pose_f32.h"

namespace dvm_tri {

using dvm_cam::kKannalaBrandt8;
using dvm_cam::kPinhole;

// the relative pose of a pair as SearchForTriangulation holds it (T12 = T1w * Tw2, ORBmatcher.cc:856-859) and what TriangulateMatches
// derives from it for every candidate (:335-336).  == dvm_pair_pose
struct PairPose {
  float R12[9], t12[3];
  float R21[9], t21[3];   // R12^T, -R21 t12
};
inline void pair_pose(const float* R12, const float* t12, PairPose& out) {
  for (int i = 0; i < 9; i++) out.R12[i] = R12[i];
  for (int i = 0; i < 3; i++) out.t12[i] = t12[i];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) out.R21[3 * r + c] = R12[3 * c + r];
  for (int r = 0; r < 3; r++) out.t21[r] = dvm_pose::sum3(-out.R21[3 * r] * t12[0], -out.R21[3 * r + 1] * t12[1], -out.R21[3 * r + 2] * t12[2]);
}

// cam = mvParameters: fx, fy, cx, cy (, k1 .. k4 under KannalaBrandt8)
template <int MODEL>
DVM_CAM_HD void unproject(const float* cam, float u, float v, float* ray) {
  if (MODEL == kKannalaBrandt8) {
    dvm_cam::kb8_unproject(cam, u, v, ray);
  } else {
    ray[0] = (u - cam[2]) / cam[0]; ray[1] = (v - cam[3]) / cam[1]; ray[2] = 1.0f;
  }
}
template <int MODEL>
DVM_CAM_HD void project(const float* cam, float x, float y, float z, float& u, float& v) {
  if (MODEL == kKannalaBrandt8) {
    dvm_cam::kb8_project(cam, x, y, z, u, v);
  } else {
    u = cam[0] * x / z + cam[2]; v = cam[1] * y / z + cam[3];
  }
}

// the right singular vector of A's smallest singular value, as floats (the reference runs Eigen::JacobiSVD<Matrix4f>: tolerance parity)
DVM_CAM_HD void null_vector(const float A[4][4], float vh[4]) {
  double B[4][4], V[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 4; k++) acc += (double)A[k][i] * (double)A[k][j];
      B[i][j] = acc;
    }
  dvm::jacobi4_dev(B, V);
  int mi = 0;
#pragma unroll
  for (int k = 1; k < 4; k++) if (B[k][k] < B[mi][mi]) mi = k;
#pragma unroll
  for (int k = 0; k < 4; k++) vh[k] = (float)(mi == 0 ? V[k][0] : mi == 1 ? V[k][1] : mi == 2 ? V[k][2] : V[k][3]);
}

// One match (kp1, kp2) of one neighbour, xn1 / xn2 = the two keypoints' rays (unproject<MODEL>): parallax of the rays, the homogeneous
// point, depth, reprojection error through project<MODEL> and scale-consistency tests in float in Eigen's evaluation order, comparisons with
// double literals in double.  Returns the status (include/dvmslam_hip.h); X = the point, zeros when no triangulation was attempted.
template <int MODEL, class PAIR, class KP>
DVM_CAM_HD int pair_geometry(const PAIR& P, const KP& kp1, const KP& kp2, const float* xn1, const float* xn2, const float* cam1, const float* cam2,
                             const float* sigma2_1, const float* sigma2_2, const float* sf1, const float* sf2, float* X) {
  using dvm_pose::sum3;
  const float* T1w = P.T1w;
  const float* T2w = P.T2w;
  float r1[3], r2[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    r1[i] = sum3(T1w[i] * xn1[0], T1w[4 + i] * xn1[1], T1w[8 + i] * xn1[2]);
    r2[i] = sum3(T2w[i] * xn2[0], T2w[4 + i] * xn2[1], T2w[8 + i] * xn2[2]);
  }
  const float nr1 = sqrtf(sum3(r1[0] * r1[0], r1[1] * r1[1], r1[2] * r1[2])), nr2 = sqrtf(sum3(r2[0] * r2[0], r2[1] * r2[1], r2[2] * r2[2]));
  const float cosParallaxRays = sum3(r1[0] * r2[0], r1[1] * r2[1], r1[2] * r2[2]) / (nr1 * nr2);
  const float cosParallaxStereo = cosParallaxRays + 1;
  if (!(cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (double)cosParallaxRays < P.cos_parallax_max)) return 1;
  float A[4][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    A[0][k] = xn1[0] * T1w[8 + k] - T1w[k];
    A[1][k] = xn1[1] * T1w[8 + k] - T1w[4 + k];
    A[2][k] = xn2[0] * T2w[8 + k] - T2w[k];
    A[3][k] = xn2[1] * T2w[8 + k] - T2w[4 + k];
  }
  double B[4][4], V[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 4; k++) acc += (double)A[k][i] * (double)A[k][j];
      B[i][j] = acc;
    }
  dvm::jacobi4_dev(B, V);
  int mi = 0;
#pragma unroll
  for (int k = 1; k < 4; k++) if (B[k][k] < B[mi][mi]) mi = k;
  float vh[4];
#pragma unroll
  for (int k = 0; k < 4; k++) vh[k] = (float)(mi == 0 ? V[k][0] : mi == 1 ? V[k][1] : mi == 2 ? V[k][2] : V[k][3]);
  if (vh[3] == 0) return 2;
  const float x3D[3] = {vh[0] / vh[3], vh[1] / vh[3], vh[2] / vh[3]};
  X[0] = x3D[0]; X[1] = x3D[1]; X[2] = x3D[2];
  const float z1 = sum3(T1w[8] * x3D[0], T1w[9] * x3D[1], T1w[10] * x3D[2]) + T1w[11];
  if (z1 <= 0) return 3;
  const float z2 = sum3(T2w[8] * x3D[0], T2w[9] * x3D[1], T2w[10] * x3D[2]) + T2w[11];
  if (z2 <= 0) return 4;
  {
    const float x1 = sum3(T1w[0] * x3D[0], T1w[1] * x3D[1], T1w[2] * x3D[2]) + T1w[3];
    const float y1 = sum3(T1w[4] * x3D[0], T1w[5] * x3D[1], T1w[6] * x3D[2]) + T1w[7];
    float u, v;
    project<MODEL>(cam1, x1, y1, z1, u, v);
    const float ex = u - kp1.x, ey = v - kp1.y;
    if ((double)(ex * ex + ey * ey) > 5.991 * (double)sigma2_1[kp1.octave]) return 5;
  }
  {
    const float x2 = sum3(T2w[0] * x3D[0], T2w[1] * x3D[1], T2w[2] * x3D[2]) + T2w[3];
    const float y2 = sum3(T2w[4] * x3D[0], T2w[5] * x3D[1], T2w[6] * x3D[2]) + T2w[7];
    float u, v;
    project<MODEL>(cam2, x2, y2, z2, u, v);
    const float ex = u - kp2.x, ey = v - kp2.y;
    if ((double)(ex * ex + ey * ey) > 5.991 * (double)sigma2_2[kp2.octave]) return 6;
  }
  const float d1[3] = {x3D[0] - P.Ow1[0], x3D[1] - P.Ow1[1], x3D[2] - P.Ow1[2]}, d2[3] = {x3D[0] - P.Ow2[0], x3D[1] - P.Ow2[1], x3D[2] - P.Ow2[2]};
  const float dist1 = sqrtf(sum3(d1[0] * d1[0], d1[1] * d1[1], d1[2] * d1[2])), dist2 = sqrtf(sum3(d2[0] * d2[0], d2[1] * d2[1], d2[2] * d2[2]));
  if (dist1 == 0 || dist2 == 0) return 7;
  if (P.far_points && (dist1 >= P.th_far || dist2 >= P.th_far)) return 8;
  const float ratioDist = dist2 / dist1;
  const float ratioOctave = sf1[kp1.octave] / sf2[kp2.octave];
  if (ratioDist * P.ratio_factor < ratioOctave || ratioDist > ratioOctave * P.ratio_factor) return 9;
  return 0;
}

// KannalaBrandt8::TriangulateMatches, all in float: r1 / r2 = the rays of kp1 (u1, v1) in camera 1 and kp2 (u2, v2) in camera 2,
// sigma1 = KF1's mvLevelSigma2[kp1.octave], sigma2 = KF2's mvLevelSigma2[kp2.octave].  Returns what the reference returns: -1 parallax
// (compared against the double 0.9998), -2 / -3 the point behind camera 1 / 2, -4 / -5 the reprojection error in image 1 / 2, else z1.
// Camera 1 is [I | 0] and camera 2 [R21 | t21]; Triangulate divides by the fourth component with no w == 0 test.
DVM_CAM_HD float kb8_triangulate_matches(const float* cam1, const float* cam2, const float* r1, const float* r2, float u1, float v1, float u2, float v2,
                                         const PairPose& R, float sigma1, float sigma2, float* x3D) {
  using dvm_pose::sum3;
  float r21[3];
#pragma unroll
  for (int i = 0; i < 3; i++) r21[i] = sum3(R.R12[3 * i] * r2[0], R.R12[3 * i + 1] * r2[1], R.R12[3 * i + 2] * r2[2]);
  const float n1 = sqrtf(sum3(r1[0] * r1[0], r1[1] * r1[1], r1[2] * r1[2])), n21 = sqrtf(sum3(r21[0] * r21[0], r21[1] * r21[1], r21[2] * r21[2]));
  const float cosParallaxRays = sum3(r1[0] * r21[0], r1[1] * r21[1], r1[2] * r21[2]) / (n1 * n21);
  x3D[0] = x3D[1] = x3D[2] = 0.0f;
  if ((double)cosParallaxRays > 0.9998) return -1.0f;
  const float T1[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  const float T2[12] = {R.R21[0], R.R21[1], R.R21[2], R.t21[0], R.R21[3], R.R21[4], R.R21[5], R.t21[1], R.R21[6], R.R21[7], R.R21[8], R.t21[2]};
  float A[4][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    A[0][k] = r1[0] * T1[8 + k] - T1[k];
    A[1][k] = r1[1] * T1[8 + k] - T1[4 + k];
    A[2][k] = r2[0] * T2[8 + k] - T2[k];
    A[3][k] = r2[1] * T2[8 + k] - T2[4 + k];
  }
  float vh[4];
  null_vector(A, vh);
  x3D[0] = vh[0] / vh[3]; x3D[1] = vh[1] / vh[3]; x3D[2] = vh[2] / vh[3];
  const float z1 = x3D[2];
  if (z1 <= 0) return -2.0f;
  const float z2 = sum3(T2[8] * x3D[0], T2[9] * x3D[1], T2[10] * x3D[2]) + T2[11];
  if (z2 <= 0) return -3.0f;
  {
    float u, v;
    dvm_cam::kb8_project(cam1, x3D[0], x3D[1], x3D[2], u, v);
    const float ex = u - u1, ey = v - v1;
    if ((double)(ex * ex + ey * ey) > 5.991 * (double)sigma1) return -4.0f;
  }
  {
    const float x2 = sum3(T2[0] * x3D[0], T2[1] * x3D[1], T2[2] * x3D[2]) + T2[3];
    const float y2 = sum3(T2[4] * x3D[0], T2[5] * x3D[1], T2[6] * x3D[2]) + T2[7];
    float u, v;
    dvm_cam::kb8_project(cam2, x2, y2, z2, u, v);
    const float ex = u - u2, ey = v - v2;
    if ((double)(ex * ex + ey * ey) > 5.991 * (double)sigma2) return -5.0f;
  }
  return z1;
}
DVM_CAM_HD bool kb8_epipolar_constrain(const float* cam1, const float* cam2, const float* r1, const float* r2, float u1, float v1, float u2, float v2,
                                       const PairPose& R, float sigma1, float sigma2) {
  float x3D[3];
  return kb8_triangulate_matches(cam1, cam2, r1, r2, u1, v1, u2, v2, R, sigma1, sigma2, x3D) > 0.0001f;
}

}  // namespace dvm_tri
