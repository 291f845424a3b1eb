// dvm_slam_amd/csrc/tri_device.h -- the two per-item bodies of LocalMapping::CreateNewMapPoints' device path, shared by the single calls
// (k_match_triangulation, k_triangulate_matches: match_kernels.hip) and by the chain (new_points_kernels.hip), so that both evaluate ONE
// operation sequence:
//   TriQuery / tri_candidate   ORBmatcher::SearchForTriangulation's per-candidate test (reference src/ORBmatcher.cc:905-960, monocular)
//   tri_pair_geometry          the per-match body of CreateNewMapPoints (src/LocalMapping.cc:598-741, GeometricTools.cc:48-67)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jacobi4.h"
#include "match_kernels.h"
#include "pose_f32.h"

namespace dvm {

// a KF1 keypoint as a query: its descriptor and its epipolar line in the second image, l = x1' F12 = [a b c]
struct TriQuery {
  uint32_t w[8];
  float a, b, c, den;
};
__device__ __forceinline__ TriQuery tri_query(const uint8_t* __restrict__ desc1, const dvm_keypoint_pod* __restrict__ kps1, int idx1, const float* F12) {
  TriQuery Q;
  const uint32_t* qd = reinterpret_cast<const uint32_t*>(desc1 + (size_t)idx1 * 32);
#pragma unroll
  for (int i = 0; i < 8; i++) Q.w[i] = qd[i];
  const float x1 = kps1[idx1].x, y1 = kps1[idx1].y;
  Q.a = __fadd_rn(__fadd_rn(__fmul_rn(x1, F12[0]), __fmul_rn(y1, F12[3])), F12[6]);
  Q.b = __fadd_rn(__fadd_rn(__fmul_rn(x1, F12[1]), __fmul_rn(y1, F12[4])), F12[7]);
  Q.c = __fadd_rn(__fadd_rn(__fmul_rn(x1, F12[2]), __fmul_rn(y1, F12[5])), F12[8]);
  Q.den = __fadd_rn(__fmul_rn(Q.a, Q.a), __fmul_rn(Q.b, Q.b));
  return Q;
}
// KF2 keypoint idx2 as a candidate of Q: its descriptor distance when it passes dist <= th_low, the epipole disc and (unless coarse)
// Pinhole::epipolarConstrain (CameraModels/Pinhole.cpp:104-127); -1 otherwise.  Reads the tables at kps2[idx2].octave.
__device__ __forceinline__ int tri_candidate(const TriQuery& Q, const uint8_t* __restrict__ desc2, const dvm_keypoint_pod* __restrict__ kps2, int idx2,
                                             const TriGeom& G, const float* __restrict__ scale_factors2, const float* __restrict__ level_sigma2_2) {
  const uint4* td = reinterpret_cast<const uint4*>(desc2 + (size_t)idx2 * 32);
  const uint4 A = td[0], B = td[1];
  const int d = __popc(A.x ^ Q.w[0]) + __popc(A.y ^ Q.w[1]) + __popc(A.z ^ Q.w[2]) + __popc(A.w ^ Q.w[3]) +
                __popc(B.x ^ Q.w[4]) + __popc(B.y ^ Q.w[5]) + __popc(B.z ^ Q.w[6]) + __popc(B.w ^ Q.w[7]);
  if (d > G.th_low) return -1;
  const dvm_keypoint_pod kp2 = kps2[idx2];
  const float distex = __fsub_rn(G.ep[0], kp2.x), distey = __fsub_rn(G.ep[1], kp2.y);
  if (__fadd_rn(__fmul_rn(distex, distex), __fmul_rn(distey, distey)) < __fmul_rn(100.f, scale_factors2[kp2.octave])) return -1;
  if (!G.coarse) {
    const float num = __fadd_rn(__fadd_rn(__fmul_rn(Q.a, kp2.x), __fmul_rn(Q.b, kp2.y)), Q.c);
    if (Q.den == 0.f) return -1;
    const float dsqr = __fdiv_rn(__fmul_rn(num, num), Q.den);
    if (!((double)dsqr < 3.84 * (double)level_sigma2_2[kp2.octave])) return -1;
  }
  return d;
}
// the sequential rule "dist > bestDist -> continue" = minimum distance, LAST position wins a tie = min over this key
__device__ __forceinline__ uint32_t tri_key(int d, int pos) { return ((uint32_t)d << 16) | (uint32_t)(0xFFFF - pos); }
__device__ __forceinline__ int tri_key_pos(uint32_t k) { return 0xFFFF - (int)(k & 0xFFFFu); }
// min over the 16 lanes of a DPP row
__device__ __forceinline__ uint32_t tri_row_min(uint32_t k) {
  k = min(k, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)k, 0xB1, 0xF, 0xF, false));
  k = min(k, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)k, 0x4E, 0xF, 0xF, false));
  k = min(k, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)k, 0x141, 0xF, 0xF, false));
  k = min(k, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)k, 0x140, 0xF, 0xF, false));
  return k;
}

// One match (kp1, kp2) of one neighbour: parallax of the two rays, the homogeneous point (null vector of the 4x4 system: eigenvector of
// the smallest eigenvalue of A^T A by cyclic Jacobi in double -- the reference runs Eigen::JacobiSVD<Matrix4f>, tolerance parity), depth,
// reprojection error and scale-consistency tests in float in Eigen's evaluation order, comparisons with double literals in double.
// Returns the status (include/dvmslam_hip.h); X = the point, zeros when no triangulation was attempted.
__device__ __forceinline__ int tri_pair_geometry(const TriPair& P, const dvm_keypoint_pod& kp1, const dvm_keypoint_pod& kp2,
                                                 const float* __restrict__ sigma2_1, const float* __restrict__ sigma2_2,
                                                 const float* __restrict__ sf1, const float* __restrict__ sf2, float* X) {
  using dvm_pose::sum3;
  X[0] = X[1] = X[2] = 0.0f;
  if (kp1.octave < 0 || kp1.octave >= P.n_levels || kp2.octave < 0 || kp2.octave >= P.n_levels) return -1;
  const float* T1w = P.T1w;
  const float* T2w = P.T2w;
  const float xn1[3] = {(kp1.x - P.K1[2]) / P.K1[0], (kp1.y - P.K1[3]) / P.K1[1], 1.0f};
  const float xn2[3] = {(kp2.x - P.K2[2]) / P.K2[0], (kp2.y - P.K2[3]) / P.K2[1], 1.0f};
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
  jacobi4_dev(B, V);
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
    const float u = P.K1[0] * x1 / z1 + P.K1[2], v = P.K1[1] * y1 / z1 + P.K1[3];
    const float ex = u - kp1.x, ey = v - kp1.y;
    if ((double)(ex * ex + ey * ey) > 5.991 * (double)sigma2_1[kp1.octave]) return 5;
  }
  {
    const float x2 = sum3(T2w[0] * x3D[0], T2w[1] * x3D[1], T2w[2] * x3D[2]) + T2w[3];
    const float y2 = sum3(T2w[4] * x3D[0], T2w[5] * x3D[1], T2w[6] * x3D[2]) + T2w[7];
    const float u = P.K2[0] * x2 / z2 + P.K2[2], v = P.K2[1] * y2 / z2 + P.K2[3];
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

}  // namespace dvm
