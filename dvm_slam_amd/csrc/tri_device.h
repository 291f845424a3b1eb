// dvm_slam_amd/csrc/tri_device.h -- the two per-item bodies of LocalMapping::CreateNewMapPoints' device path, shared by the single calls
// (k_match_triangulation, k_triangulate_matches: match_kernels.hip) and by the chain (new_points_kernels.hip), so that both evaluate ONE
// operation sequence:
//   TriQuery / tri_candidate   ORBmatcher::SearchForTriangulation's per-candidate test (reference src/ORBmatcher.cc:905-960, monocular)
//   tri_pair_geometry<MODEL>   the per-match body of CreateNewMapPoints (src/LocalMapping.cc:598-741, GeometricTools.cc:48-67)
//   tri_rows_kb8               the same test for a workgroup of 16 queries on a KannalaBrandt8 pair (CameraModels/KannalaBrandt8.cpp:216-220, :304-374)
// The arithmetic that depends on the camera lives in tri_model.h, which also compiles for the host; the descriptor distance and the row
// minimum are match_device.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_device.h"
#include "match_kernels.h"
#include "pose_f32.h"
#include "tri_model.h"

namespace dvm {

// a KF1 keypoint as a query: its descriptor and its epipolar line in the second image, l = x1' F12 = [a b c]
struct TriQuery {
  uint32_t w[8];
  float a, b, c, den;
};
__device__ __forceinline__ TriQuery tri_query(const uint8_t* __restrict__ desc1, const dvm_keypoint_pod* __restrict__ kps1, int idx1, const float* F12) {
  TriQuery Q;
  desc_load(desc1, idx1, Q.w);
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
  const int d = desc_distance(Q.w, desc2, idx2);
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

// ---- the same search on a KannalaBrandt8 pair (model 1 of camera_model.h): KannalaBrandt8::epipolarConstrain in place of the line test.
// The search on such a pair costs a double Jacobi per candidate that passes the two cheap tests, and few candidates do: left where the
// candidate is found, one lane of a row would run it while the other lanes of the wave wait (measured: the chain's search 0.52 ms against
// 0.025 ms on a pinhole pair).  So a workgroup of 16 rows works in three steps on a list in LDS:
//   1. every lane scans its candidates of its row's query: dist <= th_low, the epipole disc; a coarse search keeps the key at once,
//      otherwise the candidate joins the workgroup's list of survivors;
//   2. thread t takes survivor t -- its row's query (pixel, ray, KF1's sigma2: taken once per row by the row's first lane), its own
//      ray, KannalaBrandt8::epipolarConstrain -- and a survivor that passes lowers its row's key with an LDS atomic minimum;
//   3. the row's key is the minimum of what its lanes kept and what the list gave.
// A list that is full (kTriListCap survivors in one workgroup) sends further survivors through the constraint where they stand.
constexpr int kTriRows = 16, kTriListCap = 256;
struct TriRowQuery {             // what the constraint reads of a KF1 keypoint
  float u, v, rx, ry, sigma1;
  int32_t ok;                    // its octave lies inside KF1's tables (otherwise sigma1 is not read and only a coarse search takes it)
};
struct TriBlockKB8 {
  TriRowQuery q[kTriRows];
  uint32_t key[kTriRows];
  int32_t n;
  int32_t idx2[kTriListCap];
  uint32_t skey[kTriListCap];
  uint8_t row[kTriListCap];
};
__device__ __forceinline__ TriRowQuery tri_row_query(const dvm_keypoint_pod& kp1, const float* cam1, const float* __restrict__ level_sigma2_1, int n_levels) {
  TriRowQuery Q;
  Q.u = kp1.x; Q.v = kp1.y;
  Q.ok = (unsigned)kp1.octave < (unsigned)n_levels;
  Q.sigma1 = Q.ok ? level_sigma2_1[kp1.octave] : 0.f;
  float r[3];
  dvm_tri::unproject<dvm_cam::kKannalaBrandt8>(cam1, kp1.x, kp1.y, r);
  Q.rx = r[0]; Q.ry = r[1];
  return Q;
}
// KannalaBrandt8::epipolarConstrain of a query and a KF2 keypoint
__device__ __forceinline__ bool tri_constrain(const TriRowQuery& Q, const dvm_keypoint_pod& kp2, const TriGeomKB8& G, const float* __restrict__ level_sigma2_2) {
  if (!Q.ok) return false;
  const float r1[3] = {Q.rx, Q.ry, 1.f};
  float r2[3];
  dvm_tri::unproject<dvm_cam::kKannalaBrandt8>(G.cam2, kp2.x, kp2.y, r2);
  return dvm_tri::kb8_epipolar_constrain(G.cam1, G.cam2, r1, r2, Q.u, Q.v, kp2.x, kp2.y, G.R, Q.sigma1, level_sigma2_2[kp2.octave]);
}
// The three steps for the calling workgroup of 256 threads (every thread calls it: it holds workgroup barriers).  The row of this thread
// asks for KF1 keypoint idx1 over the candidate positions [beg, end) when `active`; cand_at(p) is the KF2 keypoint at position p or -1.
// Returns the row's key in every lane of the row: tri_key of the best candidate, 0xFFFFFFFF without one.
template <class CandAt>
__device__ __forceinline__ uint32_t tri_rows_kb8(TriBlockKB8& S, bool active, const uint8_t* __restrict__ desc1, const dvm_keypoint_pod* __restrict__ kps1,
                                                 int idx1, int beg, int end, CandAt cand_at, const uint8_t* __restrict__ desc2,
                                                 const dvm_keypoint_pod* __restrict__ kps2, const TriGeomKB8& G, const float* __restrict__ level_sigma2_1,
                                                 const float* __restrict__ scale_factors2, const float* __restrict__ level_sigma2_2, int n_levels) {
  const int lane = threadIdx.x & 15, row = threadIdx.x >> 4;
  if (threadIdx.x < kTriRows) S.key[threadIdx.x] = 0xFFFFFFFFu;
  if (threadIdx.x == 0) S.n = 0;
  __syncthreads();
  uint32_t key = 0xFFFFFFFFu;
  if (active && end > beg) {
    uint32_t w[8];
    desc_load(desc1, idx1, w);
    if (lane == 0 && !G.coarse) S.q[row] = tri_row_query(kps1[idx1], G.cam1, level_sigma2_1, n_levels);
    for (int p = beg + lane; p < end; p += 16) {
      const int idx2 = cand_at(p);
      if (idx2 < 0) continue;
      const int d = desc_distance(w, desc2, idx2);
      if (d > G.th_low) continue;
      const dvm_keypoint_pod kp2 = kps2[idx2];
      if ((unsigned)kp2.octave >= (unsigned)n_levels) continue;   // outside the tables: no candidate, nothing read
      const float distex = G.ep[0] - kp2.x, distey = G.ep[1] - kp2.y;
      if (distex * distex + distey * distey < 100.f * scale_factors2[kp2.octave]) continue;
      const uint32_t k = tri_key(d, p - beg);
      if (G.coarse) { key = min(key, k); continue; }
      const int slot = atomicAdd(&S.n, 1);
      if (slot < kTriListCap) {
        S.idx2[slot] = idx2; S.skey[slot] = k; S.row[slot] = (uint8_t)row;
      } else {                                                     // the list is full: this lane decides for itself
        const TriRowQuery Q = tri_row_query(kps1[idx1], G.cam1, level_sigma2_1, n_levels);
        if (tri_constrain(Q, kp2, G, level_sigma2_2)) key = min(key, k);
      }
    }
  }
  __syncthreads();
  const int ns = min(S.n, kTriListCap);
  for (int t = threadIdx.x; t < ns; t += 256) {
    const int idx2 = S.idx2[t], r = S.row[t];
    if (tri_constrain(S.q[r], kps2[idx2], G, level_sigma2_2)) atomicMin(&S.key[r], S.skey[t]);
  }
  __syncthreads();
  return min(row_min(key), S.key[row]);
}

// One match (kp1, kp2) of one neighbour under camera model MODEL (dvm_tri::pair_geometry, tri_model.h): the octave check, the two rays,
// then the shared body.  cam1 / cam2 = the cameras' parameters (the pinhole instantiation reads P.K1 / P.K2 and ignores them).  Returns
// the status (include/dvmslam_hip.h).
template <int MODEL = dvm_cam::kPinhole>
__device__ __forceinline__ int tri_pair_geometry(const TriPair& P, const dvm_keypoint_pod& kp1, const dvm_keypoint_pod& kp2,
                                                 const float* __restrict__ sigma2_1, const float* __restrict__ sigma2_2,
                                                 const float* __restrict__ sf1, const float* __restrict__ sf2, float* X,
                                                 const float* cam1 = nullptr, const float* cam2 = nullptr) {
  X[0] = X[1] = X[2] = 0.0f;
  if (kp1.octave < 0 || kp1.octave >= P.n_levels || kp2.octave < 0 || kp2.octave >= P.n_levels) return -1;
  if (MODEL == dvm_cam::kPinhole) { cam1 = P.K1; cam2 = P.K2; }
  float xn1[3], xn2[3];
  dvm_tri::unproject<MODEL>(cam1, kp1.x, kp1.y, xn1);
  dvm_tri::unproject<MODEL>(cam2, kp2.x, kp2.y, xn2);
  return dvm_tri::pair_geometry<MODEL>(P, kp1, kp2, xn1, xn2, cam1, cam2, sigma2_1, sigma2_2, sf1, sf2, X);
}

// The pinhole instantiation is the operation sequence the pinhole kernels have always compiled, statement for statement (dvm_tri::pair_geometry
// <kPinhole> is the same arithmetic; tests/test_kb8_tri_model.py holds the host build of that one against the float64 statement).
template <>
__device__ __forceinline__ int tri_pair_geometry<dvm_cam::kPinhole>(const TriPair& P, const dvm_keypoint_pod& kp1, const dvm_keypoint_pod& kp2,
                                                 const float* __restrict__ sigma2_1, const float* __restrict__ sigma2_2,
                                                 const float* __restrict__ sf1, const float* __restrict__ sf2, float* X, const float*, const float*) {
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
