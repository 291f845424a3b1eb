// dvm_slam_amd/csrc/sim3_kernels.hip -- loop closing's Sim3 estimation on the device, FP64 / FP32, for gfx950:
//   B9  k_optimize_sim3      Optimizer::OptimizeSim3: one workgroup, dense 7x7 Levenberg with g2o's numeric Jacobians
//       k_sim3_hypotheses    Sim3Solver: one wave per RANSAC hypothesis (Horn's closed form + inlier count)
// Both are templates over the camera models of the two keyframes (camera_model.h: 0 pinhole, 1 KannalaBrandt8), instantiated for the four pairs.
// g2o::Sim3 itself is sim3_f64.h's, the 36-value reduction reduce_f64.h's.  Launchers: ba_kernels.h.
#include <hip/hip_runtime.h>

#include "ba_kernels.h"
#include "jacobi4.h"
#include "reduce_f64.h"
#include "sim3_f64.h"

namespace dvm {

// ---------------------------------------------------------------------------------------- B9
// Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1960-2212): one 7-DoF g2o::Sim3 vertex, two
// reprojection edges per correspondence (EdgeSim3ProjectXYZ, EdgeInverseSim3ProjectXYZ) whose Jacobians
// g2o takes NUMERICALLY (central differences, delta 1e-9, base_binary_edge.hpp:131-205) because the
// analytic linearizeOplus is commented out (include/OptimizableTypes.h:186,205); dense 7x7 Levenberg,
// optimize(5), inlier test chi2 <= th2, robust kernel off, optimize(5 or 10), final inlier count.
// One workgroup runs everything; the 14 perturbed Sim3 states (and inverses) are shared by all edges.
//
// M1 / M2 = the camera model of keyframe 1 / 2 (camera_model.h; the reference's edges call pCamera1->project / pCamera2->project,
// OptimizableTypes.h:183, 202), one instantiation per pair.  <0, 0> is the pinhole kernel: camp is not read.  A KannalaBrandt8 side
// takes its eight parameters from camp[0..7] (camera 1) / camp[8..15] (camera 2) and splits the projection in two:
//   residual, chi2, both inlier tests   kb8_project(double): the reference's project(Vector3d), theta from the FLOAT atan2f;
//   the central differences             kb8_project_exact: theta from the double atan2, same 28 perturbed states, same delta.
// Through the float theta the residual is a staircase with steps of one float ulp of theta (~3e-8 rad): a perturbation of 1e-9 crosses
// a step in a few per cent of the evaluations and then reads ~1e-5 px / 2e-9, so g2o's numeric Jacobian of a fisheye edge is 0 almost
// everywhere with spikes of thousands of px per unit, decided by libm's last bit of atan2f.  Nothing can be pinned to that; the smooth
// projection is the function projectJac differentiates (bundle adjustment on a camera model splits residual and Jacobian the same way).
template <int M1, int M2>
__global__ void __launch_bounds__(256) k_optimize_sim3(double* __restrict__ S12io, int fix_scale, const double* __restrict__ P1c,
                                                       const double* __restrict__ P2c, const double* __restrict__ obs1,
                                                       const double* __restrict__ obs2, const double* __restrict__ w1,
                                                       const double* __restrict__ w2, int N, const double* __restrict__ Kio,
                                                       const float* __restrict__ camp, double th2, uint8_t* __restrict__ inlier,
                                                       int32_t* __restrict__ nin_out, double* __restrict__ chi_scratch,
                                                       uint8_t* __restrict__ flag_scratch) {
  __shared__ double s_park[256 * 37];   // the 36 sums of a Jacobian pass in ONE pass through LDS
  __shared__ double s_part[4 * 36];
  __shared__ double s_sum[36];
  __shared__ Sim3d s_S, s_bak;
  __shared__ Sim3M s_M[30];   // [0] S, [1] S^-1, [2+2d] S+d, [3+2d] (S+d)^-1, [16+2d] S-d, [17+2d] (S-d)^-1
  __shared__ double s_K[8];
  __shared__ float s_p[16];
  __shared__ double s_lambda, s_ni, s_cur, s_ini, s_rho;
  __shared__ int s_ctl, s_qmax, s_nbad, s_cnt;
  const int tid = threadIdx.x;
  double* chi12 = chi_scratch;
  double* chi21 = chi_scratch + N;
  uint8_t* alive = flag_scratch;
  uint8_t* robust = flag_scratch + N;
  if (tid < 8) s_K[tid] = Kio[tid];
  if constexpr (M1 != 0 || M2 != 0) { if (tid < 16) s_p[tid] = camp[tid]; }
  if (tid == 0) {
    for (int i = 0; i < 4; i++) s_S.q[i] = S12io[i];
    for (int i = 0; i < 3; i++) s_S.t[i] = S12io[4 + i];
    s_S.s = S12io[7];
  }
  for (int i = tid; i < N; i += 256) { alive[i] = 1; robust[i] = 1; inlier[i] = 0; chi12[i] = 0; chi21[i] = 0; }
  __syncthreads();
  const double deltaHuber = (double)sqrtf((float)th2);

  // refreshes s_M[0..1] (jac=false) or all 30 maps (jac=true) from s_S
  auto prepare = [&](bool jac) {
    if (tid == 0) { sim3_to_map(s_S, s_M[0]); Sim3d Si; sim3_inv(s_S, Si); sim3_to_map(Si, s_M[1]); }
    if (jac && tid >= 64 && tid < 78) {
      const int k = tid - 64, d = k >> 1, sgn = k & 1;
      double u[7] = {0, 0, 0, 0, 0, 0, 0};
      u[d] = sgn ? -1e-9 : 1e-9;
      if (fix_scale) u[6] = 0;
      Sim3d E, Sx, Sxi;
      sim3_exp(u, E);
      sim3_mul(E, s_S, Sx);
      sim3_inv(Sx, Sxi);
      sim3_to_map(Sx, s_M[(sgn ? 16 : 2) + 2 * d]);
      sim3_to_map(Sxi, s_M[(sgn ? 17 : 3) + 2 * d]);
    }
    __syncthreads();
  };
  auto eval = [&](bool jac) {
    prepare(jac);
    double acc[36];
#pragma unroll
    for (int i = 0; i < 36; i++) acc[i] = 0;
    for (int i = tid; i < N; i += 256) {
      if (!alive[i]) continue;
      const double* x1 = P1c + 3 * i; const double* x2 = P2c + 3 * i;
      double u, v;
      sim3_proj_cam<M1, false>(s_M[0], x2, s_K, s_p, u, v);
      const double a0 = obs1[2 * i] - u, a1 = obs1[2 * i + 1] - v;
      sim3_proj_cam<M2, false>(s_M[1], x1, s_K + 4, s_p + 8, u, v);
      const double b0 = obs2[2 * i] - u, b1 = obs2[2 * i + 1] - v;
      const double c12 = w1[i] * (a0 * a0 + a1 * a1), c21 = w2[i] * (b0 * b0 + b1 * b1);
      chi12[i] = c12; chi21[i] = c21;
      const double dl = robust[i] ? deltaHuber : 0.0;
      double r0a, r1a, r0b, r1b;
      robustify(c12, dl, r0a, r1a);
      robustify(c21, dl, r0b, r1b);
      acc[35] += r0a;
      acc[35] += r0b;
      if (jac) {
        double J12[14], J21[14];
#pragma unroll
        for (int d = 0; d < 7; d++) {
          double up, vp, um, vm;
          sim3_proj_cam<M1, true>(s_M[2 + 2 * d], x2, s_K, s_p, up, vp); sim3_proj_cam<M1, true>(s_M[16 + 2 * d], x2, s_K, s_p, um, vm);
          // e(+d) - e(-d) = (obs - proj+) - (obs - proj-)
          J12[d] = 5e8 * ((obs1[2 * i] - up) - (obs1[2 * i] - um)); J12[7 + d] = 5e8 * ((obs1[2 * i + 1] - vp) - (obs1[2 * i + 1] - vm));
          sim3_proj_cam<M2, true>(s_M[3 + 2 * d], x1, s_K + 4, s_p + 8, up, vp); sim3_proj_cam<M2, true>(s_M[17 + 2 * d], x1, s_K + 4, s_p + 8, um, vm);
          J21[d] = 5e8 * ((obs2[2 * i] - up) - (obs2[2 * i] - um)); J21[7 + d] = 5e8 * ((obs2[2 * i + 1] - vp) - (obs2[2 * i + 1] - vm));
        }
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
          const double* J = pass ? J21 : J12;
          const double e0 = pass ? b0 : a0, e1 = pass ? b1 : a1, w0 = pass ? w2[i] : w1[i], r1 = pass ? r1b : r1a;
          const double w = r1 * w0, wr0 = -w0 * e0 * r1, wr1 = -w0 * e1 * r1;
          int t = 0;
#pragma unroll
          for (int p = 0; p < 7; p++) {
            acc[28 + p] += J[p] * wr0 + J[7 + p] * wr1;
#pragma unroll
            for (int q = 0; q <= p; q++) acc[t++] += w * (J[p] * J[q] + J[7 + p] * J[7 + q]);
          }
        }
      }
    }
    if (jac) block_sum_lds<36>(acc, s_park, s_part, s_sum);
    else {          // a trial's chi2: one value (the full reduction here cost ~2 us per LM trial)
      const double c = block_sum_one(acc[35], s_part);
      if (tid == 0) s_sum[35] = c;
      __syncthreads();
    }
  };
  auto optimize = [&](int iters) {
    for (int it = 0; it < iters; it++) {
      eval(true);
      double Hs[28], bs[7], xs[7];
      if (tid == 0) {
        s_cur = s_sum[35]; s_ini = s_sum[35];
        for (int i = 0; i < 28; i++) Hs[i] = s_sum[i];
        for (int i = 0; i < 7; i++) bs[i] = s_sum[28 + i];
        if (it == 0) {
          double mx = 0;
          for (int p = 0; p < 7; p++) mx = fmax(mx, fabs(Hs[p * (p + 1) / 2 + p]));
          s_lambda = 1e-5 * mx; s_ni = 2; s_nbad = 0;
        }
        s_qmax = 0;
      }
      __syncthreads();
      while (true) {
        if (tid == 0) {
          s_bak = s_S;
          // dense 7x7 Cholesky; ri[j] = 1 / L_jj by v_rsq_f64 + two Newton steps: no double-precision division or square root on
          // this single lane (35 of them before: ~3 us per LM trial)
          double Lm[28], ri[7];
          bool ok = true;
#pragma unroll
          for (int i = 0; i < 7; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
              double sacc = Hs[i * (i + 1) / 2 + j] + (i == j ? s_lambda : 0.0);
#pragma unroll
              for (int k = 0; k < j; k++) sacc -= Lm[i * (i + 1) / 2 + k] * Lm[j * (j + 1) / 2 + k];
              if (i == j) {
                if (!(sacc > 0)) ok = false;
                const double dd = sacc > 0 ? sacc : 1.0;
                double y = __builtin_amdgcn_rsq(dd);
                y = __builtin_fma(0.5 * y, __builtin_fma(-dd * y, y, 1.0), y);
                y = __builtin_fma(0.5 * y, __builtin_fma(-dd * y, y, 1.0), y);
                double sq = dd * y;
                sq = __builtin_fma(0.5 * y, __builtin_fma(-sq, sq, dd), sq);
                Lm[i * (i + 1) / 2 + i] = sq; ri[i] = y;
              } else Lm[i * (i + 1) / 2 + j] = sacc * ri[j];
            }
          if (ok) {
#pragma unroll
            for (int i = 0; i < 7; i++) {
              double sacc = bs[i];
#pragma unroll
              for (int k = 0; k < i; k++) sacc -= Lm[i * (i + 1) / 2 + k] * xs[k];
              xs[i] = sacc * ri[i];
            }
#pragma unroll
            for (int i = 6; i >= 0; i--) {
              double sacc = xs[i];
#pragma unroll
              for (int k = i + 1; k < 7; k++) sacc -= Lm[k * (k + 1) / 2 + i] * xs[k];
              xs[i] = sacc * ri[i];
            }
            double u[7];
            for (int i = 0; i < 7; i++) u[i] = xs[i];
            if (fix_scale) u[6] = 0;
            Sim3d E, Sn;
            sim3_exp(u, E);
            sim3_mul(E, s_S, Sn);
            s_S = Sn;
          }
          s_ctl = ok ? 1 : 0;
        }
        __syncthreads();
        const bool okb = s_ctl != 0;
        if (okb) eval(false);
        if (tid == 0) {
          const double tempChi = okb ? s_sum[35] : 1.7976931348623157e308;
          double rho = s_cur - tempChi;
          double scale = 0;
          if (okb) for (int j = 0; j < 7; j++) scale += xs[j] * (s_lambda * xs[j] + bs[j]);
          scale += 1e-3;
          rho /= scale;
          if (rho > 0 && isfinite(tempChi)) {
            double alpha = 1. - f64_cube(2 * rho - 1);   // pow(2 rho - 1, 3) as the shared double-precision spec forms it (f64_spec.h)
            alpha = fmin(alpha, 2. / 3.);
            s_lambda *= fmax(1. / 3., alpha);
            s_ni = 2;
            s_cur = tempChi;
          } else {
            s_lambda *= s_ni; s_ni *= 2;
            s_S = s_bak;
          }
          s_qmax++;
          s_rho = rho;
          s_ctl = (rho < 0 && s_qmax < 10) ? 1 : 0;
        }
        __syncthreads();
        const int again = s_ctl;
        __syncthreads();
        if (!again) break;
      }
      if (tid == 0) {
        int stop = 0;
        if (s_qmax == 10 || s_rho == 0) stop = 1;
        else {
          if ((s_ini - s_cur) * 1e3 < s_ini) s_nbad++; else s_nbad = 0;
          if (s_nbad >= 3) stop = 1;
        }
        s_ctl = stop;
      }
      __syncthreads();
      const int stop = s_ctl;
      __syncthreads();
      if (stop) break;
    }
  };

  optimize(5);
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  int bad = 0;
  for (int i = tid; i < N; i += 256) {
    if (chi12[i] > th2 || chi21[i] > th2) { alive[i] = 0; bad++; } else robust[i] = 0;
  }
  if (bad) atomicAdd(&s_cnt, bad);
  __syncthreads();
  const int nBad = s_cnt;
  __syncthreads();
  if (N - nBad < 10) {
    if (tid == 0) *nin_out = 0;
    return;
  }
  optimize(nBad > 0 ? 10 : 5);
  prepare(false);
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  int in = 0;
  for (int i = tid; i < N; i += 256) {
    if (!alive[i]) continue;
    double u, v;
    sim3_proj_cam<M1, false>(s_M[0], P2c + 3 * i, s_K, s_p, u, v);
    const double a0 = obs1[2 * i] - u, a1 = obs1[2 * i + 1] - v;
    sim3_proj_cam<M2, false>(s_M[1], P1c + 3 * i, s_K + 4, s_p + 8, u, v);
    const double b0 = obs2[2 * i] - u, b1 = obs2[2 * i + 1] - v;
    const double c12 = w1[i] * (a0 * a0 + a1 * a1), c21 = w2[i] * (b0 * b0 + b1 * b1);
    if (!(c12 > th2 || c21 > th2)) { inlier[i] = 1; in++; }
  }
  if (in) atomicAdd(&s_cnt, in);
  __syncthreads();
  if (tid == 0) {
    *nin_out = s_cnt;
    for (int i = 0; i < 4; i++) S12io[i] = s_S.q[i];
    for (int i = 0; i < 3; i++) S12io[4 + i] = s_S.t[i];
    S12io[7] = s_S.s;
  }
}

void ba_launch_optimize_sim3_cam(hipStream_t s, double* S12io, int fix_scale, const double* P1c, const double* P2c,
                                 const double* obs1, const double* obs2, const double* w1, const double* w2, int N, const double* K,
                                 const float* camp, int model1, int model2, double th2, uint8_t* inlier, int32_t* nin,
                                 double* chi_scratch, uint8_t* flag_scratch) {
#define DVM_SIM3_OPT(A, B)                                                                                                          \
  hipLaunchKernelGGL((k_optimize_sim3<A, B>), dim3(1), dim3(256), 0, s, S12io, fix_scale, P1c, P2c, obs1, obs2, w1, w2, N, K, camp, \
                     th2, inlier, nin, chi_scratch, flag_scratch)
  if (model1 == 0 && model2 == 0) DVM_SIM3_OPT(0, 0);
  else if (model1 == 0) DVM_SIM3_OPT(0, 1);
  else if (model2 == 0) DVM_SIM3_OPT(1, 0);
  else DVM_SIM3_OPT(1, 1);
#undef DVM_SIM3_OPT
}

void ba_launch_optimize_sim3(hipStream_t s, double* S12io, int fix_scale, const double* P1c, const double* P2c,
                             const double* obs1, const double* obs2, const double* w1, const double* w2, int N,
                             const double* K, double th2, uint8_t* inlier, int32_t* nin, double* chi_scratch, uint8_t* flag_scratch) {
  ba_launch_optimize_sim3_cam(s, S12io, fix_scale, P1c, P2c, obs1, obs2, w1, w2, N, K, nullptr, 0, 0, th2, inlier, nin, chi_scratch,
                              flag_scratch);
}

// ------------------------------------------------------------------------------------------ Sim3Solver
// Sim3Solver::ComputeSim3 (Horn 1987 closed form, reference src/Sim3Solver.cc:294-385) + CheckInliers (:387-408) for
// a batch of RANSAC hypotheses, one wavefront each: the 3-point solve is wave-uniform (every lane computes it, no
// communication), the N correspondences are strided over the lanes, inliers counted by ballots.  The minimal sets are
// input (the reference draws them with DUtils::Random).  float / double split as in the reference except the 4x4
// eigen-decomposition: cyclic Jacobi in double ("Horn spec", same as the oracle) instead of Eigen::EigenSolver<float>.
// (jacobi4_dev: jacobi4.h)
// M1 / M2 = the camera model of keyframe 1 / 2: the four projections of CheckInliers and FromCameraToImage go through
// pCamera1->project / pCamera2->project(Vector3f) (Sim3Solver.cc:393-394, 422-446), all float.  A KannalaBrandt8 side reads its
// parameters from camp[0..7] / camp[8..15]; <0, 0> does not read camp.  Horn's closed form reads no camera: T12 has the same bits
// under every pair.

// pCamera->project(Vector3f) of model M: K = fx, fy, cx, cy (pinhole), p = mvParameters (KannalaBrandt8)
template <int M>
__device__ __forceinline__ void sim3_project_f32(const float* K, const float* p, const float* X, float& u, float& v) {
  if constexpr (M == dvm_cam::kKannalaBrandt8) dvm_cam::kb8_project(p, X[0], X[1], X[2], u, v);
  else { u = K[0] * X[0] / X[2] + K[2]; v = K[1] * X[1] / X[2] + K[3]; }
}

template <int M1, int M2>
__global__ void __launch_bounds__(64) k_sim3_hypotheses(const float* __restrict__ P1c, const float* __restrict__ P2c,
                                                        const float* __restrict__ max_err1, const float* __restrict__ max_err2,
                                                        int N, const float* __restrict__ K, const float* __restrict__ camp,
                                                        const int32_t* __restrict__ triples, int H, int fix_scale,
                                                        float* __restrict__ T12, int32_t* __restrict__ n_inliers,
                                                        uint8_t* __restrict__ mask) {
  const int h = blockIdx.x, lane = threadIdx.x;
  if (h >= H) return;
  float P1[3][3], P2[3][3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const int idx = triples[3 * h + c];
#pragma unroll
    for (int r = 0; r < 3; r++) { P1[r][c] = P1c[3 * idx + r]; P2[r][c] = P2c[3 * idx + r]; }
  }
  float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    O1[r] = ((P1[r][0] + P1[r][1]) + P1[r][2]) / 3.0f; O2[r] = ((P2[r][0] + P2[r][1]) + P2[r][2]) / 3.0f;
#pragma unroll
    for (int c = 0; c < 3; c++) { Pr1[r][c] = P1[r][c] - O1[r]; Pr2[r][c] = P2[r][c] - O2[r]; }
  }
  float M[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) M[r][c] = (Pr2[r][0] * Pr1[c][0] + Pr2[r][1] * Pr1[c][1]) + Pr2[r][2] * Pr1[c][2];
  const float N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0];
  const float N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2];
  const float N33 = -M[0][0] + M[1][1] - M[2][2], N34 = M[1][2] + M[2][1], N44 = -M[0][0] - M[1][1] + M[2][2];
  double A[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}}, V[4][4];
  jacobi4_dev(A, V);
  int mi = 0;
#pragma unroll
  for (int k = 1; k < 4; k++) if (A[k][k] > A[mi][mi]) mi = k;
  double q0 = V[0][0], vx = V[1][0], vy = V[2][0], vz = V[3][0];
#pragma unroll
  for (int k = 1; k < 4; k++) if (mi == k) { q0 = V[0][k]; vx = V[1][k]; vy = V[2][k]; vz = V[3][k]; }
  const double vn = sqrt(vx * vx + vy * vy + vz * vz);
  const double ang = atan2(vn, q0);
  float R[3][3];
  {
    double ax = 0, ay = 0, az = 0;
    if (vn > 0) { ax = vx / vn; ay = vy / vn; az = vz / vn; }
    const double w = cos(ang), sh = sin(ang), x = sh * ax, y = sh * ay, z = sh * az;
    R[0][0] = (float)(1 - 2 * (y * y + z * z)); R[0][1] = (float)(2 * (x * y - z * w)); R[0][2] = (float)(2 * (x * z + y * w));
    R[1][0] = (float)(2 * (x * y + z * w)); R[1][1] = (float)(1 - 2 * (x * x + z * z)); R[1][2] = (float)(2 * (y * z - x * w));
    R[2][0] = (float)(2 * (x * z - y * w)); R[2][1] = (float)(2 * (y * z + x * w)); R[2][2] = (float)(1 - 2 * (x * x + y * y));
  }
  float P3[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) P3[r][c] = (R[r][0] * Pr2[0][c] + R[r][1] * Pr2[1][c]) + R[r][2] * Pr2[2][c];
  float sc = 1.0f;
  if (!fix_scale) {
    float nom = 0, den = 0;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int r = 0; r < 3; r++) { nom += Pr1[r][c] * P3[r][c]; den += P3[r][c] * P3[r][c]; }
    sc = (float)((double)nom / (double)den);
  }
  float t[3], sR[3][3], sRi[3][3], ti[3];
#pragma unroll
  for (int r = 0; r < 3; r++) t[r] = O1[r] - ((sc * R[r][0]) * O2[0] + (sc * R[r][1]) * O2[1] + (sc * R[r][2]) * O2[2]);
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) { sR[r][c] = sc * R[r][c]; sRi[r][c] = (float)((1.0 / sc) * R[c][r]); }
#pragma unroll
  for (int r = 0; r < 3; r++) ti[r] = (-sRi[r][0] * t[0] + -sRi[r][1] * t[1]) + -sRi[r][2] * t[2];
  if (lane == 0) {
    float* out = T12 + 13 * (size_t)h;
    out[0] = sc;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) out[1 + 3 * r + c] = R[r][c];
#pragma unroll
    for (int r = 0; r < 3; r++) out[10 + r] = t[r];
  }
  const float Ka[4] = {K[0], K[1], K[2], K[3]}, Kb[4] = {K[4], K[5], K[6], K[7]};
  float pa[8], pb[8];
#pragma unroll
  for (int k = 0; k < 8; k++) { pa[k] = M1 != 0 ? camp[k] : 0.0f; pb[k] = M2 != 0 ? camp[8 + k] : 0.0f; }
  int nin = 0;
  for (int base = 0; base < N; base += 64) {
    const int i = base + lane;
    bool in = false;
    if (i < N) {
      const float X1[3] = {P1c[3 * i], P1c[3 * i + 1], P1c[3 * i + 2]}, X2[3] = {P2c[3 * i], P2c[3 * i + 1], P2c[3 * i + 2]};
      float a[3], b[3];
#pragma unroll
      for (int r = 0; r < 3; r++) {
        a[r] = ((sR[r][0] * X2[0] + sR[r][1] * X2[1]) + sR[r][2] * X2[2]) + t[r];
        b[r] = ((sRi[r][0] * X1[0] + sRi[r][1] * X1[1]) + sRi[r][2] * X1[2]) + ti[r];
      }
      float p1x, p1y, p2x, p2y, u1, v1, u2, v2;
      sim3_project_f32<M1>(Ka, pa, X1, p1x, p1y);   // FromCameraToImage
      sim3_project_f32<M2>(Kb, pb, X2, p2x, p2y);
      sim3_project_f32<M1>(Ka, pa, a, u1, v1);
      sim3_project_f32<M2>(Kb, pb, b, u2, v2);
      const float d1x = p1x - u1, d1y = p1y - v1, d2x = u2 - p2x, d2y = v2 - p2y;
      const float err1 = d1x * d1x + d1y * d1y, err2 = d2x * d2x + d2y * d2y;
      in = err1 < max_err1[i] && err2 < max_err2[i];
      mask[(size_t)h * N + i] = in ? 1 : 0;
    }
    nin += __popcll(__ballot(in));
  }
  if (lane == 0) n_inliers[h] = nin;
}

void ba_launch_sim3_hypotheses_cam(hipStream_t s, const float* P1c, const float* P2c, const float* e1, const float* e2, int N,
                                   const float* K, const float* camp, int model1, int model2, const int32_t* triples, int H,
                                   int fix_scale, float* T12, int32_t* nin, uint8_t* mask) {
  if (H <= 0) return;
#define DVM_SIM3_HYP(A, B)                                                                                                        \
  hipLaunchKernelGGL((k_sim3_hypotheses<A, B>), dim3(H), dim3(64), 0, s, P1c, P2c, e1, e2, N, K, camp, triples, H, fix_scale, T12, \
                     nin, mask)
  if (model1 == 0 && model2 == 0) DVM_SIM3_HYP(0, 0);
  else if (model1 == 0) DVM_SIM3_HYP(0, 1);
  else if (model2 == 0) DVM_SIM3_HYP(1, 0);
  else DVM_SIM3_HYP(1, 1);
#undef DVM_SIM3_HYP
}

void ba_launch_sim3_hypotheses(hipStream_t s, const float* P1c, const float* P2c, const float* e1, const float* e2, int N,
                               const float* K, const int32_t* triples, int H, int fix_scale, float* T12, int32_t* nin, uint8_t* mask) {
  ba_launch_sim3_hypotheses_cam(s, P1c, P2c, e1, e2, N, K, nullptr, 0, 0, triples, H, fix_scale, T12, nin, mask);
}

}  // namespace dvm
