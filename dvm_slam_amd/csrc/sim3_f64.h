// dvm_slam_amd/csrc/sim3_f64.h -- g2o::Sim3 in double for the kernels that optimise over it: OptimizeSim3 (sim3_kernels.hip) and the
// essential graph (pg_kernels.hip).  exp / log as sim3.h writes them, with the device libm (neither kernel promises g2o's bits).
#pragma once
#include <hip/hip_runtime.h>

#include "camera_model.h"
#include "se3_f64.h"

namespace dvm {

struct Sim3d { double q[4]; double t[3]; double s; };
__device__ inline void sim3_exp(const double* u, Sim3d& S) {  // g2o::Sim3(const Vector7d&), sim3.h:62-125
  const double om0 = u[0], om1 = u[1], om2 = u[2], sigma = u[6];
  const double theta = sqrt(om0 * om0 + om1 * om1 + om2 * om2);
  const double O[9] = {0, -om2, om1, om2, 0, -om0, -om1, om0, 0};
  double O2[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
  S.s = exp(sigma);
  const double eps = 0.00001;
  double A, B, C, R[9];
  if (fabs(sigma) < eps) {
    C = 1;
    if (theta < eps) { A = 0.5; B = 1. / 6.; for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + O[i] + O2[i]; }
    else {
      const double th2 = theta * theta;
      A = (1 - cos(theta)) / th2; B = (theta - sin(theta)) / (th2 * theta);
      for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + sin(theta) / theta * O[i] + (1 - cos(theta)) / (theta * theta) * O2[i];
    }
  } else {
    C = (S.s - 1) / sigma;
    if (theta < eps) {
      const double s2 = sigma * sigma;
      A = ((sigma - 1) * S.s + 1) / s2; B = ((0.5 * s2 - sigma + 1) * S.s) / (s2 * sigma);
      for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + O[i] + O2[i];
    } else {
      for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + sin(theta) / theta * O[i] + (1 - cos(theta)) / (theta * theta) * O2[i];
      const double a = S.s * sin(theta), b = S.s * cos(theta), th2 = theta * theta, s2 = sigma * sigma, c = th2 + s2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / th2;
    }
  }
  R_to_quat(R, S.q);
  double W[9];
  for (int i = 0; i < 9; i++) W[i] = A * O[i] + B * O2[i] + C * ((i % 4 == 0) ? 1.0 : 0.0);
  mat3_vec(W, u + 3, S.t);
}
__device__ inline void sim3_mul(const Sim3d& a, const Sim3d& b, Sim3d& o) {
  const double* p = a.q; const double* q = b.q;
  o.q[3] = p[3] * q[3] - p[0] * q[0] - p[1] * q[1] - p[2] * q[2];
  o.q[0] = p[3] * q[0] + p[0] * q[3] + p[1] * q[2] - p[2] * q[1];
  o.q[1] = p[3] * q[1] + p[1] * q[3] + p[2] * q[0] - p[0] * q[2];
  o.q[2] = p[3] * q[2] + p[2] * q[3] + p[0] * q[1] - p[1] * q[0];
  double R[9], rt[3];
  quat_to_R(a.q, R);
  mat3_vec(R, b.t, rt);
  for (int i = 0; i < 3; i++) o.t[i] = a.s * rt[i] + a.t[i];
  o.s = a.s * b.s;
}
__device__ inline void sim3_inv(const Sim3d& a, Sim3d& o) {
  o.q[0] = -a.q[0]; o.q[1] = -a.q[1]; o.q[2] = -a.q[2]; o.q[3] = a.q[3];
  double R[9];
  const double v[3] = {(-1. / a.s) * a.t[0], (-1. / a.s) * a.t[1], (-1. / a.s) * a.t[2]};
  quat_to_R(o.q, R);
  mat3_vec(R, v, o.t);
  o.s = 1. / a.s;
}
struct Sim3M { double R[9]; double t[3]; double s; };  // map-ready form: x -> s R x + t
__device__ __forceinline__ void sim3_to_map(const Sim3d& a, Sim3M& m) {
  quat_to_R(a.q, m.R);
  m.t[0] = a.t[0]; m.t[1] = a.t[1]; m.t[2] = a.t[2]; m.s = a.s;
}
__device__ __forceinline__ void sim3_proj(const Sim3M& m, const double* x, const double* K, double& u, double& v) {
  double rx[3];
  mat3_vec(m.R, x, rx);
  const double X = m.s * rx[0] + m.t[0], Y = m.s * rx[1] + m.t[1], Z = m.s * rx[2] + m.t[2];
  u = K[0] * X / Z + K[2];
  v = K[1] * Y / Z + K[3];
}
// sim3_proj on a camera model (camera_model.h): M == 0 is sim3_proj itself; KannalaBrandt8 projects with p = mvParameters, through the
// reference's project(Vector3d) (float theta: residuals and chi2 tests) or, EXACT, through the double atan2 (numeric Jacobians).
template <int M, bool EXACT>
__device__ __forceinline__ void sim3_proj_cam(const Sim3M& m, const double* x, const double* K, const float* p, double& u, double& v) {
  if constexpr (M == dvm_cam::kPinhole) sim3_proj(m, x, K, u, v);
  else {
    double rx[3];
    mat3_vec(m.R, x, rx);
    const double X = m.s * rx[0] + m.t[0], Y = m.s * rx[1] + m.t[1], Z = m.s * rx[2] + m.t[2];
    if constexpr (EXACT) dvm_cam::kb8_project_exact(p, X, Y, Z, u, v);
    else dvm_cam::kb8_project(p, X, Y, Z, u, v);
  }
}
__device__ inline void sim3_log(const Sim3d& S, double* res) {   // g2o Sim3::log, sim3.h:128-197
  const double sigma = log(S.s);
  double R[9];
  quat_to_R(S.q, R);
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  double omega[3];
  const double eps = 0.00001;
  double A, B, C;
  if (fabs(sigma) < eps) {
    C = 1;
    if (d > 1 - eps) { for (int i = 0; i < 3; i++) omega[i] = 0.5 * dR[i]; A = 1. / 2.; B = 1. / 6.; }
    else {
      const double theta = acos(d), theta2 = theta * theta;
      for (int i = 0; i < 3; i++) omega[i] = theta / (2 * sqrt(1 - d * d)) * dR[i];
      A = (1 - cos(theta)) / theta2; B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    C = (S.s - 1) / sigma;
    if (d > 1 - eps) {
      const double sigma2 = sigma * sigma;
      for (int i = 0; i < 3; i++) omega[i] = 0.5 * dR[i];
      A = ((sigma - 1) * S.s + 1) / sigma2; B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
    } else {
      const double theta = acos(d);
      for (int i = 0; i < 3; i++) omega[i] = theta / (2 * sqrt(1 - d * d)) * dR[i];
      const double theta2 = theta * theta, a = S.s * sin(theta), b = S.s * cos(theta), c = theta2 + sigma * sigma;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
    }
  }
  const double O[9] = {0, -omega[2], omega[1], omega[2], 0, -omega[0], -omega[1], omega[0], 0};
  double W[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double o2 = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
      W[3 * i + j] = A * O[3 * i + j] + B * o2 + C * (i == j ? 1.0 : 0.0);
    }
  const double c00 = W[4] * W[8] - W[5] * W[7], c01 = W[5] * W[6] - W[3] * W[8], c02 = W[3] * W[7] - W[4] * W[6];
  const double det = W[0] * c00 + W[1] * c01 + W[2] * c02;
  const double inv[9] = {c00, W[2] * W[7] - W[1] * W[8], W[1] * W[5] - W[2] * W[4],
                         c01, W[0] * W[8] - W[2] * W[6], W[2] * W[3] - W[0] * W[5],
                         c02, W[1] * W[6] - W[0] * W[7], W[0] * W[4] - W[1] * W[3]};
  for (int i = 0; i < 3; i++) res[i] = omega[i];
  for (int i = 0; i < 3; i++) res[3 + i] = (inv[3 * i] * S.t[0] + inv[3 * i + 1] * S.t[1] + inv[3 * i + 2] * S.t[2]) / det;
  res[6] = sigma;
}
__device__ __forceinline__ void sim3_load(const double* p, Sim3d& S) {
  S.q[0] = p[0]; S.q[1] = p[1]; S.q[2] = p[2]; S.q[3] = p[3]; S.t[0] = p[4]; S.t[1] = p[5]; S.t[2] = p[6]; S.s = p[7];
}

}  // namespace dvm
