// dvm_slam_amd/csrc/se3_f64.h -- the FP64 small algebra of the optimisers (ba_kernels.hip, ba_window_seq.hip, ba_window_cluster.hip, pose_kernels.hip, sim3_f64.h):
// quaternion <-> rotation, SE3 oplus, Huber, the 3x3 inverse.  ONE definition each: the sequential-order window kernels promise g2o's
// bits, so every expression keeps the oracle's order and every libm call is f64_spec.h's (-ffp-contract=off: one IEEE rounding each).
#pragma once
#include <hip/hip_runtime.h>

#include "f64_spec.h"

namespace dvm {

__device__ __forceinline__ void quat_to_R(const double* q, double* R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y,
               tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}
__device__ __forceinline__ void R_to_quat(const double* R, double* q) {      // Eigen's quaternion-from-matrix
  double t = R[0] + R[4] + R[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(R[i * 4] - R[j * 4] - R[k * 4] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t;
    q[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    q[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
  }
}
__device__ __forceinline__ void quat_normalize(double* q) {      // SE3Quat::normalizeRotation, se3quat.h:261-266
  if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}
__device__ __forceinline__ void mat3_vec(const double* R, const double* v, double* o) {
  o[0] = R[0] * v[0] + R[1] * v[1] + R[2] * v[2];
  o[1] = R[3] * v[0] + R[4] * v[1] + R[5] * v[2];
  o[2] = R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
}

// Tn = exp(u) * T, u = (omega, upsilon): SE3Quat::exp + operator* + normalizeRotation
// (reference Thirdparty/g2o/g2o/types/se3quat.h:212-266, types_six_dof_expmap.h:71-74).  Tn == T is allowed: all of T is read before
// the first write.
__device__ __forceinline__ void se3_oplus(const double* T, const double* u, double* Tn) {
  const double om0 = u[0], om1 = u[1], om2 = u[2];
  const double theta = sqrt(om0 * om0 + om1 * om1 + om2 * om2);
  const double O[9] = {0, -om2, om1, om2, 0, -om0, -om1, om0, 0};
  double O2[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) O2[3 * r + c] = O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c] + O[3 * r + 2] * O[6 + c];
  double R[9], Vm[9];
  if (theta < 0.00001) {
#pragma unroll
    for (int k = 0; k < 9; k++) { R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + O[k] + O2[k]; Vm[k] = R[k]; }
  } else {
    // sin / cos / pow(theta, 3) of SE3Quat::exp: the double-precision spec the oracle evaluates too (csrc/f64_spec.h), not the device libm
    const double sn = f64_sin(theta), cs = f64_cos(theta);
    const double a = sn / theta, bb = (1 - cs) / (theta * theta), c = (theta - sn) / f64_cube(theta);
#pragma unroll
    for (int k = 0; k < 9; k++) {
      const double I = (k % 4 == 0) ? 1.0 : 0.0;
      R[k] = I + a * O[k] + bb * O2[k];
      Vm[k] = I + bb * O[k] + c * O2[k];
    }
  }
  double dq[4], dt[3], Rd[9], rt[3], nq[4];
  R_to_quat(R, dq);
  quat_normalize(dq);
  mat3_vec(Vm, u + 3, dt);
  quat_to_R(dq, Rd);
  mat3_vec(Rd, T, rt);
  const double* q = T + 3;
  nq[3] = dq[3] * q[3] - dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2];
  nq[0] = dq[3] * q[0] + dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1];
  nq[1] = dq[3] * q[1] + dq[1] * q[3] + dq[2] * q[0] - dq[0] * q[2];
  nq[2] = dq[3] * q[2] + dq[2] * q[3] + dq[0] * q[1] - dq[1] * q[0];
  quat_normalize(nq);
  Tn[0] = dt[0] + rt[0]; Tn[1] = dt[1] + rt[1]; Tn[2] = dt[2] + rt[2];
  Tn[3] = nq[0]; Tn[4] = nq[1]; Tn[5] = nq[2]; Tn[6] = nq[3];
}

// Huber (robust_kernel_impl.cpp:68-81); delta <= 0 means "no robust kernel"
__device__ __forceinline__ void robustify(double e, double delta, double& rho0, double& rho1) {
  if (delta <= 0 || e <= delta * delta) { rho0 = e; rho1 = 1.; }
  else { const double s = sqrt(e); rho0 = 2 * s * delta - delta * delta; rho1 = delta / s; }
}

// 3x3 inverse by cofactors, the determinant along the first row: a landmark's damped Hll
__device__ __forceinline__ void inv3(const double* M, double* Inv) {
  const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
  const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
  const double id = 1.0 / det;
  Inv[0] = (e * i - f * h) * id; Inv[1] = (c * h - b * i) * id; Inv[2] = (b * f - c * e) * id;
  Inv[3] = (f * g - d * i) * id; Inv[4] = (a * i - c * g) * id; Inv[5] = (c * d - a * f) * id;
  Inv[6] = (d * h - e * g) * id; Inv[7] = (b * g - a * h) * id; Inv[8] = (a * e - b * d) * id;
}

}  // namespace dvm
