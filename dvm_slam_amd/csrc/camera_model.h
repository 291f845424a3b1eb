// dvm_slam_amd/csrc/camera_model.h -- the camera models of the reference's GeometricCamera, for kernels and host mirrors: Pinhole
// (CameraModels/Pinhole.cpp) and KannalaBrandt8 (CameraModels/KannalaBrandt8.cpp:31-172), restated from their formulas.
//
// Parameters are dvm_camera_model::p = mvParameters, float as the reference stores them: fx, fy, cx, cy, k1, k2, k3, k4.
// KannalaBrandt8 with (x, y, z) in the camera frame:
//     theta = atan2(sqrt(x^2 + y^2), z),  psi = atan2(y, x),  r = theta + k1 theta^3 + k2 theta^5 + k3 theta^7 + k4 theta^9,
//     u = fx r cos(psi) + cx,  v = fy r sin(psi) + cy.
// cos(psi) and sin(psi) are taken as x / rho and y / rho (rho = sqrt(x^2 + y^2)), and as 1 and 0 on the optical axis, where
// atan2(0, 0) = 0: no trigonometric call, and up to the rounding of psi the same number.
// Every function needs -ffp-contract=off on its translation unit (both Makefiles set it).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DVM_CAM_HD __host__ __device__ __forceinline__
#else
#define DVM_CAM_HD inline
#endif

namespace dvm_cam {

constexpr int kPinhole = 0, kKannalaBrandt8 = 1;
// what every *_cam entry asks of a dvm_camera_model before anything runs: a known model and non-zero focal lengths
DVM_CAM_HD bool model_ok(int model, const float* p) { return (model == kPinhole || model == kKannalaBrandt8) && p[0] != 0.0f && p[1] != 0.0f; }

// The radial polynomial r(theta) = theta + k1 theta^3 + k2 theta^5 + k3 theta^7 + k4 theta^9 as the reference's three project overloads
// sum it: the odd powers built by repeated multiplication with theta^2, the terms added left to right.  T = float or double; k = p + 4.
template <class T>
DVM_CAM_HD T kb8_radius(const float* k, T theta) {
  const T t2 = theta * theta;
  T pw = theta * t2;       // theta^3, then ^5, ^7, ^9
  T r = theta;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    r = r + (T)k[i] * pw;
    pw = pw * t2;
  }
  return r;
}

// project(Vector3f): everything in float.  The matcher and frustum sites.
DVM_CAM_HD void kb8_project(const float* p, float x, float y, float z, float& u, float& v) {
  const float rho = sqrtf(x * x + y * y);
  const float r = kb8_radius<float>(p + 4, atan2f(rho, z));
  const bool axis = !(rho > 0.0f);
  const float c = axis ? 1.0f : x / rho, s = axis ? 0.0f : y / rho;
  u = p[0] * r * c + p[2];
  v = p[1] * r * s + p[3];
}

// project(Vector3d), what the optimiser's residual is made of.  The reference evaluates theta with the FLOAT atan2f / sqrtf here too
// (x^2 + y^2 and z rounded to float on the way in) and only the polynomial and the trigonometry in double: kept, so the residual is
// quantised in theta -- it moves in steps of one float ulp of theta (about 1e-7 rad, some 3e-5 px at fx = 500).
DVM_CAM_HD void kb8_project(const float* p, double x, double y, double z, double& u, double& v) {
  const double rho2 = x * x + y * y;
  const double r = kb8_radius<double>(p + 4, (double)atan2f(sqrtf((float)rho2), (float)z));
  const double rho = sqrt(rho2);
  const bool axis = !(rho > 0.0);
  const double c = axis ? 1.0 : x / rho, s = axis ? 0.0 : y / rho;
  u = (double)p[0] * r * c + (double)p[2];
  v = (double)p[1] * r * s + (double)p[3];
}

// The double projection with theta from the DOUBLE atan2 / sqrt and nothing else changed: the smooth function projectJac is the derivative
// of.  What a numeric (central-difference) Jacobian is taken on: through the quantised theta above a step of 1e-9 sees a staircase.
DVM_CAM_HD void kb8_project_exact(const float* p, double x, double y, double z, double& u, double& v) {
  const double rho2 = x * x + y * y;
  const double r = kb8_radius<double>(p + 4, atan2(sqrt(rho2), z));
  const double rho = sqrt(rho2);
  const bool axis = !(rho > 0.0);
  const double c = axis ? 1.0 : x / rho, s = axis ? 0.0 : y / rho;
  u = (double)p[0] * r * c + (double)p[2];
  v = (double)p[1] * r * s + (double)p[3];
}

// projectJac: d(u, v) / d(x, y, z), row-major 2 x 3, double; its theta is the double atan2.  With rho = sqrt(x^2 + y^2),
// d^2 = rho^2 + z^2, r(theta) and r'(theta) = 1 + 3 k1 theta^2 + 5 k2 theta^4 + 7 k3 theta^6 + 9 k4 theta^8:
//   a = r' z / (rho^2 d^2)  (radial: d theta / d rho = z / d^2, along (x, y) / rho),   b = r / rho^3  (tangential),
//   du/dx = fx (a x^2 + b y^2),  du/dy = fx (a - b) x y,  du/dz = -fx r' x / d^2, and v likewise with x and y exchanged.
// On the optical axis (x = y = 0) the expressions are 0 / 0 and the result is NaN, as in the reference: not special-cased.
DVM_CAM_HD void kb8_project_jac(const float* p, double x, double y, double z, double* J) {
  const double xx = x * x, yy = y * y;
  const double rho2 = xx + yy, d2 = rho2 + z * z;
  const double rho = sqrt(rho2);
  const double theta = atan2(rho, z);
  const double t2 = theta * theta;
  const double r = kb8_radius<double>(p + 4, theta);
  double dr = 1.0, ev = t2;    // r'(theta): even powers theta^2 ... theta^8 with weights 3, 5, 7, 9
#pragma unroll
  for (int i = 0; i < 4; i++) {
    dr = dr + (double)(2 * i + 3) * (double)p[4 + i] * ev;
    ev = ev * t2;
  }
  const double fx = (double)p[0], fy = (double)p[1];
  const double a = dr * z / (rho2 * d2), b = r / (rho2 * rho);
  const double cross = a * y * x - b * y * x;
  J[0] = fx * (a * xx + b * yy);
  J[1] = fx * cross;
  J[2] = -fx * dr * x / d2;
  J[3] = fy * cross;
  J[4] = fy * (a * yy + b * xx);
  J[5] = -fy * dr * y / d2;
}

// unproject: the ray (X, Y, 1) through pixel (u, v), float.  The normalised offset m = ((u - cx) / fx, (v - cy) / fy) has length
// r(theta); theta is found by Newton's method on g(theta) = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) - |m|,
// g' = 1 + 3 k1 theta^2 + 5 k2 theta^4 + 7 k3 theta^6 + 9 k4 theta^8, from theta = |m|: ten steps at most, stopped after the first
// step smaller than the reference's precision of 1e-6; |m| is clamped to pi / 2 and a length below 1e-8 leaves the ray unscaled, as
// the reference does; the ray is m tan(theta) / |m|.
constexpr float kUnprojectPrecision = 1e-6f;
constexpr int kUnprojectSteps = 10;
DVM_CAM_HD void kb8_unproject(const float* p, float u, float v, float* ray) {
  const float mx = (u - p[2]) / p[0], my = (v - p[3]) / p[1];
  const float half_pi = (float)(3.1415926535897932384626433832795 / 2.0);
  const float len = fminf(fmaxf(-half_pi, sqrtf(mx * mx + my * my)), half_pi);
  float gain = 1.f;
  if (len > 1e-8) {
    float theta = len;
    for (int step = 0; step < kUnprojectSteps; step++) {
      const float t2 = theta * theta, t4 = t2 * t2;
      const float e[4] = {p[4] * t2, p[5] * t4, p[6] * (t4 * t2), p[7] * (t4 * t4)};   // k_i theta^(2 i)
      const float g = theta * (1 + e[0] + e[1] + e[2] + e[3]) - len;
      const float dg = 1 + 3 * e[0] + 5 * e[1] + 7 * e[2] + 9 * e[3];
      const float delta = g / dg;
      theta = theta - delta;
      if (fabsf(delta) < kUnprojectPrecision) break;
    }
    gain = tanf(theta) / len;
  }
  ray[0] = mx * gain; ray[1] = my * gain; ray[2] = 1.f;
}

// Pinhole::project in float as the matcher sites write it, for callers that select the model at run time (host mirrors)
DVM_CAM_HD void project(int model, const float* p, float x, float y, float z, float& u, float& v) {
  if (model == kKannalaBrandt8) kb8_project(p, x, y, z, u, v);
  else { u = p[0] * x / z + p[2]; v = p[1] * y / z + p[3]; }
}

}  // namespace dvm_cam
