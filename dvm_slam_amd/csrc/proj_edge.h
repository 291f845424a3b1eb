// dvm_slam_amd/csrc/proj_edge.h -- the reprojection edge of the FP64 optimisers, ONE definition: the camera (PoseCamPinhole / PoseCamKB8)
// and what EdgeSE3ProjectXYZ / EdgeSE3ProjectXYZOnlyPose compute with it (OptimizableTypes.cpp:51-63,136-155): the point in the camera
// frame, the residual, chi2, and the Jacobians A (2x3, landmark) and B (2x6, pose).  Its users -- k_edge_eval (ba_kernels.hip),
// pose_optimize_block (pose_kernels.hip), win_edge_pass (ba_window_seq.hip) and cl_edge_pass (ba_window_cluster.hip) -- keep only what is theirs: where the rows go,
// which edges are active, what is accumulated.  Three of them promise g2o's bits: the expressions and their order are the oracle's.
#pragma once
#include <hip/hip_runtime.h>

#include "camera_model.h"
#include "se3_f64.h"

namespace dvm {

// The camera of a projection edge: what an edge asks of it is the projection (the residual) and MINUS the projection's Jacobian
// (EdgeSE3ProjectXYZ::linearizeOplus, OptimizableTypes.cpp:147-154: -projectJac(xyz_trans) * R and * SE3deriv;
// EdgeSE3ProjectXYZOnlyPose::linearizeOplus, :51-63).
struct PoseCamPinhole {   // Pinhole::project / projectJac: four doubles, laid out as the four scalar arguments they replace
  double fx, fy, cx, cy;
  __device__ __forceinline__ void project(double x, double y, double z, double& u, double& v) const { u = fx * x / z + cx; v = fy * y / z + cy; }
  __device__ __forceinline__ void neg_jac(double x, double y, double z, double* J) const {
    J[0] = -(fx / z); J[1] = 0; J[2] = fx * x / (z * z); J[3] = 0; J[4] = -(fy / z); J[5] = fy * y / (z * z);
  }
};
struct PoseCamKB8 {       // KannalaBrandt8 (camera_model.h): mvParameters as the reference stores them
  float p[8];
  __device__ __forceinline__ void project(double x, double y, double z, double& u, double& v) const { dvm_cam::kb8_project(p, x, y, z, u, v); }
  __device__ __forceinline__ void neg_jac(double x, double y, double z, double* J) const {
    dvm_cam::kb8_project_jac(p, x, y, z, J);
#pragma unroll
    for (int i = 0; i < 6; i++) J[i] = -J[i];
  }
};

// One edge at the pose (R, T) -- R = quat_to_R(T + 3), which a caller with many edges on one pose forms once -- of the landmark X, observed at
// (o0, o1) with information info * I.  The constructor is computeError: (x, y, z) = R X + t, e = obs - project, chi2 = e^T Omega e.
template <class CAM>
struct ProjEdge {
  double x, y, z, e0, e1, info, chi2;
  __device__ __forceinline__ ProjEdge(const CAM& cam, const double* R, const double* T, const double* X, double o0, double o1, double info_) {
    double Xc[3];
    mat3_vec(R, X, Xc);
    Xc[0] += T[0]; Xc[1] += T[1]; Xc[2] += T[2];
    x = Xc[0]; y = Xc[1]; z = Xc[2];
    info = info_;
    double pu, pv;
    cam.project(x, y, z, pu, pv);
    e0 = o0 - pu;
    e1 = o1 - pv;
    chi2 = e0 * info * e0 + e1 * info * e1;
  }
  // linearizeOplus: J = -projectJac at (x, y, z), then A = J R (2x3) and B = J S (2x6), S = [-[Xc]x | I].  Each half forms J itself (a caller
  // of both pays for one: the compiler merges them), so that a caller of one half, k_pose_optimize or a fixed camera's row, names no J.
  __device__ __forceinline__ void jac_point(const CAM& cam, const double* R, double* A) const {
    double J[6];
    cam.neg_jac(x, y, z, J);
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) A[3 * r + c] = J[3 * r] * R[c] + J[3 * r + 1] * R[3 + c] + J[3 * r + 2] * R[6 + c];
  }
  __device__ __forceinline__ void jac_pose(const CAM& cam, double* B) const {
    double J[6];
    cam.neg_jac(x, y, z, J);
    const double S[18] = {0, z, -y, 1, 0, 0, -z, 0, x, 0, 1, 0, y, -x, 0, 0, 0, 1};
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
      for (int c = 0; c < 6; c++) B[6 * r + c] = J[3 * r] * S[c] + J[3 * r + 1] * S[6 + c] + J[3 * r + 2] * S[12 + c];
  }
  // the edge's part of constructQuadraticForm under the robust weight rho1 (robustify(chi2, ...)): w = rho' Omega, wr = -Omega e rho'
  __device__ __forceinline__ double w(double rho1) const { return rho1 * info; }
  __device__ __forceinline__ double wr0(double rho1) const { return -info * e0 * rho1; }
  __device__ __forceinline__ double wr1(double rho1) const { return -info * e1 * rho1; }
};
// entry (a, b) of the edge's Hpl block W = w B^T A (6x3)
__device__ __forceinline__ double proj_edge_hpl(double w, const double* B, const double* A, int a, int b) { return w * (B[a] * A[b] + B[6 + a] * A[3 + b]); }

}  // namespace dvm
