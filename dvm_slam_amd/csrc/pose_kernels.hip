// dvm_slam_amd/csrc/pose_kernels.hip -- Optimizer::PoseOptimization on the device, FP64, for gfx950:
//   B1  k_pose_optimize      one workgroup per frame runs the four rounds of optimize(10) on the pinhole camera
//       k_pose_optimize_kb8  the same body (pose_optimize_block) on a KannalaBrandt8 camera
// The projection edge and the two cameras are proj_edge.h's, the 28-value reduction reduce_f64.h's.  Launchers: ba_kernels.h.
#include <hip/hip_runtime.h>

#include "ba_kernels.h"
#include "f64_spec.h"
#include "proj_edge.h"
#include "reduce_f64.h"
#include "se3_f64.h"

namespace dvm {

// ---------------------------------------------------------------------------------------- B1
// Optimizer::PoseOptimization (reference src/Optimizer.cc:744-1028, mono edges
// EdgeSE3ProjectXYZOnlyPose, src/OptimizableTypes.cpp:51-63): one camera, N unary reprojection edges,
// 4 rounds x optimize(10) of g2o's Levenberg with a dense 6x6 solve, re-classifying inliers after every
// round (chi2 > 5.991 as float), Huber removed after round 2.  ONE workgroup runs the whole thing for
// one frame -- about 40 LM iterations with no host round trip; frames are batched over the grid.
struct PoseAccum { double v[28]; };  // 21 upper-H + 6 b + 1 chi
// The kernel is a LATENCY path -- Tracking calls PoseOptimization two or three times per frame, one frame at a time, and a
// workgroup runs ~40 dependent LM iterations -- so everything that repeats per iteration is kept off the memory system and off
// the serial thread: a thread's correspondences (up to kPoseEdgesPerThread x 256 per frame; more fall back to global reads) live
// in registers across all iterations together with their level flag and last chi2; the Jacobian pass reduces its 28 sums in one
// pass through LDS; a trial's chi2-only pass reduces ONE value; the 6x6 solve forms 1 / L_ii once per row (v_rsq_f64 + two
// Newton steps, as the tile Cholesky does) instead of 27 double-precision divisions and 6 square roots on a single lane.
// (Measured, one frame of 300 matches: 363 us per call before, of which ~2.8 us per LM trial were the divisions.)
constexpr int kPoseEdgesPerThread = 5;
// KannalaBrandt8: its Jacobian needs 78 more registers than the pinhole's six values, and 5 still does not spill (docs/NOTEBOOK.md section 16)
constexpr int kPoseEdgesPerThreadKB8 = 5;
#ifdef DVM_POSE_PROF   // make EXTRA=-DDVM_POSE_PROF: per-phase clocks of workgroup 0 (dvm_debug_pose_prof), measurement builds only
__device__ unsigned long long g_pose_prof[16];
#define POSE_T(k) do { if (tid == 0 && blockIdx.x == 0) { const unsigned long long now_ = wall_clock64(); g_pose_prof[k] += now_ - pose_last_; pose_last_ = now_; } } while (0)
#else
#define POSE_T(k) do {} while (0)
#endif
// The body of k_pose_optimize, common to every camera: LM control, speculative linearisation, the 28-value reduction, the 6x6 solve and
// the four rounds; the camera enters `edge` and `fresh` through project / neg_jac only.  EPT: correspondences a thread keeps in
// registers (kPoseEdgesPerThread for the pinhole camera, kPoseEdgesPerThreadKB8 for KannalaBrandt8).
template <class CAM, int EPT>
__device__ __forceinline__ void pose_optimize_block(const double* __restrict__ pose_in, const double* __restrict__ Xw,
                                                    const double* __restrict__ obs, const double* __restrict__ info,
                                                    const int32_t* __restrict__ n_per_frame, int stride, const CAM cam,
                                                    double* __restrict__ pose_out, uint8_t* __restrict__ outlier,
                                                    int32_t* __restrict__ n_inliers, double* __restrict__ chi_scratch) {
  __shared__ double s_park[256 * 29];
  __shared__ double s_part[4 * 28];
  __shared__ double s_sum[28];
  __shared__ double s_T[7], s_Tbak[7], s_T0[7];
  __shared__ double s_lambda, s_ni, s_cur, s_ini, s_rho;
  __shared__ int s_ctl, s_qmax, s_nbad, s_nact, s_lin;
  const int f = blockIdx.x, tid = threadIdx.x;
#ifdef DVM_POSE_PROF
  unsigned long long pose_last_ = wall_clock64();
#endif
  const int N = n_per_frame[f];
  const double* X = Xw + (size_t)f * stride * 3;
  const double* O = obs + (size_t)f * stride * 2;
  const double* W = info + (size_t)f * stride;
  uint8_t* outl = outlier + (size_t)f * stride;
  double* last_chi = chi_scratch + (size_t)f * stride;  // e->chi2() as g2o reports it (last evaluation): edges beyond the register-resident ones
  const double delta = (double)sqrtf(5.991f);
  const float chi2Mono = 5.991f;
  if (tid < 7) {
    double v = pose_in[7 * (size_t)f + tid];
    s_T0[tid] = v;
  }
  __syncthreads();
  if (tid == 0) quat_normalize(&s_T0[3]);
  // this thread's correspondences: registers for the first EPT, global memory beyond
  double eX[EPT][3], eO[EPT][2], eW[EPT], eChi[EPT];
  bool eOut[EPT];       // level(1) == outlier flag in the reference's bookkeeping
#pragma unroll
  for (int e = 0; e < EPT; e++) {
    const int i = tid + 256 * e;
    const bool in = i < N;
    const int ii = in ? i : 0;
    eX[e][0] = X[3 * ii]; eX[e][1] = X[3 * ii + 1]; eX[e][2] = X[3 * ii + 2];
    eO[e][0] = O[2 * ii]; eO[e][1] = O[2 * ii + 1];
    eW[e] = W[ii];
    eChi[e] = 0; eOut[e] = false;
  }
  for (int i = tid + 256 * EPT; i < N; i += 256) { outl[i] = 0; last_chi[i] = 0; }
  __syncthreads();
  if (N < 3) {  // nInitialCorrespondences < 3: return 0, pose untouched (Optimizer.cc:904-905)
    if (tid < 7) pose_out[7 * (size_t)f + tid] = pose_in[7 * (size_t)f + tid];
    for (int i = tid; i < N; i += 256) outl[i] = 0;
    if (tid == 0) n_inliers[f] = 0;
    return;
  }
  // one active edge at pose (R, T): chi2 (always; returned), H / b terms (jac)
  auto edge = [&](const double* R, const double* T, const double* Xp, double o0, double o1, double w0, bool jac, bool robust_on, PoseAccum& a) -> double {
    const ProjEdge<CAM> e(cam, R, T, Xp, o0, o1, w0);
    double r0, r1;
    robustify(e.chi2, robust_on ? delta : 0.0, r0, r1);
    a.v[27] += r0;
    if (jac) {
      double B[12];
      e.jac_pose(cam, B);
      const double w = e.w(r1), wr0 = e.wr0(r1), wr1 = e.wr1(r1);
      int t = 0;
#pragma unroll
      for (int p = 0; p < 6; p++) {
        a.v[21 + p] += B[p] * wr0 + B[6 + p] * wr1;
#pragma unroll
        for (int q = 0; q <= p; q++) a.v[t++] += w * (B[p] * B[q] + B[6 + p] * B[6 + q]);
      }
    }
    return e.chi2;
  };
  // evaluates the active edges at pose T: chi (always), H / b (jac); updates the edges' last chi2.  Result in s_sum ([27] = chi2).
  auto eval = [&](const double* T, bool jac, bool robust_on) {
    PoseAccum a;
#pragma unroll
    for (int i = 0; i < 28; i++) a.v[i] = 0;
    double R[9];
    quat_to_R(T + 3, R);
#pragma unroll
    for (int e = 0; e < EPT; e++) {
      if (tid + 256 * e < N && !eOut[e]) eChi[e] = edge(R, T, eX[e], eO[e][0], eO[e][1], eW[e], jac, robust_on, a);
    }
    for (int i = tid + 256 * EPT; i < N; i += 256) {
      if (outl[i]) continue;
      last_chi[i] = edge(R, T, X + 3 * i, O[2 * i], O[2 * i + 1], W[i], jac, robust_on, a);
    }
    if (jac) block_sum_lds<28>(a.v, s_park, s_part, s_sum);
    else {
      const double c = block_sum_one(a.v[27], s_part);
      if (tid == 0) s_sum[27] = c;
      __syncthreads();
    }
  };

  bool robust_on = true;
  for (int round = 0; round < 4; round++) {
    if (tid < 7) s_T[tid] = s_T0[tid];  // vSE3->setEstimate(pFrame->GetPose()) every round
    if (tid == 0) { s_nact = 0; s_ctl = 0; s_nbad = 0; s_lin = 0; }
    __syncthreads();
    int my = 0;
#pragma unroll
    for (int e = 0; e < EPT; e++) my += (tid + 256 * e < N && !eOut[e]) ? 1 : 0;
    for (int i = tid + 256 * EPT; i < N; i += 256) my += outl[i] ? 0 : 1;
    if (my) atomicAdd(&s_nact, my);
    __syncthreads();
    const int nact = s_nact;
    POSE_T(0);
    for (int it = 0; it < 10 && nact > 0; it++) {
      // Speculative linearisation (as the tile solver's LM loop does it): an accepted trial has evaluated its state WITH the Jacobians, so
      // the iteration that follows finds H, b and chi2 of its state in s_sum already -- one pass per accepted trial instead of two
      // (chi2 only, then the same edges again with Jacobians); a rejected trial's sums are simply overwritten.
      const bool have_lin = s_lin != 0;
      __syncthreads();
      if (tid == 0) s_lin = 0;
      if (!have_lin) eval(s_T, true, robust_on);
      POSE_T(1);
      if (tid == 0) {
        s_cur = s_sum[27]; s_ini = s_sum[27];
        if (it == 0) {
          double mx = 0;
          int t = 0;
          for (int p = 0; p < 6; p++) for (int q = 0; q <= p; q++) { if (p == q) mx = fmax(mx, fabs(s_sum[t])); t++; }
          s_lambda = 1e-5 * mx; s_ni = 2; s_nbad = 0;
        }
        s_qmax = 0;
      }
      __syncthreads();
      double Hs[21], bs[6];
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 21; i++) Hs[i] = s_sum[i];
#pragma unroll
        for (int i = 0; i < 6; i++) bs[i] = s_sum[21 + i];
      }
      POSE_T(2);
      while (true) {
        double xs[6];
        bool ok = true;
        if (tid == 0) {
          for (int i = 0; i < 7; i++) s_Tbak[i] = s_T[i];
          // dense 6x6 Cholesky of (H + lambda I), lower-packed Hs[p(p+1)/2 + q]; ri[j] = 1 / L_jj
          double Lm[21], ri[6];
#pragma unroll
          for (int i = 0; i < 6; i++)
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
            for (int i = 0; i < 6; i++) {
              double sacc = bs[i];
#pragma unroll
              for (int k = 0; k < i; k++) sacc -= Lm[i * (i + 1) / 2 + k] * xs[k];
              xs[i] = sacc * ri[i];
            }
#pragma unroll
            for (int i = 5; i >= 0; i--) {
              double sacc = xs[i];
#pragma unroll
              for (int k = i + 1; k < 6; k++) sacc -= Lm[k * (k + 1) / 2 + i] * xs[k];
              xs[i] = sacc * ri[i];
            }
            se3_oplus(s_T, xs, s_T);
          }
          s_ctl = ok ? 1 : 0;
        }
        __syncthreads();
        POSE_T(3);
        const bool okb = s_ctl != 0;
        const bool spec = it + 1 < 10;        // (the last iteration of a round: nobody would use the linearisation)
        if (okb) eval(s_T, spec, robust_on);
        POSE_T(4);
        if (tid == 0) {
          const double tempChi = okb ? s_sum[27] : 1.7976931348623157e308;
          double rho = s_cur - tempChi;
          double scale = 0;
          if (okb) for (int j = 0; j < 6; j++) scale += xs[j] * (s_lambda * xs[j] + bs[j]);
          scale += 1e-3;
          rho /= scale;
          if (rho > 0 && isfinite(tempChi)) {
            double alpha = 1. - f64_cube(2 * rho - 1);   // pow(2 rho - 1, 3) as the shared double-precision spec forms it (f64_spec.h)
            alpha = fmin(alpha, 2. / 3.);
            s_lambda *= fmax(1. / 3., alpha);
            s_ni = 2;
            s_cur = tempChi;
            if (spec) s_lin = 1;                   // s_sum holds this state's linearisation
          } else {
            s_lambda *= s_ni; s_ni *= 2;
            for (int i = 0; i < 7; i++) s_T[i] = s_Tbak[i];
          }
          s_qmax++;
          s_rho = rho;
          s_ctl = (rho < 0 && s_qmax < 10) ? 1 : 0;  // continue the trial loop?
        }
        __syncthreads();
        POSE_T(5);
        if (!s_ctl) break;
        __syncthreads();
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
      POSE_T(6);
#ifdef DVM_POSE_PROF
      if (tid == 0 && blockIdx.x == 0) g_pose_prof[15]++;
#endif
      if (stop) break;
    }
    // classification (Optimizer.cc:923-948): outliers recompute their error, inliers report the last evaluation
    {
      double R[9];
      quat_to_R(s_T + 3, R);
      auto fresh = [&](const double* Xp, double o0, double o1, double w0) { return ProjEdge<CAM>(cam, R, s_T, Xp, o0, o1, w0).chi2; };
#pragma unroll
      for (int e = 0; e < EPT; e++) {
        if (tid + 256 * e < N) {
          if (eOut[e]) eChi[e] = fresh(eX[e], eO[e][0], eO[e][1], eW[e]);
          eOut[e] = (float)eChi[e] > chi2Mono;
        }
      }
      for (int i = tid + 256 * EPT; i < N; i += 256) {
        if (outl[i]) last_chi[i] = fresh(X + 3 * i, O[2 * i], O[2 * i + 1], W[i]);
        outl[i] = (float)last_chi[i] > chi2Mono ? 1 : 0;
      }
    }
    if (round == 2) robust_on = false;
    __syncthreads();
    POSE_T(7);
    if (N < 10) break;  // optimizer.edges().size() < 10
  }
  if (tid == 0) s_nact = 0;
  __syncthreads();
  int bad = 0;
#pragma unroll
  for (int e = 0; e < EPT; e++) {
    const int i = tid + 256 * e;
    if (i < N) { outl[i] = eOut[e] ? 1 : 0; bad += eOut[e] ? 1 : 0; }
  }
  for (int i = tid + 256 * EPT; i < N; i += 256) bad += outl[i];
  if (bad) atomicAdd(&s_nact, bad);
  __syncthreads();
  if (tid < 7) pose_out[7 * (size_t)f + tid] = s_T[tid];
  if (tid == 0) n_inliers[f] = N - s_nact;
}
// the pinhole camera: the four intrinsics travel as scalars
__global__ void __launch_bounds__(256) k_pose_optimize(const double* __restrict__ pose_in, const double* __restrict__ Xw,
                                                       const double* __restrict__ obs, const double* __restrict__ info,
                                                       const int32_t* __restrict__ n_per_frame, int stride, double fx,
                                                       double fy, double cx, double cy, double* __restrict__ pose_out,
                                                       uint8_t* __restrict__ outlier, int32_t* __restrict__ n_inliers,
                                                       double* __restrict__ chi_scratch) {
  pose_optimize_block<PoseCamPinhole, kPoseEdgesPerThread>(pose_in, Xw, obs, info, n_per_frame, stride, PoseCamPinhole{fx, fy, cx, cy}, pose_out, outlier,
                                                           n_inliers, chi_scratch);
}
// KannalaBrandt8 (dvm_pose_optimize_cam, model 1)
__global__ void __launch_bounds__(256) k_pose_optimize_kb8(const double* __restrict__ pose_in, const double* __restrict__ Xw,
                                                           const double* __restrict__ obs, const double* __restrict__ info,
                                                           const int32_t* __restrict__ n_per_frame, int stride, PoseCamKB8 cam,
                                                           double* __restrict__ pose_out, uint8_t* __restrict__ outlier,
                                                           int32_t* __restrict__ n_inliers, double* __restrict__ chi_scratch) {
  pose_optimize_block<PoseCamKB8, kPoseEdgesPerThreadKB8>(pose_in, Xw, obs, info, n_per_frame, stride, cam, pose_out, outlier, n_inliers, chi_scratch);
}

#ifdef DVM_POSE_PROF
extern "C" int dvm_debug_pose_prof(unsigned long long* out, int reset) {
  unsigned long long h[16];
  int rc = (int)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_pose_prof), sizeof(h));
  for (int i = 0; i < 16; i++) out[i] = h[i];
  if (reset) { for (auto& v : h) v = 0; rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_pose_prof), h, sizeof(h)); }
  return rc;
}
#endif
void ba_launch_pose_optimize(hipStream_t s, const double* pose_in, const double* Xw, const double* obs, const double* info,
                             const int32_t* n_per_frame, int stride, int batch, double fx, double fy, double cx, double cy,
                             double* pose_out, uint8_t* outlier, int32_t* n_inliers, double* chi_scratch) {
  hipLaunchKernelGGL(k_pose_optimize, dim3(batch), dim3(256), 0, s, pose_in, Xw, obs, info, n_per_frame, stride, fx, fy, cx, cy,
                     pose_out, outlier, n_inliers, chi_scratch);
}
// k_pose_optimize_kb8: the same body on a KannalaBrandt8 camera, p = mvParameters (dvm_pose_optimize_cam, model 1)
void ba_launch_pose_optimize_kb8(hipStream_t s, const double* pose_in, const double* Xw, const double* obs, const double* info,
                                 const int32_t* n_per_frame, int stride, int batch, const float* p, double* pose_out, uint8_t* outlier,
                                 int32_t* n_inliers, double* chi_scratch) {
  PoseCamKB8 cam;
  for (int i = 0; i < 8; i++) cam.p[i] = p[i];
  hipLaunchKernelGGL(k_pose_optimize_kb8, dim3(batch), dim3(256), 0, s, pose_in, Xw, obs, info, n_per_frame, stride, cam, pose_out, outlier, n_inliers,
                     chi_scratch);
}

}  // namespace dvm
