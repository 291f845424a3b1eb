// dvm_slam_amd/csrc/ba_kernels.hip -- the FP64 front end of bundle adjustment for gfx950 (driver: ba_solver.cpp): everything of a trial
// but the reduced solve, which is the tile solver's (K10: chol_kernels.hip, on the TileSystem embedded in the BaView).
//
// One Levenberg-Marquardt iteration of the reference's BA (g2o BlockSolver_6_3 + Levenberg,
// reference Thirdparty/g2o/g2o/core/{block_solver.hpp,optimization_algorithm_levenberg.cpp},
// src/Optimizer.cc:55-356,1030-1387, src/OptimizableTypes.cpp:136-155, src/CameraModels/{Pinhole,KannalaBrandt8}.cpp):
//   K8  k_edge_eval<JAC, CAM>  per-edge residual, Huber weight, 2x3 / 2x6 Jacobians, Hpl block (the edge itself: proj_edge.h)
//       k_accum                Hll (3x3), bl per landmark and Hpp (6x6), bp per camera: fixed-order gathers; k_max_diag(_sharded)
//   K9  k_dinv / k_trial_prologue   Dinv = (Hll + lambda I)^-1
//       k_schur<NW>, k_clear_tiles   S = Hpp - sum W Dinv W^T, bschur = bp - sum W Dinv bl (augmented row of S)
//   K11 k_point_backsub        xl = Dinv (bl - W^T xp); T <- exp(d) T, X <- X + d;  k_edge_depth
//   sharded solve              k_pack_tiles, k_hpp_diag, k_points_exchange
// All accumulations are gathers with a fixed order: results are run-to-run deterministic.
// The other FP64 optimisers live in files of their own: pose_kernels.hip (PoseOptimization), sim3_kernels.hip (OptimizeSim3, Sim3Solver),
// pg_kernels.hip (essential graph), ba_window_seq.hip / ba_window_cluster.hip (windows); the small algebra they share is se3_f64.h's.
#include <hip/hip_runtime.h>

#include <cstring>

#include "ba_kernels.h"
#include "proj_edge.h"
#include "se3_f64.h"

namespace dvm {

__device__ __forceinline__ double ba_lambda(const BaView& V) { return V.lambda ? *V.lambda : V.lambda_v; }

// Block sum of `v` -> partial[blockIdx.x]; the last workgroup to arrive then reduces all partials exactly like
// k_reduce_sum of pg_kernels.hip (thread-strided sums, then the same tree: identical bits) and hands the result to the host (BaPublish).
template <bool MAX>
__device__ __forceinline__ void block_reduce_publish(double v, double* __restrict__ partial, const BaPublish& pub, int nb_part = 0) {
  __shared__ double s_red[256];
  __shared__ int s_last;
  const int tid = threadIdx.x, nb = nb_part ? nb_part : (int)gridDim.x;   // workgroups [0, nb) take part
  s_red[tid] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) s_red[tid] = MAX ? fmax(s_red[tid], s_red[tid + off]) : s_red[tid] + s_red[tid + off];
    __syncthreads();
  }
  if (tid == 0) {
    // 8-byte agent-scope (write-through) store of the partial, drained before the arrival is counted: whoever sees the
    // count can read the partial with an agent-scope load.  No release fence: that would write back this XCD's whole L2
    // (the edge pass has just dirtied megabytes) once per workgroup -- measured 23 -> 58 us on k_edge_eval.
    __hip_atomic_store(partial + blockIdx.x, s_red[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = __hip_atomic_fetch_add(pub.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(nb - 1);
  }
  __syncthreads();
  if (!s_last) return;
  double acc = 0;
  for (int i = tid; i < nb; i += 256) {
    const double p = __hip_atomic_load(partial + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    acc = MAX ? fmax(acc, p) : acc + p;
  }
  s_red[tid] = acc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) s_red[tid] = MAX ? fmax(s_red[tid], s_red[tid + off]) : s_red[tid] + s_red[tid + off];
    __syncthreads();
  }
  if (tid == 0) {
    __hip_atomic_store(pub.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(pub.dev_vals + pub.slot, s_red[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (pub.publish) {
      // results of earlier kernels of this phase (other slots) are in dev_vals: kernel boundaries made them visible.  ALL of them
      // (and the failure flag) are fetched before the first store: alternating agent-scope loads and system-scope stores was six
      // dependent round trips on one thread -- 4-5 us at the very end of the kernel that publishes chi2 in every trial
      double dv[6];
#pragma unroll
      for (int i = 0; i < 6; i++) dv[i] = pub.dev_vals[i];
      const int f = pub.d_fail ? *pub.d_fail : 0;
#pragma unroll
      for (int i = 0; i < 6; i++) dv[i] = (i == pub.slot) ? s_red[0] : dv[i];
#pragma unroll
      for (int i = 0; i < 6; i++) __hip_atomic_store(pub.host_vals + i, dv[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(pub.host_vals + 6, (double)f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (pub.spec) {
        // OptimizationAlgorithmLevenberg::solve's accept / reject and lambda update (optimization_algorithm_levenberg.cpp:
        // 113-131) exactly as dvm_ba_optimize takes them on the host, which checks the result bit for bit before it relies on
        // anything derived from it.  pow(t, 3) is formed with the rounding errors of both products carried along (the
        // correctly rounded cube, which is what libm returns for almost every t).
        const double tmp = f == 0 ? s_red[0] : 1.7976931348623157e308;
        const double scale = dv[2] + 1e-3;                     // computeScale() runs on whatever x holds, failed solve or not
        const double rho = (pub.cur_chi - tmp) / scale;
        double next = -1.0;
        if (pub.spec_mode == 1) next = 1e-5 * s_red[0];   // computeLambdaInit (_tau = 1e-5) on the max |diag| this workgroup has just reduced
        else if (rho > 0 && isfinite(tmp)) {
          const double t = 2 * rho - 1;
          const double t2 = t * t, e2 = __builtin_fma(t, t, -t2);
          const double t3 = t2 * t, e3 = __builtin_fma(t2, t, -t3);
          const double cube = t3 + (e3 + e2 * t);
          double alpha = 1. - cube;
          alpha = fmin(alpha, 2. / 3.);
          next = pub.lambda * fmax(1. / 3., alpha);
          if ((pub.cur_chi - tmp) * 1e3 < pub.cur_chi && pub.n_bad + 1 >= 3) next = -2.0;   // accepted, and the optimisation stops here
        }
        __hip_atomic_store(pub.spec, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pub.host_vals + 7, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      __hip_atomic_store(pub.host_seq, pub.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// the same for one wave (64 lanes), no workgroup barrier: lane i < N returns the sum of value i over the lanes, in lane order
template <int N>
__device__ __forceinline__ double wave_sum_lds(const double* v, double* park /* 64 * (N + 1) doubles of this wave */) {
  const int lane = threadIdx.x & 63;
  __builtin_amdgcn_wave_barrier();
  double* mine = park + (size_t)lane * (N + 1);
#pragma unroll
  for (int i = 0; i < N; i++) mine[i] = v[i];
  __builtin_amdgcn_wave_barrier();
  double s = 0;
  if (lane < N) {
#pragma unroll 16
    for (int l = 0; l < 64; l++) s += park[(size_t)l * (N + 1) + lane];
  }
  __builtin_amdgcn_wave_barrier();
  return s;
}

// the camera of a bundle-adjustment problem out of its view: the four doubles, or mvParameters (BaView::cam_p)
template <class CAM> __device__ __forceinline__ CAM ba_view_cam(const BaView& V);
template <> __device__ __forceinline__ PoseCamPinhole ba_view_cam<PoseCamPinhole>(const BaView& V) { return PoseCamPinhole{V.fx, V.fy, V.cx, V.cy}; }
template <> __device__ __forceinline__ PoseCamKB8 ba_view_cam<PoseCamKB8>(const BaView& V) {
  PoseCamKB8 c;
#pragma unroll
  for (int i = 0; i < 8; i++) c.p[i] = V.cam_p[i];
  return c;
}

// ------------------------------------------------------------------------------------------ K8
// JAC=false: residual / chi2 only (computeActiveErrors + activeRobustChi2 terms).
// JAC=true : additionally Jacobians A (2x3, point), B (2x6, pose), weights and Hpl block W (6x3).
// The Jacobian rows leave through LDS: a thread's rows are 128 B (e_lin: camera half) + 128 B (e_linA: landmark half) + 144 B (W),
// and per-thread row stores touch 64 different cache lines per instruction (1 344 line writes per wave for 172 lines of data when
// the halves still shared a 192-byte row: ~10 of the kernel's 28 us).  A wave's 64 rows are one contiguous 8 KB / 8 KB / 9 KB image
// in global memory: every lane parks its row in LDS (row pitch 18 doubles: 16-byte writes without bank conflicts), three times in
// turn, and the wave copies the image out with 16-byte stores, 1 KB per instruction.
// CAM: the problem's camera (PoseCamPinhole / PoseCamKB8), which enters through project and neg_jac only.  Under KannalaBrandt8 the residual's
// theta is the float atan2f of project(Vector3d) and the Jacobian's the double atan2 (camera_model.h), the chi2-only pass evaluates no
// Jacobian, and a point on the optical axis gets NaN rows as in the reference (an inactive edge exact zeros all the same).
constexpr int kLinPitch = 18;
template <bool JAC, class CAM>
__global__ void __launch_bounds__(256) k_edge_eval(BaView V, BaPublish pub) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  __shared__ double2 s_rows[JAC ? 4 * 64 * kLinPitch / 2 : 1];
  double* park = reinterpret_cast<double*>(s_rows) + (size_t)(threadIdx.x >> 6) * 64 * kLinPitch;   // this wave's rows
  const int lane = threadIdx.x & 63;
  double Wv[18], Av[9];
  double rho0 = 0;
  if (k < V.E) {
    const int p = V.e_pose[k], l = V.e_point[k];
    const double* T = (JAC ? V.poses : V.poses_new) + 7 * (size_t)p;     // chi2-only evaluations look at the TRIAL state
    const double* X = (JAC ? V.points : V.points_new) + 3 * (size_t)l;
    double R[9];
    quat_to_R(T + 3, R);
    const CAM cam = ba_view_cam<CAM>(V);
    const ProjEdge<CAM> e(cam, R, T, X, V.e_obs[2 * (size_t)k], V.e_obs[2 * (size_t)k + 1], V.e_info[k]);
    const unsigned fl = V.e_flags ? V.e_flags[k] : 3u;
    const bool active = (fl & 1u) != 0;                 // g2o: level 0.  A level-1 edge is outside the active set: no error evaluation
    if (active) V.e_chi2[k] = e.chi2;                   // (its chi2() stays what it was), nothing in chi2 / H / b
    double rho1;
    robustify(e.chi2, (fl & 2u) ? V.delta : 0.0, rho0, rho1);
    if (!active) { rho0 = 0; rho1 = 0; }
    if (JAC) {
      double A[6], B[12];
      e.jac_point(cam, R, A);
      e.jac_pose(cam, B);
      if (!active) {                                    // exact zeros whatever the geometry (a point on the camera plane: inf / NaN rows)
#pragma unroll
        for (int i = 0; i < 6; i++) A[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 12; i++) B[i] = 0.0;
      }
      const double w = active ? e.w(rho1) : 0.0;
      const double wr0 = active ? e.wr0(rho1) : 0.0, wr1 = active ? e.wr1(rho1) : 0.0;
      double2* mine = reinterpret_cast<double2*>(park + (size_t)lane * kLinPitch);
#pragma unroll
      for (int i = 0; i < 6; i++) mine[i] = make_double2(B[2 * i], B[2 * i + 1]);
      mine[6] = make_double2(w, wr0); mine[7] = make_double2(wr1, 0.0);
#pragma unroll
      for (int i = 0; i < 6; i++) Av[i] = A[i];
      Av[6] = w; Av[7] = wr0; Av[8] = wr1;
      const bool pose_free = V.pidx[p] >= 0;
#pragma unroll
      for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) Wv[3 * a + b] = pose_free ? proj_edge_hpl(w, B, A, a, b) : 0.0;
    }
  }
  if (JAC) {
    const int first = blockIdx.x * 256 + (threadIdx.x & ~63);      // the wave's first edge
    const int nrow = min(64, V.E - first);                          // (<= 0 for a wave beyond the last edge)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    double2* img = reinterpret_cast<double2*>(V.e_lin + (size_t)first * kEdgeLinStride);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int g = 64 * i + lane, row = g >> 3, c = g & 7;      // 16-byte chunk g of the image = chunk c of row `row`
      if (row < nrow) img[g] = *reinterpret_cast<const double2*>(park + (size_t)row * kLinPitch + 2 * c);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (k < V.E) {                                   // the landmark half the same way
      double2* mine = reinterpret_cast<double2*>(park + (size_t)lane * kLinPitch);
#pragma unroll
      for (int i = 0; i < 4; i++) mine[i] = make_double2(Av[2 * i], Av[2 * i + 1]);
      mine[4] = make_double2(Av[8], 0.0); mine[5] = make_double2(0.0, 0.0); mine[6] = make_double2(0.0, 0.0); mine[7] = make_double2(0.0, 0.0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    double2* imga = reinterpret_cast<double2*>(V.e_linA + (size_t)first * kEdgeLinStride);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int g = 64 * i + lane, row = g >> 3, c = g & 7;
      if (row < nrow) imga[g] = *reinterpret_cast<const double2*>(park + (size_t)row * kLinPitch + 2 * c);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (k < V.E) {
      double2* mine = reinterpret_cast<double2*>(park + (size_t)lane * 18);
#pragma unroll
      for (int i = 0; i < 9; i++) mine[i] = make_double2(Wv[2 * i], Wv[2 * i + 1]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    double2* imgw = reinterpret_cast<double2*>(V.e_W + (size_t)first * 18);
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const int g = 64 * i + lane, row = g / 9;
      if (row < nrow) imgw[g] = *reinterpret_cast<const double2*>(park + 2 * (size_t)g);      // pitch 18 = the image itself
    }
  }
  block_reduce_publish<false>(rho0, V.partial, pub);   // fixed-order sum of rho0 over all edges -> host
}

// (Hll + lambda I)^-1 and its product with bl for one landmark
__device__ __forceinline__ void dinv_apply(const double* H, const double* bl, double lambda, double* __restrict__ D, double* __restrict__ db) {
  const double M[9] = {H[0] + lambda, H[1], H[2], H[3], H[4] + lambda, H[5], H[6], H[7], H[8] + lambda};
  double o[9];
  inv3(M, o);     // (the operations of ba_window_cluster.hip's w_dinv in the same order: the same bits)
#pragma unroll
  for (int k = 0; k < 9; k++) D[k] = o[k];
  mat3_vec(o, bl, db);
}

// a KEPT landmark (BaView::kept_slot) is not eliminated: it contributes nothing to the Schur complement or its right-hand side
__device__ __forceinline__ void dinv_kept(const BaView& V, int l) {
#pragma unroll
  for (int k = 0; k < 9; k++) V.Dinv[9 * (size_t)l + k] = 0.0;
  V.db[3 * (size_t)l] = V.db[3 * (size_t)l + 1] = V.db[3 * (size_t)l + 2] = 0.0;
}
// Hll (3x3) and bl per landmark: thread per landmark, edges in input order.
__device__ __forceinline__ double point_accum_body(const BaView& V, int block, const double* __restrict__ spec) {   // returns max |Hll diagonal|
  const int l = block * 256 + threadIdx.x;
  if (l >= V.L) return 0.0;
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
  const int e_end = V.pt_start[l + 1];
  for (int i0 = V.pt_start[l]; i0 < e_end; i0 += 4) {      // four edges in flight (index -> row: two dependent round trips each)
    int k[4];
#pragma unroll
    for (int u = 0; u < 4; u++) k[u] = (i0 + u < e_end) ? V.pt_edges[i0 + u] : -1;
    double Av[4][6], wv[4][3];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const double* lin = V.e_linA + (size_t)max(k[u], 0) * kEdgeLinStride;
#pragma unroll
      for (int j = 0; j < 6; j++) Av[u][j] = lin[j];
      wv[u][0] = lin[6]; wv[u][1] = lin[7]; wv[u][2] = lin[8];
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (k[u] < 0) continue;
      const double* lin = Av[u];
      const double w = wv[u][0], wr0 = wv[u][1], wr1 = wv[u][2];
#pragma unroll
      for (int a = 0; a < 3; a++) {
        b[a] += lin[a] * wr0 + lin[3 + a] * wr1;
#pragma unroll
        for (int c = 0; c < 3; c++) H[3 * a + c] += w * (lin[a] * lin[c] + lin[3 + a] * lin[3 + c]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 9; i++) V.Hll[9 * (size_t)l + i] = H[i];
#pragma unroll
  for (int i = 0; i < 3; i++) V.bl[3 * (size_t)l + i] = b[i];
  // the trial this state belongs to was accepted on the device (spec[0] = the next damping): the next trial's prologue work --
  // (Hll + lambda I)^-1 and Dinv bl, dinv_landmark's arithmetic on the same values -- is done here, from registers
  if (spec) {
    const double lambda = *spec;
    if (lambda >= 0 && V.pt_start[l + 1] != V.pt_start[l]) {
      if (V.T.nkept && V.kept_slot[l] >= 0) dinv_kept(V, l);
      else dinv_apply(H, b, lambda, V.Dinv + 9 * (size_t)l, V.db + 3 * (size_t)l);
    }
  }
  return V.pt_start[l + 1] > V.pt_start[l] ? fmax(fabs(H[0]), fmax(fabs(H[4]), fabs(H[8]))) : 0.0;   // (a landmark nobody observes is no vertex)
}

// Hpp (6x6) and bp per free camera: one wave per camera, lanes stride over the camera's edges, then a
// fixed-order xor-butterfly reduction (identical on every run).
// SPLIT (BaView::schur_wide, a local-BA window: a few cameras with hundreds of edges each on an otherwise empty chip): ONE
// camera per workgroup, its edges dealt over the four waves, the waves' sums added in wave order.
template <bool SPLIT>
__device__ __forceinline__ double pose_accum_body(const BaView& V, int block) {   // returns this thread's |Hpp diagonal entry| (or 0)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fi = SPLIT ? block : block * 4 + wave;
  if (fi >= V.nfree) return 0.0;
  const int p = V.free_pose[fi];
  double H[21], b[6];
#pragma unroll
  for (int i = 0; i < 21; i++) H[i] = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) b[i] = 0;
  // four edges per lane in flight: index -> row is a dependent pair of global round trips, and a camera of the BASELINE problem
  // gives a lane five edges -- one after the other that was ten round trips (the kernel's whole 15 us); same summation order
  const int e_end = V.ps_start[p + 1];
  const int step = SPLIT ? 256 : 64;
  for (int i0 = V.ps_start[p] + lane + (SPLIT ? 64 * wave : 0); i0 < e_end; i0 += 4 * step) {
    int k[4];
#pragma unroll
    for (int u = 0; u < 4; u++) k[u] = (i0 + step * u < e_end) ? V.ps_edges[i0 + step * u] : -1;
    double Bv[4][12], wv[4][3];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const double* lin = V.e_lin + (size_t)max(k[u], 0) * kEdgeLinStride;
#pragma unroll
      for (int j = 0; j < 12; j++) Bv[u][j] = lin[j];
      wv[u][0] = lin[12]; wv[u][1] = lin[13]; wv[u][2] = lin[14];
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (k[u] < 0) continue;
      const double* B = Bv[u];
      const double w = wv[u][0], wr0 = wv[u][1], wr1 = wv[u][2];
      int t = 0;
#pragma unroll
      for (int a = 0; a < 6; a++) {
        b[a] += B[a] * wr0 + B[6 + a] * wr1;
#pragma unroll
        for (int c = 0; c <= a; c++) H[t++] += w * (B[a] * B[c] + B[6 + a] * B[6 + c]);
      }
    }
  }
  // lane t < 21 ends with H[t], lanes 21..26 with b (sum over the lanes through LDS, lane order: see wave_sum_lds)
  __shared__ double s_park[4][64 * 28];
  double v27[27];
#pragma unroll
  for (int i = 0; i < 21; i++) v27[i] = H[i];
#pragma unroll
  for (int i = 0; i < 6; i++) v27[21 + i] = b[i];
  double tot = wave_sum_lds<27>(v27, s_park[wave]);
  if (SPLIT) {
    __shared__ double s_w[4][27];
    if (lane < 27) s_w[wave][lane] = tot;
    __syncthreads();
    if (wave != 0) return 0.0;
    if (lane < 27) tot = ((s_w[0][lane] + s_w[1][lane]) + s_w[2][lane]) + s_w[3][lane];
  }
  if (lane < 21) {
    const int a = lane >= 15 ? 5 : lane >= 10 ? 4 : lane >= 6 ? 3 : lane >= 3 ? 2 : lane >= 1 ? 1 : 0;
    const int c = lane - a * (a + 1) / 2;
    double* out = V.Hpp + 36 * (size_t)fi;
    out[6 * a + c] = tot;
    out[6 * c + a] = tot;
    return a == c ? fabs(tot) : 0.0;
  } else if (lane < 27) {
    V.bp[6 * (size_t)fi + (lane - 21)] = tot;
  }
  return 0.0;
}

// one structurally non-zero tile of the reduced system back to "empty": zeros, identity on the padding rows of a diagonal tile
__device__ __forceinline__ void clear_tile(const BaView& V, int t) {
  const int ti = V.T.nz_tiles[2 * t], tj = V.T.nz_tiles[2 * t + 1];
  double* base = V.T.S + (size_t)ti * 64 * V.T.ldS + tj * 64;
  for (int i = threadIdx.x; i < 64 * 32; i += 256) {
    const int r = i >> 5, c2 = i & 31;
    reinterpret_cast<double2*>(base + (size_t)r * V.T.ldS)[c2] = make_double2(0.0, 0.0);
  }
  if (ti == tj && ti * 64 < V.T.n_pad) {
    __syncthreads();
    const int w = threadIdx.x;
    if (V.T.nkept && ti >= V.T.ncamt) {      // a tile of kept landmarks: 3 rows each, 21 to the tile
      if (w < 64 && (w >= 63 || (ti - V.T.ncamt) * 21 + w / 3 >= V.T.nkept)) base[(size_t)w * V.T.ldS + w] = V.damp_s;
    } else if (w < 64 && (w >= V.T.per_tile * V.T.dof || ti * V.T.per_tile + w / V.T.dof >= V.nfree)) base[(size_t)w * V.T.ldS + w] = V.damp_s;
  }
}

// Both accumulations in ONE launch (they are independent of each other): workgroups [0, nb_pose) take the cameras -- the
// longer job, so it starts first --, the next nb_point the landmarks (two dependent 14 us launches before), and the rest
// empty the reduced system for the trial that follows: every trial is preceded by a linearisation, the factor of the last
// trial is dead by then, and this launch runs while the host decides -- the trial's own first launch shrinks to the 79
// landmark workgroups.
// with_max: the launch also delivers max |diag| over Hpp and Hll (computeLambdaInit; k_max_diag as a launch of its own before).
__global__ void __launch_bounds__(256) k_accum(BaView V, int nb_pose, int nb_point, const double* __restrict__ spec, BaPublish pub, int with_max) {
  if (spec && *spec == -2.0) return;   // the device-side decision: accepted, and the optimisation ends with it -- nobody reads this linearisation
  double m;
  if ((int)blockIdx.x < nb_pose) m = V.schur_wide ? pose_accum_body<true>(V, blockIdx.x) : pose_accum_body<false>(V, blockIdx.x);
  else if ((int)blockIdx.x < nb_pose + nb_point) m = point_accum_body(V, blockIdx.x - nb_pose, spec);
  else { clear_tile(V, blockIdx.x - nb_pose - nb_point); return; }
  if (with_max) block_reduce_publish<true>(m, V.partial2, pub, nb_pose + nb_point);
}

// max |diag| over Hpp and Hll (computeLambdaInit) -> host, grid-wide with the last workgroup finishing the reduction.
__global__ void __launch_bounds__(256) k_max_diag(BaView V, BaPublish pub) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  double m = 0;
  if (i < V.nfree * 6) m = fabs(V.Hpp[36 * (size_t)(i / 6) + 7 * (i % 6)]);
  if (i < V.L * 3 && V.pt_start[i / 3 + 1] > V.pt_start[i / 3]) m = fmax(m, fabs(V.Hll[9 * (size_t)(i / 3) + 4 * (i % 3)]));
  block_reduce_publish<true>(m, V.partial2, pub);
}

// ------------------------------------------------------------------------------------------ K9
__device__ __forceinline__ void dinv_landmark(const BaView& V, int l) {
  const double lambda = ba_lambda(V);
  if (l >= V.L) return;
  if (V.pt_start[l + 1] == V.pt_start[l]) return;  // landmark without observation: not a vertex of the graph
  if (V.T.nkept && V.kept_slot[l] >= 0) { dinv_kept(V, l); return; }
  dinv_apply(V.Hll + 9 * (size_t)l, V.bl + 3 * (size_t)l, lambda, V.Dinv + 9 * (size_t)l, V.db + 3 * (size_t)l);
}
__global__ void __launch_bounds__(256) k_dinv(BaView V) { dinv_landmark(V, blockIdx.x * 256 + threadIdx.x); }

// One wave per non-zero lower block (i1 >= i2) of the reduced camera matrix:
//   S[i1,i2] = Hpp[i1] (+lambda I) if i1 == i2  -  sum over co-observed landmarks of W1 Dinv W2^T
// `pairs` lists (edge of pose i1, edge of pose i2) per block (symbolic structure built once on host).
// Gather form: the pairs of a block reference W rows (144 B) and Dinv blocks (72 B) scattered over tens of MB.  Read
// lane-per-pair, every load instruction touches 64 different cache lines and the kernel runs at the texture addresser's
// line rate (measured 75 us, whatever the occupancy).  So a wave stages 32 pairs at a time through LDS with CHUNK-PARALLEL
// loads -- consecutive lanes read consecutive 16-byte chunks of the same row: ~7 rows per instruction instead of 64 -- and
// then computes from LDS, two lanes per pair (lane half hf owns rows 3 hf .. 3 hf + 2 of the 6x6 product).  Summation order:
// pair slots p, p + 32, ... per lane, then the xor-butterfly over the 32 slots -- fixed, identical on every run.
constexpr int kSchurStagePairs = 32, kSchurRow = 45;   // doubles per staged pair: W1 (18) | W2 (18) | Dinv (9); odd dword-pair stride: conflict-free
template <int NW>   // waves of the workgroup = waves sharing one block
__device__ __forceinline__ void schur_blocks_body(const BaView& V, int block) {
  __shared__ double s_stage[NW][kSchurStagePairs * kSchurRow];
  __shared__ int32_t s_idx[NW][3][kSchurStagePairs];
  const double lambda = ba_lambda(V);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int blk = block;                                   // one block per WORKGROUP: its stages are dealt over the four waves
  const int i1 = V.blk_i1[blk], i2 = V.blk_i2[blk];
  const int hf = lane & 1, slot = lane >> 1;
  double* stage = s_stage[wave];
  int32_t (*idx)[kSchurStagePairs] = s_idx[wave];
  double acc[18];
#pragma unroll
  for (int i = 0; i < 18; i++) acc[i] = 0;
  // Software pipeline over the stages of the block (a wave walks its stages serially, so every dependent global round trip
  // inside a stage is paid n_stages times: measured 2.1 us per stage, 12 stages for the largest blocks): the (edge, edge, point)
  // indices are fetched two stages ahead, the rows one stage ahead into registers; a stage then costs max(compute, one load
  // latency) instead of three latencies plus the compute.
  constexpr int kIt = (kSchurStagePairs * 9 + 63) / 64;
  const int t_beg = V.blk_start[blk], t_end = V.blk_start[blk + 1];
  const int nst = (t_end - t_beg + kSchurStagePairs - 1) / kSchurStagePairs;
  auto load_idx = [&](int st, int& k1, int& k2, int& pt) {
    const int t = t_beg + st * kSchurStagePairs + lane;
    k1 = k2 = pt = 0;
    if (st < nst && lane < kSchurStagePairs && t < t_end) { k1 = V.pair_k1[t]; k2 = V.pair_k2[t]; pt = V.pair_pt[t]; }
  };
  double2 rw1[kIt], rw2[kIt];
  double rd[kIt];
  auto load_rows = [&](int st) {     // reads the indices of stage `st` from LDS
    const int np = min(kSchurStagePairs, t_end - (t_beg + st * kSchurStagePairs));
#pragma unroll
    for (int i = 0; i < kIt; i++) {
      const int c = i * 64 + lane;
      const int pr = (c * 57) >> 9, part = c - 9 * pr;     // c / 9 for c < 512
      if (pr < np) {
        rw1[i] = *reinterpret_cast<const double2*>(V.e_W + (size_t)idx[0][pr] * 18 + 2 * part);
        rw2[i] = *reinterpret_cast<const double2*>(V.e_W + (size_t)idx[1][pr] * 18 + 2 * part);
        rd[i] = V.Dinv[9 * (size_t)idx[2][pr] + part];
      }
    }
  };
  int a1, a2, a3, b1, b2, b3;
  load_idx(wave, a1, a2, a3);
  load_idx(wave + NW, b1, b2, b3);
  if (lane < kSchurStagePairs) { idx[0][lane] = a1; idx[1][lane] = a2; idx[2][lane] = a3; }
  __builtin_amdgcn_wave_barrier();
  if (wave < nst) load_rows(wave);
  for (int st = wave; st < nst; st += NW) {
    const int np = min(kSchurStagePairs, t_end - (t_beg + st * kSchurStagePairs));
    __builtin_amdgcn_wave_barrier();                       // stage st - 1 has been consumed (DS operations of a wave execute in order)
#pragma unroll
    for (int i = 0; i < kIt; i++) {
      const int c = i * 64 + lane;
      const int pr = (c * 57) >> 9, part = c - 9 * pr;
      if (pr < np) {
        double* row = stage + pr * kSchurRow;
        row[2 * part] = rw1[i].x; row[2 * part + 1] = rw1[i].y;
        row[18 + 2 * part] = rw2[i].x; row[18 + 2 * part + 1] = rw2[i].y;
        row[36 + part] = rd[i];
      }
    }
    if (st + NW < nst) {
      if (lane < kSchurStagePairs) { idx[0][lane] = b1; idx[1][lane] = b2; idx[2][lane] = b3; }
      __builtin_amdgcn_wave_barrier();
      load_rows(st + NW);                                  // in flight while stage st is computed
      load_idx(st + 2 * NW, b1, b2, b3);
    }
    __builtin_amdgcn_wave_barrier();
    if (slot < np) {
      const double* row = stage + slot * kSchurRow;
      const double* W1 = row + 9 * hf;                     // rows 3 hf .. 3 hf + 2 of W1 (6 x 3, row-major)
      const double* W2 = row + 18;
      const double* D = row + 36;
      double WD[9];
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) WD[3 * a + b] = W1[3 * a] * D[b] + W1[3 * a + 1] * D[3 + b] + W1[3 * a + 2] * D[6 + b];
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 6; b++) acc[6 * a + b] += WD[3 * a] * W2[3 * b] + WD[3 * a + 1] * W2[3 * b + 1] + WD[3 * a + 2] * W2[3 * b + 2];
    }
  }
  // Sum over the 32 pair slots THROUGH LDS: every lane parks its 18 partial sums in the (now idle) stage buffer, then lane
  // (hf, a, b) adds the 32 slots of its output in slot order.  ds_bpermute_b32 -- what __shfl_xor compiles to -- occupies the
  // CU's LDS unit for 24 cycles per instruction (tools/valu_issue2.hip): the 180 of them a double-precision butterfly over
  // 18 values needs were ~30 us of this kernel; 18 ds_write_b64 + 32 ds_read_b64 are ~200 cycles.
  __builtin_amdgcn_wave_barrier();
  {
    static_assert(2 * kSchurStagePairs * 19 <= kSchurStagePairs * kSchurRow, "the parking area reuses the stage buffer");
    double* red = stage + (size_t)lane * 19;                // 19-double pitch: odd dword-pair stride, conflict-free both ways
    if (lane < 2 * kSchurStagePairs) {
#pragma unroll
      for (int i = 0; i < 18; i++) red[i] = acc[i];
    }
  }
  if (NW > 1) __syncthreads(); else __builtin_amdgcn_wave_barrier();
  if (threadIdx.x < 36) {
    const int ohf = lane / 18, oi = lane - 18 * ohf;        // output (row 3 ohf + oi / 6, column oi % 6)
    double v = 0;
    for (int w = 0; w < NW; w++) {                          // waves in order, slots in order: a fixed summation order
      const double* st_w = s_stage[w];
#pragma unroll 8
      for (int sl = 0; sl < kSchurStagePairs; sl++) v += st_w[(size_t)(2 * sl + ohf) * 19 + oi];
    }
    const int ra = 3 * ohf + oi / 6, cb = oi % 6;
    v = -v;
    if (i1 == i2) v += V.Hpp[36 * (size_t)i1 + 6 * ra + cb] + (ra == cb ? lambda * V.damp_s : 0.0);
    V.T.S[(size_t)(ba_row(i1) + ra) * V.T.ldS + ba_row(i2) + cb] = v;
  }
}

// bschur[i] = bp[i] - sum_{edges k of camera i} W_k (Dinv bl)_{point(k)}  -> augmented row n of S.
// SPLIT = false: one wave per camera (NW cameras per workgroup) -- the global problem has hundreds of cameras, and the rhs hides
// under the block workgroups.  SPLIT = true (BaView::schur_wide, a local-BA window): ONE camera per workgroup, its edges dealt
// over the NW waves (wave w takes edges w*64 + lane, then + 64 NW, ...): twenty cameras of 500 edges each were twenty waves
// walking three dependent global round trips per 256 edges, 27 us -- longer than the blocks.  Fixed summation order either way:
// per lane in edge order, xor butterfly over the lanes, then (SPLIT) the waves in order.
template <int NW, bool SPLIT>
__device__ __forceinline__ void schur_rhs_body(const BaView& V, int block) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fi = SPLIT ? block : block * NW + wave;
  if (fi >= V.nfree) return;
  const int p = V.free_pose[fi];
  double acc[6] = {0, 0, 0, 0, 0, 0};
  // four edges per lane in flight: edge index -> (W row, landmark index -> Dinv bl) is a chain of three global round trips; same
  // summation order as one after the other
  const int e_end = V.ps_start[p + 1];
  const int first = V.ps_start[p] + lane + (SPLIT ? 64 * wave : 0), step = SPLIT ? 64 * NW : 64;
  for (int i0 = first; i0 < e_end; i0 += 4 * step) {
    int k[4], pt[4];
#pragma unroll
    for (int u = 0; u < 4; u++) k[u] = (i0 + step * u < e_end) ? V.ps_edges[i0 + step * u] : -1;
#pragma unroll
    for (int u = 0; u < 4; u++) pt[u] = V.e_point[max(k[u], 0)];
    double Wv[4][18], dv[4][3];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const double* W = V.e_W + (size_t)max(k[u], 0) * 18;
      const double* db = V.db + 3 * (size_t)pt[u];
#pragma unroll
      for (int j = 0; j < 18; j++) Wv[u][j] = W[j];
      dv[u][0] = db[0]; dv[u][1] = db[1]; dv[u][2] = db[2];
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (k[u] < 0) continue;
#pragma unroll
      for (int a = 0; a < 6; a++) acc[a] += Wv[u][3 * a] * dv[u][0] + Wv[u][3 * a + 1] * dv[u][1] + Wv[u][3 * a + 2] * dv[u][2];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int a = 0; a < 6; a++) acc[a] += __shfl_xor(acc[a], off);
  if (SPLIT) {
    __shared__ double s_w[NW][6];
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < 6; a++) s_w[wave][a] = acc[a];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
      double t = 0;
      for (int w = 0; w < NW; w++) t += s_w[w][threadIdx.x];
      V.T.S[(size_t)V.T.n_pad * V.T.ldS + ba_row(fi) + threadIdx.x] = V.bp[6 * (size_t)fi + threadIdx.x] - t;
    }
    if (fi == 0 && threadIdx.x == 0) V.T.S[(size_t)V.T.n_pad * V.T.ldS + V.T.n_pad] = 1e200 * V.damp_s;  // augmented corner: keeps the last pivot positive
    return;
  }
  if (lane == 0) {
    for (int a = 0; a < 6; a++) V.T.S[(size_t)V.T.n_pad * V.T.ldS + ba_row(fi) + a] = V.bp[6 * (size_t)fi + a] - acc[a];
    if (fi == 0) V.T.S[(size_t)V.T.n_pad * V.T.ldS + V.T.n_pad] = 1e200 * V.damp_s;  // augmented corner: keeps the last pivot positive
  }
}

// The three rows of kept landmark j (TileSystem::kept_list): Hll + lambda I on the diagonal, the transposed Hpl block of every observation
// by a free camera left of it (dvm_ba_set_problem keeps no landmark with two observations from one camera: every block is written
// once), bl in the rhs row.  The tiles were emptied for this trial like every other non-zero tile.
__device__ __forceinline__ void schur_kept_body(const BaView& V, int j) {
  if (j >= V.T.nkept) return;
  const int l = V.T.kept_list[j];
  const int row0 = 64 * (V.T.ncamt + j / 21) + 3 * (j % 21);
  const double lambda = ba_lambda(V);
  double* const Sr = V.T.S + (size_t)row0 * V.T.ldS;
  const int i0 = V.pt_start[l], i1 = V.pt_start[l + 1];
  for (int i = i0 + (int)threadIdx.x; i < i1; i += (int)blockDim.x) {
    const int fi = V.pt_fi[i];
    if (fi < 0) continue;
    const double* W = V.e_W + (size_t)V.pt_edges[i] * 18;       // 6 (camera) x 3 (landmark)
    const int c0 = ba_row(fi);
#pragma unroll
    for (int bb = 0; bb < 3; bb++)
#pragma unroll
      for (int a = 0; a < 6; a++) Sr[(size_t)bb * V.T.ldS + c0 + a] = W[3 * a + bb];
  }
  if (threadIdx.x < 9) {
    const int a = threadIdx.x / 3, c = threadIdx.x % 3;
    if (c <= a) Sr[(size_t)a * V.T.ldS + row0 + c] = V.Hll[9 * (size_t)l + 3 * a + c] + (a == c ? lambda * V.damp_s : 0.0);
  } else if (threadIdx.x < 12) {
    V.T.S[(size_t)V.T.n_pad * V.T.ldS + row0 + (threadIdx.x - 9)] = V.bl[3 * (size_t)l + (threadIdx.x - 9)];
  }
}

// The reduced system and its right-hand side in ONE launch (independent of each other; both only need Dinv / db of the
// prologue): workgroups [0, nb_blk) build the 6x6 blocks, the rest the rhs row.
// Waves per block: 2 for the global problem (thousands of blocks of ~180 pairs: 12 KB of LDS per wave, every block resident at
// once), 8 for a local-BA window (BaView::schur_wide: ~100 blocks of ~500 pairs -- with two waves a block was eight dependent
// stages of gathers per wave on a chip that is otherwise empty: 28 us for 45 000 pairs).  The stages of a block are dealt
// round-robin over its waves and the waves' partial sums are added in wave order: deterministic for either width.
constexpr int kSchurWaves = 2, kSchurWavesWide = 8;
template <int kNW>
__global__ void __launch_bounds__(64 * kNW) k_schur(BaView V, int nb_blk, int nb_chunk, int nb_rhs, int* __restrict__ fail_reset) {
  constexpr int kSchurWaves = kNW;
  // speculative launch (ba_launch_schur_speculative): the damping comes from the device-side decision; a negative value = the
  // trial before this one was rejected, the host will start the next one itself.  There is no prologue launch in front of a
  // speculative one: the Cholesky failure flag is reset here.
  if (fail_reset) {
    if (*V.lambda < 0) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) *fail_reset = 0;
  }
  // The rhs workgroups come FIRST: a camera's rhs is one wave walking ~320 edges (17 us on its own); dispatched behind
  // thousands of block workgroups it would start late and set the kernel's tail.
  if ((int)blockIdx.x < nb_rhs) { schur_rhs_body<kSchurWaves, kNW == kSchurWavesWide>(V, blockIdx.x); return; }
  // XCD-aware order: workgroups are dealt round-robin over the 8 XCDs, each with its own 4 MB L2.  Workgroup b takes block
  // group (b % 8) * nb_chunk + b / 8, so an XCD works through a CONTIGUOUS run of the (camera-sorted) block list: the W rows
  // of its ~60 cameras (46 KB each) stay in that L2.
  const int b = (int)blockIdx.x - nb_rhs;
  if (b >= 8 * nb_chunk) { schur_kept_body(V, b - 8 * nb_chunk); return; }      // the rows of a kept landmark (behind the block workgroups)
  const int g = (b & 7) * nb_chunk + (b >> 3);
  if (g < nb_blk) schur_blocks_body<kSchurWaves>(V, g);
}

// Start of a BA trial: the damped landmark blocks are inverted (k_dinv); the Cholesky failure flag is reset on the way.  (The
// reduced system was emptied by the linearisation's launch, k_accum.)
__global__ void __launch_bounds__(256) k_trial_prologue(BaView V, int* __restrict__ fail) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *fail = 0;
  dinv_landmark(V, blockIdx.x * 256 + threadIdx.x);
}

// ----------------------------------------------------------------------------------------- K11
// xl = Dinv (bl - sum_k W_k^T xp[pose(k)])   (block_solver.hpp:459-483); thread per landmark.
// Eight lanes per landmark (a landmark of the BASELINE problem has eight observations): lane j takes edges j, j + 8, ...;
// the partial sums meet by three DPP steps inside the group of eight (quad swaps, then the half-row mirror) -- a fixed
// order.  A thread per landmark walked its edges one dependent gather after the other, on 79 workgroups (19 us).
__device__ __forceinline__ double dpp_xor_add(double v, int ctrl_is) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  if (ctrl_is == 0) { lo = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xF, 0xF, false); hi = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xF, 0xF, false); }        // quad_perm [1,0,3,2]
  else if (ctrl_is == 1) { lo = __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xF, 0xF, false); hi = __builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xF, 0xF, false); }   // quad_perm [2,3,0,1]
  else { lo = __builtin_amdgcn_update_dpp(0, lo, 0x141, 0xF, 0xF, false); hi = __builtin_amdgcn_update_dpp(0, hi, 0x141, 0xF, 0xF, false); }                  // row_half_mirror
  return v + __hiloint2double(hi, lo);
}
// Landmark back substitution, oplus of cameras and landmarks into the TRIAL state and the terms of computeScale =
// sum x (lambda x + b) in ONE launch (oplus: se3quat.h:212-240, types_six_dof_expmap.h:71-74): workgroups [0, nb_pose)
// update the cameras (thread per camera), the rest the landmarks; every workgroup feeds the grid-wide reduction.
__global__ void __launch_bounds__(256) k_point_backsub(BaView V, BaPublish pub, int nb_pose, const int* __restrict__ fail) {
  const double lambda = ba_lambda(V);
  double sc = 0;
  const bool failed = fail && *fail != 0;   // the reduced solve failed: x (cameras: untouched by the back substitution) and xl keep the last good values
  if ((int)blockIdx.x < nb_pose) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < V.nfree) {
      const int p = V.free_pose[i];
      const double* u = V.T.x + 6 * (size_t)i;
      const double* b = V.bp + 6 * (size_t)i;
#pragma unroll
      for (int a = 0; a < 6; a++) sc += u[a] * (lambda * V.damp_s * u[a] + b[a]);
      double T[7];
#pragma unroll
      for (int a = 0; a < 7; a++) T[a] = V.poses[7 * (size_t)p + a];
      se3_oplus(T, u, T);
#pragma unroll
      for (int a = 0; a < 7; a++) V.poses_new[7 * (size_t)p + a] = T[a];
    }
  } else {
    const int g = ((int)blockIdx.x - nb_pose) * 256 + threadIdx.x;
    const int l = g >> 3, j = g & 7;
    const bool live = l < V.L;
    double t[3] = {0, 0, 0};
    int i0 = 0, i1 = 0;
    if (live) { i0 = V.pt_start[l]; i1 = V.pt_start[l + 1]; }
    for (int i = i0 + j; i < i1; i += 8) {
      const int k = V.pt_edges[i];
      const int fi = V.pt_fi[i];
      if (fi < 0) continue;
      const double* W = V.e_W + (size_t)k * 18;
      const double* xp = V.T.x + 6 * (size_t)fi;
#pragma unroll
      for (int b = 0; b < 3; b++)
#pragma unroll
        for (int a = 0; a < 6; a++) t[b] += W[3 * a + b] * xp[a];
    }
#pragma unroll
    for (int b = 0; b < 3; b++) {
      t[b] = dpp_xor_add(t[b], 0);
      t[b] = dpp_xor_add(t[b], 1);
      t[b] = dpp_xor_add(t[b], 2);
    }
    if (live && j == 0) {
      const int n = 6 * V.nfree;
      double* xl = V.T.x + n + 3 * (size_t)l;
      if (i1 == i0) {
        xl[0] = xl[1] = xl[2] = 0;
      } else {
        const double* bl = V.bl + 3 * (size_t)l;
        const double c[3] = {bl[0] - t[0], bl[1] - t[1], bl[2] - t[2]};
        const double* D = V.Dinv + 9 * (size_t)l;
        double u[3];
        u[0] = D[0] * c[0] + D[1] * c[1] + D[2] * c[2];
        u[1] = D[3] * c[0] + D[4] * c[1] + D[5] * c[2];
        u[2] = D[6] * c[0] + D[7] * c[1] + D[8] * c[2];
        // (block_solver.hpp:445-446 returns before the landmark part); a kept landmark is an unknown of the reduced system: the back
        // substitution has written its x already
        if (failed || (V.T.nkept && V.kept_slot[l] >= 0)) { u[0] = xl[0]; u[1] = xl[1]; u[2] = xl[2]; }
        const double* X = V.points + 3 * (size_t)l;
        double* Xn = V.points_new + 3 * (size_t)l;
#pragma unroll
        for (int a = 0; a < 3; a++) { xl[a] = u[a]; sc += u[a] * (lambda * u[a] + bl[a]); Xn[a] = X[a] + u[a]; }
      }
    }
  }
  block_reduce_publish<false>(sc, V.partial2, pub);
}

// per-edge depth sign at the current state (EdgeSE3ProjectXYZ::isDepthPositive)
__global__ void __launch_bounds__(256) k_edge_depth(BaView V, uint8_t* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= V.E) return;
  const double* T = V.poses + 7 * (size_t)V.e_pose[k];
  const double* X = V.points + 3 * (size_t)V.e_point[k];
  double R[9];
  quat_to_R(T + 3, R);
  const double z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + T[2];
  out[k] = z > 0.0;
}

// ------------------------------------------------------------------------------------- launchers
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

void ba_launch_edge_eval(hipStream_t s, const BaView& V, bool jac, const BaPublish& pub) {
  const int nb = cdiv(V.E, 256);
  if (V.cam_model == dvm_cam::kKannalaBrandt8) {
    if (jac) hipLaunchKernelGGL((k_edge_eval<true, PoseCamKB8>), dim3(nb), dim3(256), 0, s, V, pub);
    else hipLaunchKernelGGL((k_edge_eval<false, PoseCamKB8>), dim3(nb), dim3(256), 0, s, V, pub);
  } else {
    if (jac) hipLaunchKernelGGL((k_edge_eval<true, PoseCamPinhole>), dim3(nb), dim3(256), 0, s, V, pub);
    else hipLaunchKernelGGL((k_edge_eval<false, PoseCamPinhole>), dim3(nb), dim3(256), 0, s, V, pub);
  }
}
void ba_launch_accum(hipStream_t s, const BaView& V, const double* spec, const BaPublish* max_pub) {
  const int nb_pose = V.nfree > 0 ? (V.schur_wide ? V.nfree : cdiv(V.nfree, 4)) : 0;   // (wide: a workgroup per camera)
  const int nb_point = cdiv(V.L, 256);
  BaPublish none;
  std::memset(&none, 0, sizeof(none));
  hipLaunchKernelGGL(k_accum, dim3(nb_pose + nb_point + (V.nfree > 0 ? V.T.n_nz : 0)), dim3(256), 0, s, V, nb_pose, nb_point, spec,
                     max_pub ? *max_pub : none, max_pub ? 1 : 0);
}
void ba_launch_max_diag(hipStream_t s, const BaView& V, const BaPublish& pub) {
  hipLaunchKernelGGL(k_max_diag, dim3(cdiv(std::max(3 * V.L, 6 * V.nfree), 256)), dim3(256), 0, s, V, pub);
}
static void launch_schur_kernel(hipStream_t s, const BaView& V, int* fail_reset) {
  const int nb_blk = V.nblk, nb_chunk = cdiv(nb_blk, 8);   // one workgroup per 6x6 block
  const int nw = V.schur_wide ? kSchurWavesWide : kSchurWaves;
  const int nb_rhs = ((V.schur_wide ? V.nfree : cdiv(V.nfree, nw)) + 7) & ~7;   // (wide: a workgroup per camera) a multiple of 8 keeps the XCD phase of the block workgroups
  if (V.schur_wide) hipLaunchKernelGGL(k_schur<kSchurWavesWide>, dim3(nb_rhs + 8 * nb_chunk + V.T.nkept), dim3(64 * kSchurWavesWide), 0, s, V, nb_blk, nb_chunk, nb_rhs, fail_reset);
  else hipLaunchKernelGGL(k_schur<kSchurWaves>, dim3(nb_rhs + 8 * nb_chunk + V.T.nkept), dim3(64 * kSchurWaves), 0, s, V, nb_blk, nb_chunk, nb_rhs, fail_reset);
}
void ba_launch_schur(hipStream_t s, const BaView& V, int* d_fail) {
  const int nb_dinv = cdiv(V.L, 256);
  hipLaunchKernelGGL(k_trial_prologue, dim3(nb_dinv), dim3(256), 0, s, V, d_fail);
  if (V.nfree == 0) return;
  launch_schur_kernel(s, V, nullptr);
}
void ba_launch_schur_speculative(hipStream_t s, const BaView& V, int* d_fail) {
  if (V.nfree == 0 || !V.lambda) return;
  launch_schur_kernel(s, V, d_fail);
}
__global__ void __launch_bounds__(256) k_clear_tiles(BaView V) { clear_tile(V, blockIdx.x); }
void ba_launch_clear_tiles(hipStream_t s, const BaView& V) {
  if (V.nfree > 0 && V.T.n_nz > 0) hipLaunchKernelGGL(k_clear_tiles, dim3(V.T.n_nz), dim3(256), 0, s, V);
}
void ba_launch_backsub_update(hipStream_t s, const BaView& V, const BaPublish& pub, const int* d_fail) {
  const int nb_pose = cdiv(std::max(V.nfree, 1), 256);
  hipLaunchKernelGGL(k_point_backsub, dim3(nb_pose + cdiv(8 * V.L, 256)), dim3(256), 0, s, V, pub, nb_pose, d_fail);
}
__global__ void __launch_bounds__(256) k_pack_tiles(BaView V, double* __restrict__ buf, int unpack) {
  const int ti = V.T.nz_tiles[2 * blockIdx.x], tj = V.T.nz_tiles[2 * blockIdx.x + 1];
  double* base = V.T.S + (size_t)ti * 64 * V.T.ldS + tj * 64;
  double* b = buf + (size_t)blockIdx.x * 4096;
  for (int i = threadIdx.x; i < 64 * 32; i += 256) {
    const int r = i >> 5, c2 = i & 31;
    double2* g = reinterpret_cast<double2*>(base + (size_t)r * V.T.ldS) + c2;
    double2* p = reinterpret_cast<double2*>(b + r * 64) + c2;
    if (unpack) *g = *p; else *p = *g;
  }
}
__global__ void __launch_bounds__(256) k_hpp_diag(BaView V, double* __restrict__ buf) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < V.nfree * 6) buf[i] = V.Hpp[36 * (size_t)(i / 6) + 7 * (i % 6)];
}
__global__ void __launch_bounds__(256) k_max_diag_sharded(BaView V, const double* __restrict__ hpp_diag, BaPublish pub) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  double m = 0;
  if (i < V.nfree * 6) m = fabs(hpp_diag[i]);
  if (i < V.L * 3 && V.pt_start[i / 3 + 1] > V.pt_start[i / 3]) m = fmax(m, fabs(V.Hll[9 * (size_t)(i / 3) + 4 * (i % 3)]));
  block_reduce_publish<true>(m, V.partial2, pub);
}
__global__ void __launch_bounds__(256) k_points_exchange(BaView V, double* __restrict__ buf, int scatter) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= V.L) return;
  const bool own = l % V.shard_world == V.shard_rank;   // by index, not by "has local edges": a landmark nobody observes keeps its value
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (scatter) V.points[3 * (size_t)l + k] = buf[3 * (size_t)l + k];
    else buf[3 * (size_t)l + k] = own ? V.points[3 * (size_t)l + k] : 0.0;
  }
}
void ba_launch_pack_tiles(hipStream_t s, const BaView& V, double* buf, bool unpack) {
  hipLaunchKernelGGL(k_pack_tiles, dim3(V.T.n_nz), dim3(256), 0, s, V, buf, unpack ? 1 : 0);
}
void ba_launch_hpp_diag(hipStream_t s, const BaView& V, double* buf) {
  hipLaunchKernelGGL(k_hpp_diag, dim3(cdiv(6 * V.nfree, 256)), dim3(256), 0, s, V, buf);
}
void ba_launch_max_diag_sharded(hipStream_t s, const BaView& V, const double* hpp_diag, const BaPublish& pub) {
  hipLaunchKernelGGL(k_max_diag_sharded, dim3(cdiv(std::max(3 * V.L, 6 * V.nfree), 256)), dim3(256), 0, s, V, hpp_diag, pub);
}
void ba_launch_points_exchange(hipStream_t s, const BaView& V, double* buf, bool scatter) {
  hipLaunchKernelGGL(k_points_exchange, dim3(cdiv(V.L, 256)), dim3(256), 0, s, V, buf, scatter ? 1 : 0);
}
void ba_launch_edge_depth(hipStream_t s, const BaView& V, uint8_t* d_out) {
  hipLaunchKernelGGL(k_edge_depth, dim3(cdiv(V.E, 256)), dim3(256), 0, s, V, d_out);
}

}  // namespace dvm
