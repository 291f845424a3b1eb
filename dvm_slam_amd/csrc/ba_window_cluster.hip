// dvm_slam_amd/csrc/ba_window_cluster.hip -- dvm_ba_optimize_windows_fast (k_ba_window_cluster): the optimizer of ba_window_seq.hip for MANY
// LocalBundleAdjustment windows per call (Optimizer.cc:1030-1387, one per agent): tree sums in a fixed order instead of the sequential ones,
// edges sorted camera-major with structure-of-arrays rows, a cluster of G = 1 / 2 / 4 / 8 workgroups per window separated by agent-scope phase
// barriers, the reduced system solved in workgroup 0's LDS.  Deterministic, independent of G; equal to the oracle to the general
// solver's contract (same LM trial sequence, 1e-6), not bit for bit (tests/test_gpu_ba_window_fast.py, tools/soak_r06.py).
// dvm_ba_optimize_windows_fast_cam / dvm_ba_pool_optimize_cam: the same kernel as a template on the camera (proj_edge.h), a dvm_camera_model
// per window, one launch per model type present in the call (tests/test_gpu_ba_window_fast_kb8.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ba_kernels.h"
#include "ba_window_cluster_tables.h"
#include "f64_spec.h"
#include "se3_f64.h"       // the small algebra, in the oracle's sequences

namespace dvm {

// device view of one window: pointers into its tables (one page-locked block, ClusterBuild::pack_fast) and into the call's staging block.
// The edges are SORTED camera-major on the host -- free cameras first, a camera's edges by landmark, the fixed cameras' edges behind
// them -- and the per-edge rows are structure-of-arrays with pitch Fp, so that a lane per edge reads and writes consecutive words.
// e_pose / e_point / e_obs / e_info are in that order; the first F edges are the free cameras' (the rows of W / T / B).
struct ClusterWin {
  int32_t P, L, E, F, nfree, nact, nblk, iterations;
  double fx, fy, cx, cy, delta;
  double *poses, *poses_t;            // [P][7] accepted / trial state
  double *pts, *pts_t;                // [L][3]
  double *out_poses, *out_pts;        // the accepted state at the end (what the host fetches)
  const int32_t *free_pose, *act_pt;  // [nfree], [nact]
  const int32_t *e_pose, *e_point;    // [E]
  const double *e_obs, *e_info;       // [E][2], [E]
  const int32_t *pt_start;            // [nact + 1] a landmark's range of pt_edges
  const int32_t *f_cam;               // [F] free camera index of the row
  double *rowA;                       // [E][12] A (2x3), w, wr0, wr1
  double *e_chi2, *e_rho;             // [E] chi2 in the caller's order (written at the end), rho(chi2) of the last evaluation in the sorted order
  uint8_t* e_depth;                   // [E] isDepthPositive() at the final state, the caller's order
  const int32_t *blk_ij;              // [nblk] i1 | i2 << 8
  double *Hpp, *bp, *HB, *x, *terms;  // [nfree][36], [6 nfree], [nact][12] = Hll (9) bl (3), [6 nfree + 3 nact] x 2
  dvm_ba_stats* stats;
  unsigned long long* prof;           // [16] shader-clock cycles per phase of the cluster's workgroup 0 (DVM_BA_WINDOW_PROF=1), or null
  int32_t Fp;                         // pitch of the rows: F rounded up to 64
  const int32_t *e_orig;              // [E] the edge's index in the caller's list (chi2 / depth go back there)
  const int32_t *e_lm;                // [E] active landmark of the edge
  const int32_t *cam_start;           // [nfree + 1] a free camera's edges
  const int32_t *pt_edges;            // [E] a landmark's edges (sorted indices, ascending: its free-camera rows come first), ranges pt_start
  const int32_t *bp_start;            // [nblk + 1] a block's (row of camera i1, row of camera i2) pairs, landmark order
  const int2* bp_pairs;
  const int32_t *sched_start, *sched_task;   // the Schur pass's tasks per wave of the cluster (8 G waves): task < nfree: rhs of that camera, else block task - nfree
  double *Bs, *Ws, *Ts, *Cs;          // [15][Fp] B (12) w wr0 wr1 | [18][Fp] W | [24][Fp] W Dinv (18), W Dinv bl (6) | [3][Fp] W^T x_p
  double *chi_s;                      // [E] chi2 of the last evaluation, sorted order
  // what the cluster's workgroups hand each other through global memory
  unsigned int *cl_ctr, *cl_tmo;      // arrival counter of the window's barriers, time-out word (both zeroed before every launch)
  double *Sblk, *rhsg;                // [nblk][36] the blocks of the reduced system as their owner waves leave them, [6 nfree]
  double *cl_part;                    // [4][8] partial sums of the eight fixed parts: chi2, scale terms, max |diag|
  double *cl_ctl;                     // [4] 0: the solve succeeded, 1: the stop word as the leader saw it
  float kb8[8];                       // k_ba_window_cluster<PoseCamKB8> only: mvParameters of the window's KannalaBrandt8 camera (fx, fy, cx, cy are not read then)
};

// ------------------------------------------------------------------------------------------------ the reduced system's solve
// (Its contract is a tolerance, not the column-by-column bits of the sequential-order kernel's win_cholesky:) six columns a step, with
//   * the right-hand side as row n of the matrix -- it sits behind the packed triangle, i.e. AT tri(n, 0): its panel entries ARE the forward
//     substitution's y, its trailing entries take the same subtractions as any other row -- no separate forward pass (one wave, 20
//     dependent steps: 16 us of a 310 us iteration);
//   * the 6 x 6 diagonal block factorised only by the waves that own panel rows (every thread of a wave for itself, as before) and by wave 0
//     -- eight waves doing it side by side shared four SIMDs: 1 800 cycles a step instead of 600 --, fused multiply-adds throughout;
//   * the trailing update on the FP64 matrix cores: A(i, j) -= sum_k L(i, k) L(j, k), k = 6 padded to 8, as two v_mfma_f64_16x16x4 per
//     16 x 16 tile of the lower triangle (rows from the step's first trailing row), tiles dealt round-robin to the eight waves.  The panel
//     copy Lp (pitch 9 doubles, columns 6 and 7 zero) supplies both operands.  A tile strictly below the diagonal whose sixteen rows all
//     exist takes the short path (one multiplication for its four row offsets, no masks); diagonal tiles and the last tile row the masked
//     one.  One entry at a time (six dependent multiply-subtract pairs behind seven LDS reads) the update was 1.5 us a step -- 30 of the
//     factorisation's 51 us.
// rinv[k] = 1 / L_kk and the diagonal block's own factor (rows k0 .. k0 + 5 of Lp, dead since their panel step) are what the backward
// substitution reads.  flag: an LDS word (the positivity verdict).
typedef double win_d4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ double w_rsqrt_fma(double v) {
  double y = __builtin_amdgcn_rsq(v);
  y = __builtin_fma(0.5 * y, __builtin_fma(-v * y, y, 1.0), y);
  y = __builtin_fma(0.5 * y, __builtin_fma(-v * y, y, 1.0), y);
  return y;
}
__device__ bool win_cholesky_rhs(double* __restrict__ S, double* __restrict__ rinv, double* __restrict__ Lp, int n, int* __restrict__ flag,
                                 unsigned long long* prof) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // (uniform: the tile loop below branches on it)
  constexpr int NW = kWinThreads / 64, LPP = kLpPitch;
  // (phase clocks of thread 0, kept in registers and added to prof[12..15] at the end: a read-modify-write of global memory per lap would put
  //  its latency into the phase that follows)
  unsigned long long tp = (prof && tid == 0) ? __builtin_amdgcn_s_memtime() : 0ull, pacc[4] = {0, 0, 0, 0};
  auto lapc = [&](int slot) { if (prof && tid == 0) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const unsigned long long t = __builtin_amdgcn_s_memtime(); pacc[slot - 12] += t - tp; tp = t; } };
  if (tid == 0) *flag = 1;
  __syncthreads();
  for (int k0 = 0; k0 < n; k0 += 6) {
    const int base = k0 + 6, rows = n + 1 - base;              // trailing rows base .. n (row n = the right-hand side)
    if (wave == 0 || 64 * wave < rows) {
      double Ld[21], rdg[6];
      bool ok = true;
#pragma unroll
      for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int c = 0; c <= a; c++) {
          double v = S[tri(k0 + a, k0 + c)];
#pragma unroll
          for (int k = 0; k < c; k++) v = __builtin_fma(-Ld[a * (a + 1) / 2 + k], Ld[c * (c + 1) / 2 + k], v);
          if (a == c) {
            if (!(v > 0)) ok = false;
            rdg[a] = w_rsqrt_fma(v > 0 ? v : 1.0);
            Ld[a * (a + 1) / 2 + a] = v;
          } else Ld[a * (a + 1) / 2 + c] = v * rdg[c];
        }
      }
      lapc(12);
      const int i = base + tid;
      if (i <= n) {
        double* row = S + tri(i, k0);
        double l[6];
#pragma unroll
        for (int c = 0; c < 6; c++) {
          double v = row[c];
#pragma unroll
          for (int k = 0; k < c; k++) v = __builtin_fma(-l[k], Ld[c * (c + 1) / 2 + k], v);
          l[c] = v * rdg[c];
        }
        double* lp = Lp + LPP * i;
#pragma unroll
        for (int c = 0; c < 6; c++) { row[c] = l[c]; lp[c] = l[c]; }
        lp[6] = 0.0; lp[7] = 0.0;
      }
      if (tid == 0) {
        if (!ok) *flag = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
          rinv[k0 + a] = rdg[a];
#pragma unroll
          for (int c = 0; c < a; c++) Lp[LPP * (k0 + a) + c] = Ld[a * (a + 1) / 2 + c];
        }
      }
      lapc(13);
    }
    __syncthreads();
    lapc(14);
    if (*flag == 0) break;                       // (uniform: read behind the barrier; nobody writes it before the next one)
    // ---- trailing update, 16 x 16 tiles of rows / columns base + 16 t; tile t = ti (ti + 1) / 2 + tj goes to wave t mod 8
    const int T = (rows + 15) >> 4, ntiles = T * (T + 1) / 2;
    const int lr = lane & 15, lq = lane >> 4;
    int ti = 0, tj = wave;
    while (tj > ti) { tj -= ti + 1; ti++; }
    for (int t = wave; t < ntiles; t += NW) {
      const int i0 = base + 16 * ti, j0 = base + 16 * tj;
      const int j = j0 + lr, ifirst = i0 + lq;
      if (ti > tj && i0 + 15 <= n) {
        const double* ra = Lp + LPP * (i0 + lr) + lq;
        const double* rb = Lp + LPP * (j0 + lr) + lq;
        const double a0 = ra[0], b0 = rb[0], a1 = ra[4], b1 = rb[4];
        double* e0 = S + tri(ifirst, j);                   // rows ifirst + 4 r: tri(i + 4, j) = tri(i, j) + 4 i + 10
        double* e1 = e0 + 4 * ifirst + 10;
        double* e2 = e1 + 4 * ifirst + 26;
        double* e3 = e2 + 4 * ifirst + 42;
        const double c0 = *e0, c1 = *e1, c2 = *e2, c3 = *e3;
        win_d4 acc = {0, 0, 0, 0};
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc, 0, 0, 0);
        *e0 = c0 - acc[0]; *e1 = c1 - acc[1]; *e2 = c2 - acc[2]; *e3 = c3 - acc[3];
      } else {
        const double* ra = Lp + LPP * min(i0 + lr, n) + lq;
        const double* rb = Lp + LPP * min(j0 + lr, n) + lq;
        const double a0 = ra[0], b0 = rb[0], a1 = ra[4], b1 = rb[4];
        double* e[4];
        double cur[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int i = ifirst + 4 * r;
          e[r] = (i > n || j > i || j >= n) ? nullptr : S + tri(i, j);
          cur[r] = e[r] ? *e[r] : 0.0;
        }
        win_d4 acc = {0, 0, 0, 0};
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; r++) if (e[r]) *e[r] = cur[r] - acc[r];
      }
      tj += NW;
      while (tj > ti) { tj -= ti + 1; ti++; }
    }
    lapc(15);
    __syncthreads();
    lapc(14);
  }
  if (prof && tid == 0) for (int i = 0; i < 4; i++) prof[12 + i] += pacc[i];
  return *flag != 0;
}
// backward substitution behind win_cholesky_rhs (rhs = row n of S holds y): x(i) = y(i) / L(i, i); y(j) -= L(i, j) x(i) for j < i, i
// descending, a camera's six unknowns per step.  ONE wave.
__device__ void win_backsubstitute(const double* __restrict__ S, const double* __restrict__ rinv, const double* __restrict__ Lp, double* __restrict__ rhs, int n) {
  const int lane = threadIdx.x & 63;
  for (int k0 = n - 6; k0 >= 0; k0 -= 6) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double x6[6];
#pragma unroll
    for (int a = 5; a >= 0; a--) {
      double v = rhs[k0 + a];
#pragma unroll
      for (int c = 5; c > a; c--) v = __builtin_fma(-Lp[kLpPitch * (k0 + c) + a], x6[c], v);        // (the block's own factor: win_cholesky_rhs left it in Lp)
      x6[a] = v * rinv[k0 + a];
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 6) { double xv = x6[0]; xv = lane == 1 ? x6[1] : xv; xv = lane == 2 ? x6[2] : xv; xv = lane == 3 ? x6[3] : xv; xv = lane == 4 ? x6[4] : xv; xv = lane == 5 ? x6[5] : xv; rhs[k0 + lane] = xv; }
    for (int j = lane; j < k0; j += 64) {
      double v = rhs[j];
#pragma unroll
      for (int a = 5; a >= 0; a--) v = __builtin_fma(-S[tri(k0 + a, j)], x6[a], v);
      rhs[j] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------ tree reductions (cluster form)
// Sums as trees in a FIXED order (deterministic, but not g2o's sequential order): partial sums per lane meet in four DPP steps and one
// LDS hop.  Used by the cluster form below (k_ba_window_cluster); the sequential-order kernel (k_ba_window) does not use them.
template <int CTRL>
__device__ __forceinline__ double w_dpp_add(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, false);
  return v + __hiloint2double(hi, lo);
}
// the sum over a DPP row (16 lanes), in all of its lanes: quad swaps, half-row mirror, row mirror
__device__ __forceinline__ double w_row_sum(double v) {
  v = w_dpp_add<0xB1>(v); v = w_dpp_add<0x4E>(v); v = w_dpp_add<0x141>(v); v = w_dpp_add<0x140>(v);
  return v;
}
// acc[0..N) of the 64 lanes -> lane i < N returns the wave's sum of acc[i] ((row0 + row1) + (row2 + row3)); wbuf: 4 * N doubles of LDS, this wave's
template <int N>
__device__ __forceinline__ double w_wave_reduce(double (&acc)[N], double* __restrict__ wbuf) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < N; i++) acc[i] = w_row_sum(acc[i]);
  __builtin_amdgcn_wave_barrier();      // (the previous use of wbuf has been read)
  if ((lane & 15) == 0) {
#pragma unroll
    for (int i = 0; i < N; i++) wbuf[(lane >> 4) * N + i] = acc[i];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  double r = 0.0;
  if (lane < N) r = (wbuf[lane] + wbuf[N + lane]) + (wbuf[2 * N + lane] + wbuf[3 * N + lane]);
  return r;
}

// ------------------------------------------------------------------------------------------------ the CLUSTER form
// dvm_ba_optimize_windows_fast: the optimizer with tree sums in a fixed order, on G workgroups per window (G = 1, 2, 4, 8).  One CU streams a window's ~23 MB per iteration through ONE 64 B/clk
// memory pipe with eight waves' worth of requests in flight (~40 GB/s): with K <= 32 windows on 256 CUs the other seven eighths of the
// chip idle.  Here every data-parallel phase is split over the cluster -- element ranges in EIGHT fixed parts (part p belongs to
// workgroup p % G: the partial sums and therefore the results do not depend on G), cameras / blocks round-robin over the cluster's
// waves -- and the phases are separated by cluster barriers (Guideline 16, counter form: every wave drains, lane 0 releases at agent
// scope, arrives on the window's counter, polls it relaxed, acquires).  The reduced system is solved by workgroup 0 (S in its LDS);
// every workgroup takes the LM decisions redundantly on the same words.  Correctness does not depend on where the workgroups run;
// the block -> window map only tries to keep a window's workgroups on one XCD (observed: block b runs on XCD b % 8).  Every spin is
// bounded: a barrier that times out (a workgroup of the cluster is not resident) raises cl_tmo and the whole cluster leaves; the
// host then solves the batch with G = 1, which needs no co-residency.
constexpr int kParts = 8;
struct ClusterCtx { int g, G; unsigned int epoch; bool dead; };

__device__ __forceinline__ bool cluster_barrier(const ClusterWin& W, ClusterCtx& C, int* s_flag) {
  if (C.G == 1) { __syncthreads(); return true; }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // every wave: its stores have left
  __syncthreads();
  C.epoch++;
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // (restated: the compiler may drop the wait behind buffer_wbl2)
    __hip_atomic_fetch_add(W.cl_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned int target = C.epoch * (unsigned int)C.G;
    int ok = 1;
    for (unsigned int spins = 0; __hip_atomic_load(W.cl_ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target; spins++) {
      __builtin_amdgcn_s_sleep(2);
      if ((spins & 63u) == 63u && __hip_atomic_load(W.cl_tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) { ok = 0; break; }
      if (spins > (1u << 20)) { __hip_atomic_store(W.cl_tmo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); ok = 0; break; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    *s_flag = ok;
  }
  __syncthreads();
  const bool ok = *s_flag != 0;
  __syncthreads();
  if (!ok) C.dead = true;
  return ok;
}
// the elements [lo, hi) of part p of n (fixed eight parts, multiples of 64)
__device__ __forceinline__ void part_range(int n, int p, int& lo, int& hi) {
  const int chunk = (((n + kParts - 1) / kParts) + 63) & ~63;
  lo = min(n, p * chunk); hi = min(n, lo + chunk);
}
// the partial sums of this workgroup's parts of v[0..n) -> W.cl_part[slot * 8 + part]
__device__ void cluster_partial_sums(const ClusterWin& W, const ClusterCtx& C, const double* __restrict__ v, int n, int slot, double* red) {
  __syncthreads();                    // (v's entries of this workgroup's parts were written by its own threads just before)
  for (int p = C.g; p < kParts; p += C.G) {
    int lo, hi;
    part_range(n, p, lo, hi);
    double s = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += kWinThreads) s += v[i];
    s = w_row_sum(s);
    __syncthreads();
    if ((threadIdx.x & 15) == 0) red[threadIdx.x >> 4] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
#pragma unroll
      for (int i = 0; i < kWinThreads / 16; i++) t += red[i];
      W.cl_part[slot * kParts + p] = t;
    }
  }
}
__device__ __forceinline__ double cluster_total(const ClusterWin& W, int slot) {
  double t = 0.0;
#pragma unroll
  for (int p = 0; p < kParts; p++) t += W.cl_part[slot * kParts + p];
  return t;
}
// Dinv and Dinv bl of a landmark from Hll | bl and the damping: formed where they are needed (the T rows, the back substitution) --
// the same operations on the same words give the same bits, and a phase (and its barrier) less
__device__ __forceinline__ void w_dinv(const double* __restrict__ h, double lambda, double* Di, double* d3) {
  double D[9];
#pragma unroll
  for (int i = 0; i < 9; i++) D[i] = h[i];
  const double g3[3] = {h[9], h[10], h[11]};
  D[0] += lambda; D[4] += lambda; D[8] += lambda;
  inv3(D, Di);
  mat3_vec(Di, g3, d3);
}

template <bool JAC, class CAM>
__device__ void cl_edge_pass(const ClusterWin& W, const ClusterCtx& C, const double* __restrict__ poses, const double* __restrict__ pts) {
  const CAM cam = win_cam<CAM>(W);
  const size_t Fp = (size_t)W.Fp;
  for (int p = C.g; p < kParts; p += C.G) {
    int lo, hi;
    part_range(W.E, p, lo, hi);
    for (int k = lo + threadIdx.x; k < hi; k += kWinThreads) {
      const int pi = W.e_pose[k], l = W.e_point[k];
      const double* T = poses + 7 * (size_t)pi;
      const double* X = pts + 3 * (size_t)l;
      double R[9];
      quat_to_R(T + 3, R);
      const ProjEdge<CAM> e(cam, R, T, X, W.e_obs[2 * k], W.e_obs[2 * k + 1], W.e_info[k]);
      double r0, r1;
      robustify(e.chi2, W.delta, r0, r1);
      W.chi_s[k] = e.chi2;
      W.e_rho[k] = r0;
      if (!JAC) continue;
      double A[6], B[12];
      e.jac_point(cam, R, A);
      const double w = e.w(r1), wr0 = e.wr0(r1), wr1 = e.wr1(r1);
      double2* oA = reinterpret_cast<double2*>(W.rowA + kRowA * (size_t)k);
      oA[0] = make_double2(A[0], A[1]); oA[1] = make_double2(A[2], A[3]); oA[2] = make_double2(A[4], A[5]);
      oA[3] = make_double2(w, wr0); oA[4] = make_double2(wr1, 0.0);
      if (k < W.F) {
        e.jac_pose(cam, B);     // (the pose half only for the rows that have one: a free camera's)
#pragma unroll
        for (int i = 0; i < 12; i++) W.Bs[i * Fp + k] = B[i];
        W.Bs[12 * Fp + k] = w; W.Bs[13 * Fp + k] = wr0; W.Bs[14 * Fp + k] = wr1;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
          for (int b2 = 0; b2 < 3; b2++) W.Ws[(3 * a + b2) * Fp + k] = proj_edge_hpl(w, B, A, a, b2);
      }
    }
  }
}
// Hll / bl of this workgroup's landmarks, Hpp / bp of its waves' cameras; mx = max |diagonal| over what it formed
__device__ double cl_accumulate(const ClusterWin& W, const ClusterCtx& C, double* wred) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t Fp = (size_t)W.Fp;
  double mx = 0.0;
  for (int p = C.g; p < kParts; p += C.G) {
    int lo, hi;
    part_range(W.nact, p, lo, hi);
    for (int li = lo + threadIdx.x; li < hi; li += kWinThreads) {
      double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, g3[3] = {0, 0, 0};
      for (int q = W.pt_start[li]; q < W.pt_start[li + 1]; q++) {
        const double2* Ap = reinterpret_cast<const double2*>(W.rowA + kRowA * (size_t)W.pt_edges[q]);
        const double2 a01 = Ap[0], a23 = Ap[1], a45 = Ap[2], ww = Ap[3], w1 = Ap[4];
        const double A[6] = {a01.x, a01.y, a23.x, a23.y, a45.x, a45.y};
        const double w = ww.x, wr0 = ww.y, wr1 = w1.x;
#pragma unroll
        for (int a = 0; a < 3; a++) {
          g3[a] += A[a] * wr0 + A[3 + a] * wr1;
#pragma unroll
          for (int b2 = 0; b2 < 3; b2++) h[3 * a + b2] += w * (A[a] * A[b2] + A[3 + a] * A[3 + b2]);
        }
      }
      double* o = W.HB + kRowH * (size_t)li;
#pragma unroll
      for (int i = 0; i < 9; i++) o[i] = h[i];
#pragma unroll
      for (int i = 0; i < 3; i++) o[9 + i] = g3[i];
      mx = fmax(mx, fmax(fabs(h[0]), fmax(fabs(h[4]), fabs(h[8]))));
    }
  }
  double* wbuf = wred + wave * 4 * 36;
  for (int i = C.g * (kWinThreads / 64) + wave; i < W.nfree; i += C.G * (kWinThreads / 64)) {
    double acc[27];
#pragma unroll
    for (int t = 0; t < 27; t++) acc[t] = 0.0;
    const int q1 = W.cam_start[i + 1];
    for (int q = W.cam_start[i] + lane; q < q1; q += 64) {
      double B[15];
#pragma unroll
      for (int j = 0; j < 15; j++) B[j] = W.Bs[j * Fp + q];
      const double w = B[12], wr0 = B[13], wr1 = B[14];
      int t = 0;
#pragma unroll
      for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int b2 = 0; b2 <= a; b2++) acc[t++] += w * (B[a] * B[b2] + B[6 + a] * B[6 + b2]);
      }
#pragma unroll
      for (int a = 0; a < 6; a++) acc[21 + a] += B[a] * wr0 + B[6 + a] * wr1;
    }
    const double tot = w_wave_reduce<27>(acc, wbuf);
    if (lane < 21) {
      int a = 0, r = lane; while (r > a) { r -= a + 1; a++; }
      const int b2 = r;
      W.Hpp[36 * (size_t)i + 6 * a + b2] = tot; W.Hpp[36 * (size_t)i + 6 * b2 + a] = tot;
      if (a == b2) mx = fmax(mx, fabs(tot));
    } else if (lane < 27) W.bp[6 * (size_t)i + (lane - 21)] = tot;
  }
  return mx;
}
// W Dinv | W Dinv bl of this workgroup's rows
__device__ void cl_t_rows(const ClusterWin& W, const ClusterCtx& C, double lambda) {
  const size_t Fp = (size_t)W.Fp;
  for (int p = C.g; p < kParts; p += C.G) {
    int lo, hi;
    part_range(W.F, p, lo, hi);
    for (int r = lo + threadIdx.x; r < hi; r += kWinThreads) {
      const double2* hp = reinterpret_cast<const double2*>(W.HB + kRowH * (size_t)W.e_lm[r]);
      double w[18], h[12], Di[9], d3[3];
#pragma unroll
      for (int j = 0; j < 6; j++) { const double2 v = hp[j]; h[2 * j] = v.x; h[2 * j + 1] = v.y; }
#pragma unroll
      for (int j = 0; j < 18; j++) w[j] = W.Ws[j * Fp + r];
      w_dinv(h, lambda, Di, d3);
#pragma unroll
      for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int b2 = 0; b2 < 3; b2++) W.Ts[(3 * a + b2) * Fp + r] = w[3 * a] * Di[b2] + w[3 * a + 1] * Di[3 + b2] + w[3 * a + 2] * Di[6 + b2];
        W.Ts[(18 + a) * Fp + r] = w[3 * a] * d3[0] + w[3 * a + 1] * d3[1] + w[3 * a + 2] * d3[2];
      }
    }
  }
}
// the reduced right-hand side and the blocks of the reduced system, each formed completely by ONE wave of the cluster
// (inlined by force: with two instantiations of the kernel calling it the inliner would otherwise leave it a function, and a call costs the
//  kernel the full register file and a stack)
__device__ __forceinline__ void cl_schur(const ClusterWin& W, const ClusterCtx& C, double* wred, double lambda) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t Fp = (size_t)W.Fp;
  double* wbuf = wred + wave * 4 * 36;
  // Which wave forms what is the host's schedule (build_window_fast: longest task first onto the least loaded of the cluster's 8 G waves): a
  // diagonal block has ~8 rounds of 64 pairs, an off-diagonal one 1-2, and dealt round-robin the waves' loads differed by a factor of two.
  // Every right-hand side and every block is still formed completely by ONE wave, in its own pair order: the same bits whatever the schedule.
  const int gw = C.g * (kWinThreads / 64) + wave;
  for (int idx = W.sched_start[gw]; idx < W.sched_start[gw + 1]; idx++) {
    const int task = W.sched_task[idx];
    if (task >= W.nfree) continue;
    const int i = task;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    const int q1 = W.cam_start[i + 1];
    for (int q = W.cam_start[i] + lane; q < q1; q += 64) {
#pragma unroll
      for (int a = 0; a < 6; a++) acc[a] += W.Ts[(18 + a) * Fp + q];
    }
    const double tot = w_wave_reduce<6>(acc, wbuf);
    if (lane < 6) W.rhsg[6 * i + lane] = W.bp[6 * (size_t)i + lane] - tot;
  }
  for (int idx = W.sched_start[gw]; idx < W.sched_start[gw + 1]; idx++) {
    const int bk = W.sched_task[idx] - W.nfree;
    if (bk < 0) continue;
    double acc[36];
#pragma unroll
    for (int t = 0; t < 36; t++) acc[t] = 0.0;
    const int q1 = W.bp_start[bk + 1];
    for (int q = W.bp_start[bk] + lane; q < q1; q += 64) {
      const int2 pr = W.bp_pairs[q];
      double t1[18], w2[18];
      // (gathered out of the column-major arrays, 36 eight-byte loads per pair.  Row-major copies of W Dinv and W -- a pair's operands in three
      //  cache lines each instead of eighteen -- were measured: the pass went from 54 to 70 us, the pass that writes the rows from 19 to 31)
#pragma unroll
      for (int j = 0; j < 18; j++) { t1[j] = W.Ts[j * Fp + pr.x]; w2[j] = W.Ws[j * Fp + pr.y]; }
#pragma unroll
      for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b2 = 0; b2 < 6; b2++) acc[6 * a + b2] += t1[3 * a] * w2[3 * b2] + t1[3 * a + 1] * w2[3 * b2 + 1] + t1[3 * a + 2] * w2[3 * b2 + 2];
    }
    const double tot = w_wave_reduce<36>(acc, wbuf);
    const int ij = W.blk_ij[bk], i1 = ij & 255, i2 = (ij >> 8) & 255;
    if (lane < 36) {
      const int a = lane / 6, b2 = lane - 6 * a;
      const double base = i1 == i2 ? W.Hpp[36 * (size_t)i1 + 6 * a + b2] + (a == b2 ? lambda : 0.0) : 0.0;
      W.Sblk[36 * (size_t)bk + lane] = base - tot;
    }
  }
}

// CAM: the camera of every window of the launch (a call's windows are grouped by model type on the host).  Only the three edge passes name it.
template <class CAM>
__global__ void __launch_bounds__(kWinThreads) k_ba_window_cluster(const ClusterWin* __restrict__ wins, const volatile int* __restrict__ stop, int K, int G) {
  extern __shared__ double lds[];
  constexpr int NT = kWinThreads;
  // K < 0: the placement test's map (tests/test_gpu_ba_window_fast.py) -- a window's workgroups are CONSECUTIVE blocks, i.e. spread over all
  // eight XCDs; the results must not depend on it (they do not: the barriers release and acquire at agent scope)
  const bool scatter = K < 0;
  if (scatter) K = -K;
  const int bid = blockIdx.x, slot = bid >> 3;
  const int wi = scatter ? bid / G : (slot / G) * 8 + (bid & 7);
  if (wi >= K) return;
  const ClusterWin& W = wins[wi];
  ClusterCtx C{scatter ? bid % G : slot % G, G, 0u, false};
  const bool leader = C.g == 0;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int n = 6 * W.nfree, nl = 3 * W.nact;
  double* S = lds;                                  // (workgroup 0 of the cluster only) packed lower triangle, n (n + 1) / 2
  double* rhs = S + (size_t)n * (n + 1) / 2;
  double* diag = rhs + n;
  double* ctl = diag + n;                           // [64]
  double* red = ctl + 64;                           // [256] partial sums of the tree reductions
  double* wred = ctl + 64 + 256;                    // the waves' reduction buffers
  int* const s_flag_p = reinterpret_cast<int*>(ctl + 60);   // the barrier's verdict (no static LDS beside the 160 KB dynamic block)
#define s_flag (*s_flag_p)
  dvm_ba_stats* const st = W.stats;
  // DVM_BA_WINDOW_PROF: shader-clock cycles per phase of the cluster's workgroup 0 (slot 10: waiting in the barriers), by its thread 0
  unsigned long long tprev = (W.prof && leader && tid == 0) ? __builtin_amdgcn_s_memtime() : 0ull;
  auto lap = [&](int slot) { if (W.prof && leader && tid == 0) { const unsigned long long t = __builtin_amdgcn_s_memtime(); W.prof[slot] += t - tprev; tprev = t; } };
#define CL_BARRIER() do { lap(ph); if (!cluster_barrier(W, C, &s_flag)) return; lap(10); } while (0)
  int ph = 11;
  if (leader && tid == 0) {
    win_stats_zero(st);
    W.cl_ctl[1] = (stop && *stop) ? 1.0 : 0.0;
  }
  for (int p = C.g; p < kParts; p += G) {
    int lo, hi;
    part_range(n + nl, p, lo, hi);
    for (int i = lo + tid; i < hi; i += NT) W.x[i] = 0.0;
    part_range(7 * W.P, p, lo, hi);
    for (int i = lo + tid; i < hi; i += NT) W.poses_t[i] = W.poses[i];
    part_range(3 * W.L, p, lo, hi);
    for (int i = lo + tid; i < hi; i += NT) W.pts_t[i] = W.pts[i];
  }
  double* poses = W.poses; double* poses_t = W.poses_t; double* pts = W.pts; double* pts_t = W.pts_t;
  CL_BARRIER();

  double lambda = -1, ni = 2, currentChi = 0, chi_last = 0;
  int nBad = 0, it_done = 0, trials_total = 0, stop_reason = 0;
  bool stopped = W.cl_ctl[1] != 0.0;
  for (int it = 0; it < W.iterations && !stopped; it++) {
    ph = 0;
    // (Evaluating a trial WITH its Jacobians into a second set of rows, so that an accepted trial hands the next iteration its linearisation --
    //  as the tile solver's loop and k_pose_optimize do -- was measured: 2.92 -> 3.27 ms for 32 windows.  The pass it saves is 15 us, but
    //  two sets of rows are 260 MB for 32 windows and no longer stay in the 256 MB memory-side cache: the accumulation behind it went from
    //  27 to 48 us, the W Dinv pass from 18 to 25.)
    cl_edge_pass<true, CAM>(W, C, poses, pts);
    if (it == 0) cluster_partial_sums(W, C, W.e_rho, W.E, 0, red);
    CL_BARRIER();
    ph = 1;
    {
      double mx = cl_accumulate(W, C, wred);
      if (it == 0) {      // computeLambdaInit's max |diagonal|: this workgroup's share -> its parts' slots (a maximum has no order)
        for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
        __syncthreads();
        if ((tid & 63) == 0) red[wave] = mx;
        __syncthreads();
        if (tid == 0) {
          double m = red[0];
          for (int w2 = 1; w2 < NT / 64; w2++) m = fmax(m, red[w2]);
          for (int p = 0; p < kParts; p++) if (p % G == C.g) W.cl_part[2 * kParts + p] = m;
        }
      }
    }
    CL_BARRIER();
    if (it == 0) {
      currentChi = cluster_total(W, 0);
      if (leader && tid == 0) st->chi2_initial = currentChi;
      double mx = 0;
      for (int p = 0; p < kParts; p++) mx = fmax(mx, W.cl_part[2 * kParts + p]);
      lambda = 1e-5 * mx;
      ni = 2; nBad = 0;
    }
    const double iniChi = currentChi;
    double tempChi = currentChi, rho = 0;
    int qmax = 0;
    do {
      ph = 2;
      cl_t_rows(W, C, lambda);
      CL_BARRIER();
      ph = 3;
      cl_schur(W, C, wred, lambda);
      CL_BARRIER();
      ph = 6;
      if (leader) {
        for (int i = tid; i < n * (n + 1) / 2; i += NT) S[i] = 0.0;
        __syncthreads();
        for (int t = tid; t < 36 * W.nblk; t += NT) {
          const int bk = t / 36, e = t - 36 * bk, a = e / 6, b2 = e - 6 * a;
          const int ij = W.blk_ij[bk], i1 = ij & 255, i2 = (ij >> 8) & 255;
          if (i1 != i2 || b2 <= a) S[tri(6 * i1 + a, 6 * i2 + b2)] = W.Sblk[t];
        }
        for (int t = tid; t < n; t += NT) rhs[t] = W.rhsg[t];
        __syncthreads();
        lap(4);
        // (rhs IS row n of the packed triangle; diag: 1 / L_kk; Lp: the reduction buffers are idle during the solve)
        const bool ok = win_cholesky_rhs(S, diag, ctl + 64, n, reinterpret_cast<int*>(ctl + 61), W.prof);
        lap(5);
        if (ok) {
          if (wave == 0) win_backsubstitute(S, diag, ctl + 64, rhs, n);
          __syncthreads();
          for (int i = tid; i < n; i += NT) W.x[i] = rhs[i];
        }
        if (tid == 0) { W.cl_ctl[0] = ok ? 1.0 : 0.0; W.cl_ctl[1] = (stop && *stop) ? 1.0 : 0.0; }
      }
      CL_BARRIER();
      ph = 7;
      const bool ok = W.cl_ctl[0] != 0.0;
      const size_t Fp = (size_t)W.Fp;
      if (ok) {      // W^T x_p of this workgroup's rows
        for (int p = C.g; p < kParts; p += G) {
          int lo, hi;
          part_range(W.F, p, lo, hi);
          for (int r = lo + tid; r < hi; r += NT) {
            const double* xp = W.x + 6 * W.f_cam[r];
            double c0 = 0, c1 = 0, c2 = 0;
#pragma unroll
            for (int a = 0; a < 6; a++) {
              const double xa = xp[a];
              c0 += W.Ws[(3 * a) * Fp + r] * xa; c1 += W.Ws[(3 * a + 1) * Fp + r] * xa; c2 += W.Ws[(3 * a + 2) * Fp + r] * xa;
            }
            W.Cs[r] = c0; W.Cs[Fp + r] = c1; W.Cs[2 * Fp + r] = c2;
          }
        }
      }
      CL_BARRIER();
      ph = 8;
      // landmarks of this workgroup: xl = Dinv (bl - sum of their rows' W^T x_p), the trial point, the scale terms; its cameras: oplus
      for (int p = C.g; p < kParts; p += G) {
        int lo, hi;
        part_range(W.nact, p, lo, hi);
        for (int li = lo + tid; li < hi; li += NT) {
          const double* hb = W.HB + kRowH * (size_t)li;
          double xl[3];
          if (ok) {
            double h[12], Di[9], d3[3];
#pragma unroll
            for (int j = 0; j < 12; j++) h[j] = hb[j];
            w_dinv(h, lambda, Di, d3);
            double c0 = h[9], c1 = h[10], c2 = h[11];
            // (the rows' W^T x_p come from the phase above: formed here, by the landmark's thread -- one phase and one barrier less -- the
            //  scattered W loads made this phase 46-54 us instead of 18 + 18)
            for (int q = W.pt_start[li]; q < W.pt_start[li + 1]; q++) {
              const int r = W.pt_edges[q];
              if (r >= W.F) break;
              c0 -= W.Cs[r]; c1 -= W.Cs[Fp + r]; c2 -= W.Cs[2 * Fp + r];
            }
            const double c[3] = {c0, c1, c2};
            mat3_vec(Di, c, xl);
#pragma unroll
            for (int a = 0; a < 3; a++) W.x[n + 3 * (size_t)li + a] = xl[a];
          } else {
#pragma unroll
            for (int a = 0; a < 3; a++) xl[a] = W.x[n + 3 * (size_t)li + a];     // (a failed solve: the last successful one's x)
          }
          const int l = W.act_pt[li];
#pragma unroll
          for (int a = 0; a < 3; a++) {
            pts_t[3 * (size_t)l + a] = pts[3 * (size_t)l + a] + xl[a];
            W.terms[n + 3 * li + a] = xl[a] * (lambda * xl[a] + hb[9 + a]);
          }
        }
        part_range(W.nfree, p, lo, hi);
        for (int i = lo + tid; i < hi; i += NT) {
          const int pp = W.free_pose[i];
          se3_oplus(poses + 7 * (size_t)pp, W.x + 6 * (size_t)i, poses_t + 7 * (size_t)pp);
#pragma unroll
          for (int a = 0; a < 6; a++) { const double xj = W.x[6 * i + a]; W.terms[6 * i + a] = xj * (lambda * xj + W.bp[6 * i + a]); }
        }
      }
      CL_BARRIER();
      ph = 9;
      cl_edge_pass<false, CAM>(W, C, poses_t, pts_t);
      cluster_partial_sums(W, C, W.e_rho, W.E, 0, red);
      cluster_partial_sums(W, C, W.terms, n + nl, 1, red);
      CL_BARRIER();
      ph = 11;
      // ---- the decision, taken by every thread of every workgroup on the same words (optimization_algorithm_levenberg.cpp:113-147)
      tempChi = ok ? cluster_total(W, 0) : 1.7976931348623157e308;
      rho = currentChi - tempChi;
      const double scale = cluster_total(W, 1) + 1e-3;
      rho /= scale;
      if (rho > 0 && isfinite(tempChi)) {
        double alpha = 1. - f64_cube(2 * rho - 1);
        alpha = (2. / 3. < alpha) ? 2. / 3. : alpha;
        lambda *= (1. / 3. < alpha) ? alpha : 1. / 3.;
        ni = 2;
        currentChi = tempChi;
        double* sw = poses; poses = poses_t; poses_t = sw;
        sw = pts; pts = pts_t; pts_t = sw;
      } else {
        lambda *= ni;
        ni *= 2;
      }
      qmax++;
      trials_total++;
      stopped = W.cl_ctl[1] != 0.0;
    } while (rho < 0 && qmax < 10 && !stopped);
    it_done++;
    chi_last = currentChi;
    if (leader && tid == 0 && it < 64) { st->trials_per_iter[it] = qmax; st->chi2_per_iter[it] = currentChi; st->lambda_per_iter[it] = lambda; }
    if (qmax == 10 || rho == 0) { stop_reason = 1; break; }
    if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
    if (nBad >= 3) { stop_reason = 2; break; }
  }
  if (it_done == 0) {     // no iteration ran: the edges are evaluated at the unchanged input state (see k_ba_window, ba_window_seq.hip)
    cl_edge_pass<false, CAM>(W, C, poses, pts);
    cluster_partial_sums(W, C, W.e_rho, W.E, 0, red);
    CL_BARRIER();
    chi_last = cluster_total(W, 0);
    if (leader && tid == 0) st->chi2_initial = chi_last;
  }
  // results: the accepted state, chi2 / depth signs back in the caller's edge order (every workgroup its parts; all inputs are final:
  // the last barrier is behind every write of the state and of chi_s)
  for (int p = C.g; p < kParts; p += G) {
    int lo, hi;
    part_range(7 * W.P, p, lo, hi);
    for (int i = lo + tid; i < hi; i += NT) W.out_poses[i] = poses[i];
    part_range(3 * W.L, p, lo, hi);
    for (int i = lo + tid; i < hi; i += NT) W.out_pts[i] = pts[i];
    part_range(W.E, p, lo, hi);
    for (int k = lo + tid; k < hi; k += NT) {
      const double* T = poses + 7 * (size_t)W.e_pose[k];
      const double* X = pts + 3 * (size_t)W.e_point[k];
      double R[9], Xc[3];
      quat_to_R(T + 3, R);
      mat3_vec(R, X, Xc);
      const int ko = W.e_orig[k];
      W.e_depth[ko] = (Xc[2] + T[2]) > 0.0 ? 1 : 0;
      W.e_chi2[ko] = W.chi_s[k];
    }
  }
  if (leader && tid == 0) {
    st->iterations = it_done; st->total_trials = trials_total; st->chi2_final = chi_last; st->lambda_final = lambda; st->stop_reason = stop_reason;
  }
  lap(11);
#undef CL_BARRIER
#undef s_flag
}

}  // namespace dvm

using namespace dvm;

namespace {

// a window's tables (build_window_fast), packed into page-locked memory by the builder's own thread while they are in its caches: a span
// of the call's shared block, or the window's own arena where that is full -- sent to the device from where they lie
struct ClusterBuild : ClusterTables {
  PinnedArena arena;
  struct ArenaOff { ptrdiff_t poses, free_pose, act_pt, e_pose, e_point, e_obs, e_info, pt_start, f_cam, blk_ij, e_orig, e_lm, cam_start, pt_edges, bp_start, bp_pairs, sched_start, sched_task; } ao;
  ptrdiff_t shared_off = -1;          // >= 0: the tables lie at this offset of the call's shared block, not in `arena`
  size_t packed_bytes = 0;
  int pack_fast(PinnedArena* shared) {
    auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    auto b4 = [&](const std::vector<int32_t>& v) { return pad(v.size() * 4); };
    auto b8 = [&](const std::vector<double>& v) { return pad(v.size() * 8); };
    const size_t total = b8(g.poses) + b4(g.free_pose) + b4(g.act_pt) + b4(g.e_pose) + b4(g.e_point) + b8(g.e_obs) + b8(g.e_info) + b4(pt_start) + b4(f_cam) +
                         b4(blk_ij) + b4(e_orig) + b4(e_lm) + b4(cam_start) + b4(pt_edges) + b4(bp_start) + b4(bp_pairs) + b4(sched_start) + b4(sched_task);
    shared_off = shared ? shared->claim(total) : -1;
    if (shared_off < 0) { const int rc = arena.reserve(total); if (rc != DVM_OK) return rc; }
    else arena.used = 0;
    // (a span of the shared block is filled through a view of it: base at the span, the same bump logic)
    uint8_t* const base = shared_off >= 0 ? shared->base + shared_off : arena.base;
    size_t used = 0;
    auto put = [&](const void* src, size_t bytes) -> ptrdiff_t {
      if (!bytes) return -1;
      const size_t off = used;
      std::memcpy(base + off, src, bytes);
      used = off + pad(bytes);
      return (ptrdiff_t)off;
    };
    auto p4 = [&](const std::vector<int32_t>& v) { return put(v.data(), v.size() * 4); };
    auto p8 = [&](const std::vector<double>& v) { return put(v.data(), v.size() * 8); };
    ao.poses = p8(g.poses); ao.free_pose = p4(g.free_pose); ao.act_pt = p4(g.act_pt); ao.e_pose = p4(g.e_pose); ao.e_point = p4(g.e_point);
    ao.e_obs = p8(g.e_obs); ao.e_info = p8(g.e_info); ao.pt_start = p4(pt_start); ao.f_cam = p4(f_cam); ao.blk_ij = p4(blk_ij); ao.e_orig = p4(e_orig); ao.e_lm = p4(e_lm);
    ao.cam_start = p4(cam_start); ao.pt_edges = p4(pt_edges); ao.bp_start = p4(bp_start); ao.bp_pairs = p4(bp_pairs);
    ao.sched_start = p4(sched_start); ao.sched_task = p4(sched_task);
    if (shared_off < 0) arena.used = used;
    packed_bytes = used;
    return DVM_OK;
  }
};

// The tables of ALL windows of a call travel to one device block, every window's span the moment its builder has packed it (from the
// builder's thread, on one of four upload streams: the copies of the first windows run under the builds of the last, and side by side -- one
// 32 MB copy behind the builds took 1.4 ms, 23 GB/s); the launch's stream waits for the four streams' events
struct TableUpload {
  hipStream_t s[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  uint8_t* dev = nullptr; size_t dcap = 0; int device = -1;
  void release() {
    for (int i = 0; i < 4; i++) { if (s[i]) { hipStreamSynchronize(s[i]); hipStreamDestroy(s[i]); } if (e[i]) hipEventDestroy(e[i]); s[i] = nullptr; e[i] = nullptr; }
    if (dev) hipFree(dev);
    dev = nullptr; dcap = 0;
  }
  int ensure(int dev_id, size_t bytes) {
    if (dev_id != device) { release(); device = dev_id; }
    for (int i = 0; i < 4; i++) {
      if (!s[i]) { int rc = hip_check(hipStreamCreateWithFlags(&s[i], hipStreamNonBlocking), "stream"); if (rc != DVM_OK) return rc; }
      if (!e[i]) { int rc = hip_check(hipEventCreateWithFlags(&e[i], hipEventDisableTiming), "event"); if (rc != DVM_OK) return rc; }
    }
    if (bytes > dcap) {
      if (dev) hipFree(dev);
      dev = nullptr; dcap = 0;
      int rc = hip_check(hipMalloc(reinterpret_cast<void**>(&dev), bytes), "hipMalloc(window tables)");
      if (rc != DVM_OK) return rc;
      dcap = bytes;
    }
    return DVM_OK;
  }
  ~TableUpload() { release(); }
};

}  // namespace

// The cluster size: the largest of 8 / 4 / 2 / 1 workgroups per window whose grid (`groups` * G workgroups, one per CU: the reduced system's
// LDS) is resident at once; `forced` (the G = 1 repeat after a barrier time-out, the two launches of DVM_BA_SPLIT) or DVM_BA_CLUSTER decide otherwise.
int ba_cluster_size(int device, int groups, int forced) {
  int cus = 0;
  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  const char* env_c = std::getenv("DVM_BA_CLUSTER");      // (read at every call: the tests walk the cluster sizes)
  const int want = forced > 0 ? forced : env_c ? atoi(env_c) : 0;
  for (int g = 8; g >= 1; g >>= 1) if ((want > 0 && g == want) || (want <= 0 && groups * g <= cus)) return g;
  return 1;
}

// models NULL: pinhole windows; else the camera model of every window.  Model 0: the window's cam.fx, fy, cx, cy, as without models; model 1
// (KannalaBrandt8): models[k].p, and cam.huber_delta.  The windows are grouped by model type and each type present runs as ONE launch of its
// instantiation of k_ba_window_cluster, one after the other on the calling thread's staging stream, G chosen per launch from its own window
// count: a homogeneous call is one launch, a mixed one two.  A window's result depends neither on its batch nor on G, hence not on the other
// model types of the call either.
// res (dvm_ba_resident_optimize): the windows' edges and points are not the caller's arrays (edges and points of `windows` are NULL) but
// lie in resident stores -- a gather kernel in front of the solver fills e_obs / e_info / pts, the prepare kernels run behind it
// (ba_window_resident.hip); tables, views and launch are the same.
int ba_windows_cluster(int device, const dvm_ba_window* windows, int K, const volatile uint8_t* stop_flag, dvm_ba_stats* stats, int cluster, const dvm_camera_model* models,
                       const ResidentCall* res) {
  if (K < 0 || (K && !windows)) { set_error("dvm_ba_optimize_windows: null windows"); return DVM_ERR_INVALID; }
  if (K == 0) return DVM_OK;
  int n_kb8 = 0;
  for (int k = 0; models && k < K; k++) n_kb8 += models[k].model == dvm_cam::kKannalaBrandt8 ? 1 : 0;
  const bool kb8 = n_kb8 == K;
  int rc = DVM_OK;
  if (n_kb8 > 0 && n_kb8 < K) {
    for (int k = 0; k < K; k++) if ((rc = win_graph(windows[k], true, nullptr, res ? resident_obs(*res->win[k].w) : nullptr)) != DVM_OK) return rc;     // ALL windows are checked before the first launch
    for (int type = 0; type < 2; type++) {
      std::vector<int> idx;
      std::vector<dvm_ba_window> gw;
      std::vector<dvm_camera_model> gm;
      std::vector<WinResident> gr;
      for (int k = 0; k < K; k++) if ((models[k].model == dvm_cam::kKannalaBrandt8 ? 1 : 0) == type) { idx.push_back(k); gw.push_back(windows[k]); gm.push_back(models[k]); if (res) gr.push_back(res->win[k]); }
      std::vector<dvm_ba_stats> gs(idx.size());
      ResidentCall gres;
      if (res) { gres = *res; gres.win = gr.data(); }
      if ((rc = ba_windows_cluster(device, gw.data(), (int)idx.size(), stop_flag, stats ? gs.data() : nullptr, cluster, gm.data(), res ? &gres : nullptr)) != DVM_OK) return rc;
      for (size_t j = 0; stats && j < idx.size(); j++) stats[idx[j]] = gs[j];
    }
    return DVM_OK;
  }
  rc = dvm_set_device(device);
  if (rc != DVM_OK) return rc;
  WinCall call(windows, K, stop_flag);
  // chosen before the builds: the windows' Schur schedules are per wave of the cluster
  const int groups = 8 * ((K + 7) / 8);
  const int G = ba_cluster_size(device, groups, cluster);
  // the windows' host tables live in a per-thread pool (see ClusterTables' scratch members)
  static thread_local std::vector<ClusterBuild> build_pool;
  if ((int)build_pool.size() < K) build_pool.resize(K);
  std::vector<ClusterBuild>& B = build_pool;
  for (int k = 0; k < K; k++) B[k].cluster_waves = (kWinThreads / 64) * G;
  // the tables of ALL windows go into one page-locked block (one DMA): sized before the builds from a generous estimate -- ~66 bytes per
  // edge are typical --; a window that finds it full packs into a block of its own
  static thread_local PinnedArena shared_tables_tls;
  static thread_local TableUpload tup_tls;
  // (the builders' threads must see THIS thread's block and streams: a thread_local named inside their lambda would be their own)
  PinnedArena& shared_tables = shared_tables_tls;
  TableUpload& tup = tup_tls;
  size_t est = 0;
  for (int k = 0; k < K; k++) est += 80 * (size_t)std::max(windows[k].n_poses, 0) + 16 * (size_t)std::max(windows[k].n_points, 0) + 96 * (size_t)std::max(windows[k].n_edges, 0) + (64 << 10);
  if ((rc = shared_tables.reserve(est)) != DVM_OK) return rc;
  if ((rc = tup.ensure(device, shared_tables.cap)) != DVM_OK) return rc;
  const bool private_tables = std::getenv("DVM_BA_TEST_PRIVATE_TABLES") != nullptr;   // (test hook: every second window packs into a block of its own, as one that finds the shared block full does)
  auto send_tables = [&](int k) -> int {        // window k's span of the shared block -> the device block, asynchronously
    const ClusterBuild& b = B[k];
    if (b.shared_off < 0 || !b.packed_bytes) return (int)DVM_OK;
    return hip_check(hipMemcpyAsync(tup.dev + b.shared_off, shared_tables.base + b.shared_off, b.packed_bytes, hipMemcpyHostToDevice, tup.s[k & 3]), "upload(window tables)");
  };
  if (K > 1) {
    // the windows' index tables are independent: built by up to 32 pooled host threads (0.2 ms each; 32 of them one after the other would cost
    // more than the launch that solves them)
    std::vector<int> rcs(K, DVM_OK);
    std::vector<std::string> errs(K);
    static const int bt = std::getenv("DVM_BA_BUILD_THREADS") ? std::max(1, atoi(std::getenv("DVM_BA_BUILD_THREADS"))) : 32;
    HostPool::get().run((size_t)K, bt, [&](size_t k) {
      rcs[k] = build_window_fast(windows[k], B[k], res ? resident_obs(*res->win[k].w) : nullptr);
      if (rcs[k] == DVM_OK) { hipSetDevice(device); rcs[k] = B[k].pack_fast((private_tables && (k & 1)) ? nullptr : &shared_tables); }
      if (rcs[k] == DVM_OK) rcs[k] = send_tables((int)k);     // (a pooled thread: the device of the call, for the arena's first allocation)
      if (rcs[k] != DVM_OK) errs[k] = last_error_cstr();
    });
    for (int k = 0; k < K; k++) if (rcs[k] != DVM_OK) { set_error(errs[k]); return rcs[k]; }
  } else {
    if ((rc = build_window_fast(windows[0], B[0], res ? resident_obs(*res->win[0].w) : nullptr)) != DVM_OK || (rc = B[0].pack_fast(&shared_tables)) != DVM_OK || (rc = send_tables(0)) != DVM_OK) return rc;
  }
  call.mark(1);
  if (std::getenv("DVM_BA_WINDOW_TIMING")) {     // (measurement only: how long the tables' copies run on behind the builds)
    for (int i = 0; i < 4; i++) hipStreamSynchronize(tup.s[i]);
    std::fprintf(stderr, "tables: %.1f MB, copies done %.2f ms behind the builds\n", shared_tables.top() / 1048576.0, std::chrono::duration<double, std::milli>(WinCall::clock::now() - call.t[1]).count());
  }
  int* stop_dev = nullptr;
  if ((rc = call.arm(&stop_dev)) != DVM_OK) return rc;

  Stage st;
  struct Slots { int pts, arena, cl_sync, poses_t, pts_t, rowA, erho, Hpp, bp, HB, x, terms, Bs, Ws, Ts, Cs, chi_s, Sblk, rhsg, cl_part, cl_ctl; };
  std::vector<Slots> sl(K);
  for (int i = 0; i < 4; i++) DVM_HIP(hipEventRecord(tup.e[i], tup.s[i]));
  for (int k = 0; k < K; k++) {     // inputs: the window's tables are already page-locked (pack_fast); the landmarks from the caller's array
    const ClusterBuild& b = B[k]; Slots& s = sl[k];
    s.arena = b.shared_off < 0 ? st.in_pinned(b.arena.used ? b.arena.base : nullptr, b.arena.used) : -1;
    s.pts = res ? -1 : st.in(b.g.L ? windows[k].points : nullptr, 24 * (size_t)b.g.L);
  }
  ResidentStage rstage(res ? *res : ResidentCall{}, res ? K : 0);     // (without res: nothing added, nothing launched)
  if (res) rstage.add_inputs(st);
  std::vector<uint32_t> sync_zero(16, 0u);        // a window's arrival counter [0] and time-out word [8], zero at every launch
  std::vector<std::vector<uint32_t>> sync_back(K, std::vector<uint32_t>(16, 0u));
  for (int k = 0; k < K; k++) sl[k].cl_sync = st.add(sync_zero.data(), sync_back[k].data(), 64);
  std::vector<ClusterWin> views(K);
  const int views_slot = st.in(views.data(), sizeof(ClusterWin) * (size_t)K);   // filled in below, once layout() has placed everything
  call.add_outputs(st);
  if (res) { rstage.add_outputs(st); rstage.add_scratch(st); }
  for (int k = 0; k < K; k++) {                     // working memory
    const ClusterBuild& b = B[k]; Slots& s = sl[k];
    const size_t E = b.g.E, Fp = (size_t)b.Fp, n = 6 * (size_t)b.g.nfree, nl = 3 * (size_t)b.g.nact;
    s.poses_t = st.scratch(56 * (size_t)b.g.P); s.pts_t = st.scratch(24 * (size_t)b.g.L);
    s.rowA = st.scratch(8 * kRowA * E); s.erho = st.scratch(8 * E);
    s.Hpp = st.scratch(288 * (size_t)b.g.nfree); s.bp = st.scratch(8 * n); s.HB = st.scratch(8 * kRowH * (size_t)b.g.nact);
    s.x = st.scratch(8 * (n + nl)); s.terms = st.scratch(8 * (n + nl));
    s.Bs = st.scratch(8 * 15 * Fp); s.Ws = st.scratch(8 * 18 * Fp); s.Ts = st.scratch(8 * 24 * Fp); s.Cs = st.scratch(8 * 3 * Fp); s.chi_s = st.scratch(8 * E);
    s.Sblk = st.scratch(8 * 36 * (size_t)std::max(b.nblk, 1)); s.rhsg = st.scratch(8 * std::max<size_t>(n, 1)); s.cl_part = st.scratch(8 * 4 * 8); s.cl_ctl = st.scratch(8 * 4);
  }
  call.mark(2);
  if ((rc = st.layout()) != DVM_OK) return rc;
  call.mark(3);
  size_t lds_doubles = 0;
  for (int k = 0; k < K; k++) {
    const ClusterBuild& b = B[k]; const WinGraph& g = b.g; const Slots& s = sl[k]; ClusterWin& v = views[k];
    std::memset(&v, 0, sizeof(v));
    v.P = g.P; v.L = g.L; v.E = g.E; v.F = b.F; v.nfree = g.nfree; v.nact = g.nact; v.nblk = b.nblk; v.iterations = windows[k].iterations;
    v.Fp = b.Fp;
    v.fx = windows[k].cam.fx; v.fy = windows[k].cam.fy; v.cx = windows[k].cam.cx; v.cy = windows[k].cam.cy; v.delta = windows[k].cam.huber_delta;
    if (kb8) std::memcpy(v.kb8, models[k].p, sizeof(v.kb8));
    uint8_t* const ab = b.shared_off >= 0 ? tup.dev + b.shared_off : st.ptr<uint8_t>(s.arena);   // the window's tables on the device
    auto A4 = [&](ptrdiff_t off) { return off < 0 ? nullptr : reinterpret_cast<int32_t*>(ab + off); };
    auto A8 = [&](ptrdiff_t off) { return off < 0 ? nullptr : reinterpret_cast<double*>(ab + off); };
    v.poses = A8(b.ao.poses); v.free_pose = A4(b.ao.free_pose); v.act_pt = A4(b.ao.act_pt);
    v.e_pose = A4(b.ao.e_pose); v.e_point = A4(b.ao.e_point); v.e_obs = A8(b.ao.e_obs); v.e_info = A8(b.ao.e_info);
    v.pt_start = A4(b.ao.pt_start); v.f_cam = A4(b.ao.f_cam); v.blk_ij = A4(b.ao.blk_ij);
    v.e_orig = A4(b.ao.e_orig); v.e_lm = A4(b.ao.e_lm); v.cam_start = A4(b.ao.cam_start); v.pt_edges = A4(b.ao.pt_edges);
    v.bp_start = A4(b.ao.bp_start); v.bp_pairs = reinterpret_cast<const int2*>(A4(b.ao.bp_pairs));
    v.sched_start = A4(b.ao.sched_start); v.sched_task = A4(b.ao.sched_task);
    if (res) { v.e_obs = rstage.e_obs(st, k); v.e_info = rstage.e_info(st, k); }
    v.pts = res ? rstage.pts(st, k) : st.ptr<double>(s.pts); v.poses_t = st.ptr<double>(s.poses_t); v.pts_t = st.ptr<double>(s.pts_t);
    v.rowA = st.ptr<double>(s.rowA); v.e_rho = st.ptr<double>(s.erho);
    v.Bs = st.ptr<double>(s.Bs); v.Ws = st.ptr<double>(s.Ws); v.Ts = st.ptr<double>(s.Ts); v.Cs = st.ptr<double>(s.Cs); v.chi_s = st.ptr<double>(s.chi_s);
    v.cl_ctr = st.ptr<unsigned int>(s.cl_sync); v.cl_tmo = v.cl_ctr + 8;
    v.Sblk = st.ptr<double>(s.Sblk); v.rhsg = st.ptr<double>(s.rhsg); v.cl_part = st.ptr<double>(s.cl_part); v.cl_ctl = st.ptr<double>(s.cl_ctl);
    v.Hpp = st.ptr<double>(s.Hpp); v.bp = st.ptr<double>(s.bp); v.HB = st.ptr<double>(s.HB);
    v.x = st.ptr<double>(s.x); v.terms = st.ptr<double>(s.terms);
    call.fill(st, k, v);
    if (res) rstage.fill(st, k, v.e_orig, v.out_poses, v.out_pts, v.e_chi2, v.e_depth);
    const size_t n = 6 * (size_t)g.nfree;
    lds_doubles = std::max(lds_doubles, n * (n + 1) / 2 + 2 * n + 64 + 256 + (size_t)b.stage_doubles);
  }
  call.mark(4);
  if ((rc = st.upload()) != DVM_OK) return rc;
  for (int i = 0; i < 4; i++) DVM_HIP(hipStreamWaitEvent(st.stream(), tup.e[i], 0));     // the tables have arrived before the launch starts
  if (res) {
    if ((rc = rstage.gather(st)) != DVM_OK) return rc;
    int64_t up = (int64_t)st.in_bytes;
    for (int k = 0; k < K; k++) up += (int64_t)(B[k].shared_off >= 0 ? B[k].packed_bytes : B[k].arena.used);
    *res->h2d += up;
  }
  call.mark(5);
  // dynamic LDS: the packed reduced system of the largest window, rhs / diagonal, control words and the reduction buffers
  const size_t lds_bytes = sizeof(double) * lds_doubles;
  if (lds_bytes > 160 * 1024) { set_error("dvm_ba_optimize_windows: a window needs more than 160 KB of LDS"); return DVM_ERR_CAPACITY; }
  // on the staging stream of the calling thread (upload -> kernel -> download is one in-order chain there; the legacy NULL stream would
  // also order this launch against every other thread's staging stream: dvm_ba_optimize_batch's workers serialised on it)
  struct KernelEvents { hipEvent_t a = nullptr, b = nullptr; ~KernelEvents() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); } };
  thread_local KernelEvents kev;     // the launch's duration -> dvm_ba_stats::kernel_us (the roofline figure in bench_legs.lba_fast)
  const auto kernel = kb8 ? k_ba_window_cluster<PoseCamKB8> : k_ba_window_cluster<PoseCamPinhole>;
  DVM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  if (!kev.a) { DVM_HIP(hipEventCreate(&kev.a)); DVM_HIP(hipEventCreate(&kev.b)); }
  hipEventRecord(kev.a, st.stream());
  const bool scatter = std::getenv("DVM_BA_CLUSTER_SCATTER") != nullptr;     // (placement test: see the kernel)
  hipLaunchKernelGGL(kernel, dim3(groups * G), dim3(kWinThreads), lds_bytes, st.stream(), st.ptr<ClusterWin>(views_slot), stop_dev, scatter ? -K : K, G);
  hipEventRecord(kev.b, st.stream());
  DVM_HIP(hipGetLastError());
  if (res) {
    if ((rc = rstage.prepare(st)) != DVM_OK) return rc;
    size_t lo = st.total, hi = 0;      // the span Stage::download fetches
    for (const Stage::Item& it : st.items) if (it.dst && it.bytes && !it.mapped) { lo = std::min(lo, it.off); hi = std::max(hi, it.off + it.bytes); }
    if (hi > lo) *res->d2h += (int64_t)(hi - lo);
  }
  if ((rc = call.wait(st, G)) != DVM_OK) return rc;
  if (G > 1) {
    bool timed_out = std::getenv("DVM_BA_TEST_TIMEOUT") != nullptr;      // (test hook: take the repeat path without a real time-out)
    for (int k = 0; k < K; k++) timed_out = timed_out || sync_back[k][8] != 0u;
    if (timed_out)     // a cluster's workgroups were not all resident (other work held compute units): solve the batch again, one workgroup per window
      return ba_windows_cluster(device, windows, K, stop_flag, stats, 1, models, res);
  }
  static const char* names[16] = {"edge pass + Jacobians", "Hll / bl, Hpp / bp", "W Dinv rows", "Schur blocks + rhs", "assemble S in LDS", "Cholesky", "substitution + x", "W^T x rows",
                                  "landmarks + oplus", "edge pass chi2 + sums", "IN BARRIERS (workgroup 0)", "decision + rest", "  chol: diagonal block", "  chol: panel", "  chol: barriers", "  chol: trailing update"};
  float kernel_ms = 0;
  const bool timed = hipEventElapsedTime(&kernel_ms, kev.a, kev.b) == hipSuccess;
  call.finish(stats, names, timed ? (int)(kernel_ms * 1e3f + 0.5f) : -1);
  return DVM_OK;
}
