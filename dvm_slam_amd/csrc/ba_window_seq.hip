// dvm_slam_amd/csrc/ba_window_seq.hip -- dvm_ba_optimize_windows: K independent bundle adjustments ("windows"), ONE launch, one workgroup per
// window, the whole optimizer.optimize(n) -- Levenberg-Marquardt iterations, trials, stopping rules -- on the device.
//
// What it is for.
//  (1) Several agents sharing one GPU (BASELINE.json config 4 with more agents than GPUs): their LocalBundleAdjustment windows
//      (Optimizer.cc:1030-1387) are independent problems; K of them fill K compute units side by side instead of queueing behind one
//      another on the 40-launches-per-trial tile solver (ba_solver.cpp), which is laid out for one large map.
//  (2) Tiny problems -- GlobalBundleAdjustemnt(map, 20) on the TWO keyframes of a monocular initialisation (Tracking.cc:2330), local
//      windows of 3..5 keyframes right after it.  One free camera with free points leaves the scale gauge to the damping alone; the
//      result of such a problem moves by 1e-3 .. 1e-1 when nothing but the ORDER of the floating-point sums changes (tools/
//      ba_sensitivity.py: the CPU oracle against itself with its edge list permuted).  "Within 1e-6 of the reference" is then only
//      meaningful for an implementation that adds in the reference's order -- so this kernel does:
//
// Every sum runs in the order g2o's single-threaded code runs it, and every rounding is one IEEE operation (-ffp-contract=off, IEEE
// division and square root, the libm calls replaced by csrc/f64_spec.h on both sides):
//   * chi2 = sum of rho(e) over the edges in edge order (SparseOptimizer::activeRobustChi2), by ONE wave, sequentially;
//   * Hpp / bp of a camera, Hll / bl of a landmark: contributions in edge order (BaseBinaryEdge::constructQuadraticForm called
//     edge by edge, block_solver.hpp:502-560) -- one lane per matrix entry walks the vertex's edges in order;
//   * Schur complement (block_solver.hpp:381-439): landmark by landmark, Hschur(i1, i2) -= W1 Dinv W2^T in landmark order -- one lane
//     per entry walks the block's (edge, edge) pairs in that order; bschur likewise;
//   * the reduced system: Cholesky by rows with ascending-k dot products (the oracle's envelope form; a right-looking elimination
//     applies the same subtractions to every entry in the same order, so it runs in parallel and gives the same bits), forward and
//     backward substitution likewise; LDS-resident (packed lower triangle: up to 30 free cameras = 130 KB of the CU's 160 KB);
//   * landmark back substitution, oplus (SE3Quat::exp, se3quat.h:212-240), computeScale (sequential), the gain ratio and the damping
//     update of optimization_algorithm_levenberg.cpp:107-147, the stopping rules of Optimizer / g2o (:154-162).
// tests/test_gpu_ba_window.py holds the result to the CPU oracle BIT FOR BIT (poses, points, per-edge chi2, LM trial sequence, lambda).
//
// The price is speed per window -- the sequential sums are one lane's dependent FP64 additions (8 cycles each) -- which K windows side
// by side buy back; one large window is the tile solver's job (dvm_ba_optimize), many windows per call the cluster form's
// (ba_window_cluster.hip: tree sums, a tolerance instead of the bits).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ba_kernels.h"
#include "ba_window_seq_tables.h"
#include "f64_spec.h"
#include "se3_f64.h"       // the small algebra, in the oracle's sequences

namespace dvm {

// device view of one window: pointers into the call's staging block.
// Per-edge rows live in the order their consumer walks them, so that a chunk of consecutive rows is one coalesced copy into LDS:
//   rowB [E][16]  edge order            B (2x6), w, wr0, wr1         -> Hpp / bp chains of the cameras (edge order)
//   rowA [E][12]  landmark-major (lpos) A (2x3), w, wr0, wr1         -> Hll / bl of a landmark: its rows are contiguous
//   rowW [F][18]  landmark-major over the F edges of FREE cameras (fpos): W = w B^T A
// (W Dinv and W Dinv bl of a trial never reach global memory: the Schur pass forms them in LDS from the staged W rows.)
struct SeqWin {
  int32_t P, L, E, nfree, nact, iterations;
  int32_t C, C2, n_sc, n_hc;          // rows per Schur chunk / per Hessian chunk, number of chunks
  double fx, fy, cx, cy, delta;
  double *poses, *poses_t;            // [P][7] accepted / trial state
  double *pts, *pts_t;                // [L][3]
  double *out_poses, *out_pts;        // the accepted state at the end (what the host fetches)
  const int32_t *free_pose, *act_pt;  // [nfree], [nact]
  const int32_t *e_pose, *e_point;    // [E]
  const double *e_obs, *e_info;       // [E][2], [E]
  const int32_t *lpos, *fpos;         // [E] row of the edge in landmark-major order over all edges / over free-camera edges (-1)
  const int32_t *pt_start, *f_start;  // [nact + 1] a landmark's rows in rowA / in rowW
  const int32_t *f_cam;               // [F] free camera index of the row
  double *rowB, *rowA, *rowW;
  double *e_chi2, *e_rho;             // [E] chi2 / rho(chi2) of the last evaluation, edge order
  uint8_t* e_depth;                   // [E] isDepthPositive() at the final state
  // Hessian chunks (edge order, C2 rows each), one fixed-size int block per chunk:
  // [per camera the range of its rows in the list (nfree + 1) | the chunk's free-camera row slots, camera-major (C2)]
  const int32_t *hc_ints;             // [n_hc][nfree + 1 + C2]
  // Schur chunks (whole landmarks, <= C free rows, <= C landmarks): descriptor {first row, rows, int offset, int length, runs, pairs, first
  // landmark, landmarks}; int block = [per camera the range of its rows (nfree + 1) | row slots camera-major (rows) | landmark of every row,
  // relative (rows) | runs: i1 | i2 << 8 | first pair << 16, + sentinel | pairs: slot1 | slot2 << 16, sorted by block]
  const int32_t *sc_desc, *sc_ints;   // [n_sc][8]
  double *Hpp, *bp, *HB, *DD, *x, *terms;   // [nfree][36], [6 nfree], [nact][12] = Hll (9) bl (3), [nact][12] = Dinv (9) Dinv bl (3), [6 nfree + 3 nact] x 2
  dvm_ba_stats* stats;
  unsigned long long* prof;           // [16] shader-clock cycles per phase, accumulated by thread 0 (DVM_BA_WINDOW_PROF=1), or null
};

// ------------------------------------------------------------------------------------------------ the sequential sum
// sum of v[0..n) in index order, s = ((0 + v0) + v1) + ..., by ONE wave: 64 values at a time go lane -> LDS, every lane then adds them
// with uniform-address (broadcast) reads -- the chain of dependent v_add_f64 is the cost (8 cycles per value), the next 64 values
// are in flight meanwhile.  Padding a short last chunk with +0.0 is exact (s + 0.0 == s; s is never -0.0: it starts as +0.0).
__device__ double wave_sequential_sum(const double* __restrict__ v, int n, double* __restrict__ buf /* 128 doubles of LDS, this wave's */) {
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  double mine = lane < n ? v[lane] : 0.0;
  for (int base = 0, c = 0; base < n; base += 64, c ^= 1) {
    double* b = buf + 64 * c;
    b[lane] = mine;
    const int nx = base + 64 + lane;
    mine = nx < n ? v[nx] : 0.0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // 16 values at a time into registers, the next 16 requested before the current 16 are added: left to itself the compiler waits
    // for every ds_read right in front of its add (~26 cycles per value instead of the add's own 8)
    double t[2][16];
#pragma unroll
    for (int j = 0; j < 16; j++) t[0][j] = b[j];
#pragma unroll
    for (int g = 0; g < 4; g++) {
      if (g < 3) {
#pragma unroll
        for (int j = 0; j < 16; j++) t[(g + 1) & 1][j] = b[16 * (g + 1) + j];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 16; j++) s += t[g & 1][j];
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  return s;
}

// ------------------------------------------------------------------------------------------------ edge pass
// JAC = false: computeActiveErrors -- chi2 and rho of every edge at the state (poses, pts).  JAC = true: additionally linearizeOplus +
// the edge's part of constructQuadraticForm: A (2x3), B (2x6), w = rho' Omega, wr = -Omega e rho', W = w B^T A, each into the row its
// consumer will stream.  CAM: the window's camera (proj_edge.h); instantiated for the pinhole camera only (win_cam, ba_window_common.h).
template <bool JAC, class CAM>
__device__ void win_edge_pass(const SeqWin& W, const double* __restrict__ poses, const double* __restrict__ pts) {
  const CAM cam = win_cam<CAM>(W);
  for (int k = threadIdx.x; k < W.E; k += kWinThreads) {
    const int p = W.e_pose[k], l = W.e_point[k];
    const double* T = poses + 7 * (size_t)p;
    const double* X = pts + 3 * (size_t)l;
    double R[9];
    quat_to_R(T + 3, R);
    const ProjEdge<CAM> e(cam, R, T, X, W.e_obs[2 * k], W.e_obs[2 * k + 1], W.e_info[k]);
    double r0, r1;
    robustify(e.chi2, W.delta, r0, r1);
    W.e_chi2[k] = e.chi2;
    W.e_rho[k] = r0;
    if (!JAC) continue;
    double A[6], B[12];
    e.jac_point(cam, R, A);
    e.jac_pose(cam, B);
    const double w = e.w(r1), wr0 = e.wr0(r1), wr1 = e.wr1(r1);
    double* oB = W.rowB + kRowB * (size_t)k;
    double* oA = W.rowA + kRowA * (size_t)W.lpos[k];
#pragma unroll
    for (int i = 0; i < 12; i++) oB[i] = B[i];
    oB[12] = w; oB[13] = wr0; oB[14] = wr1; oB[15] = 1.0;       // (slot 15: the "weight" of a bp chain step, see win_accumulate_cameras)
#pragma unroll
    for (int i = 0; i < 6; i++) oA[i] = A[i];
    oA[6] = w; oA[7] = wr0; oA[8] = wr1;
    const int fp = W.fpos[k];
    if (fp >= 0) {
      double* oW = W.rowW + kRowW * (size_t)fp;
#pragma unroll
      for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) oW[3 * a + b] = proj_edge_hpl(w, B, A, a, b);
    }
  }
}

// A chunk of a streamed pass travels global memory -> registers -> LDS: every thread fetches its share of the NEXT chunk (fixed
// stride, a handful of values) before the current one is consumed, so the round trip to L2 runs under the chain steps instead of in
// front of them (a copy loop per chunk cost ~6 us of dependent latencies: descriptor -> rows -> LDS -> barrier).
template <int ND, int NI>
struct ChunkRegs {
  double d[ND];
  int32_t i[NI];
  __device__ __forceinline__ void load_d(int slot0, const double* __restrict__ src, int n) {     // values slot0, slot0 + 1, ... of this thread
#pragma unroll
    for (int u = 0; u < ND; u++) if (u >= slot0) { const int idx = threadIdx.x + (u - slot0) * kWinThreads; d[u] = idx < n ? src[idx] : 0.0; }
  }
  __device__ __forceinline__ void load_i(const int32_t* __restrict__ src, int n) {
#pragma unroll
    for (int u = 0; u < NI; u++) { const int idx = threadIdx.x + u * kWinThreads; i[u] = idx < n ? src[idx] : 0; }
  }
};
template <int N0, int N1, int ND, int NI>
__device__ __forceinline__ void store_d(const ChunkRegs<ND, NI>& r, double* __restrict__ dst, int n) {   // registers N0 .. N1 - 1 -> dst
#pragma unroll
  for (int u = N0; u < N1; u++) { const int idx = threadIdx.x + (u - N0) * kWinThreads; if (idx < n) dst[idx] = r.d[u]; }
}
template <int ND, int NI>
__device__ __forceinline__ void store_i(const ChunkRegs<ND, NI>& r, int32_t* __restrict__ dst, int n) {
#pragma unroll
  for (int u = 0; u < NI; u++) { const int idx = threadIdx.x + u * kWinThreads; if (idx < n) dst[idx] = r.i[u]; }
}

// Hpp / bp of the free cameras: every entry is ONE lane's chain over the camera's edges in edge order (BaseBinaryEdge::
// constructQuadraticForm is called edge by edge).  The B rows stream through LDS C2 edges at a time, the chunk's rows listed per
// camera (host tables), so that a chain step is a few LDS reads.  21 lower (a, b) entries + 6 of bp = 27 lanes per camera, at most two
// (camera, entry) pairs per thread (27 * 30 <= 2 * 512).
__device__ void win_accumulate_cameras(const SeqWin& W, double* stage) {
  const int tid = threadIdx.x, nlanes = 27 * W.nfree;
  double* rows = stage;                                               // [C2][16]
  int32_t* ints = reinterpret_cast<int32_t*>(rows + (size_t)W.C2 * kRowB);   // [nfree + 1] ranges | [<= C2] row slots, camera-major
  double acc[2] = {0.0, 0.0};
  int cam[2], ea[2], eb[2];
  // one form for both kinds of chain: acc += row[ow] * (row[o1] * row[o2] + row[o3] * row[o4]) -- an Hpp entry (a, b): w * (B_a B_b + B_6+a B_6+b);
  // a bp entry a: 1.0 * (B_a wr0 + B_6+a wr1), and 1.0 * x is x
  int o1[2], o2[2], o3[2], o4[2], ow[2];
#pragma unroll
  for (int u = 0; u < 2; u++) {
    const int t = tid + u * kWinThreads;
    cam[u] = t < nlanes ? t / 27 : -1;
    const int e = t - 27 * (t / 27);
    int a, b;
    if (e < 21) { a = 0; int r = e; while (r > a) { r -= a + 1; a++; } b = r; }   // e = a (a + 1) / 2 + b, b <= a
    else { a = e - 21; b = -1; }                                                   // bp(a)
    ea[u] = a; eb[u] = b;
    o1[u] = a; o3[u] = 6 + a;
    if (b >= 0) { o2[u] = b; o4[u] = 6 + b; ow[u] = 12; } else { o2[u] = 13; o4[u] = 14; ow[u] = 15; }
  }
  if (W.n_hc > 0) {
    // chunk c = edges [c C2, c C2 + C2) and the int block at c * (nfree + 1 + C2): nothing to look up before its loads can go out
    const int istride = W.nfree + 1 + W.C2;
    ChunkRegs<8, 1> pre;
    pre.load_d(0, W.rowB, min(W.C2, W.E) * kRowB);
    pre.load_i(W.hc_ints, istride);
    for (int c = 0; c < W.n_hc; c++) {
      const int nr = min(W.C2, W.E - c * W.C2);
      lds_barrier();                                                  // the previous chunk has been consumed
      store_d<0, 8>(pre, rows, nr * kRowB);
      store_i(pre, ints, istride);
      if (c + 1 < W.n_hc) {
        const int k1 = (c + 1) * W.C2;
        pre.load_d(0, W.rowB + kRowB * (size_t)k1, min(W.C2, W.E - k1) * kRowB);
        pre.load_i(W.hc_ints + (size_t)(c + 1) * istride, istride);
      }
      lds_barrier();
      const int32_t* range = ints;
      const int32_t* list = ints + W.nfree + 1;
#pragma unroll
      for (int u = 0; u < 2; u++) {
        if (cam[u] < 0) continue;
        double sacc = acc[u];
        const int q1 = range[cam[u] + 1];
        // four steps at a time: their operands are fetched together, then the four dependent additions; a step beyond the camera's
        // range adds +0.0, which changes nothing (the accumulator is never -0.0)
        for (int q = range[cam[u]]; q < q1; q += 4) {
          double term[4];
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const bool in = q + j < q1;
            const double* B = rows + kRowB * (in ? list[q + j] : 0);
            const double v = B[ow[u]] * (B[o1[u]] * B[o2[u]] + B[o3[u]] * B[o4[u]]);
            term[j] = in ? v : 0.0;
          }
#pragma unroll
          for (int j = 0; j < 4; j++) sacc += term[j];
        }
        acc[u] = sacc;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 2; u++) {
    if (cam[u] < 0) continue;
    const int i = cam[u], a = ea[u], b = eb[u];
    if (b >= 0) { W.Hpp[36 * (size_t)i + 6 * a + b] = acc[u]; W.Hpp[36 * (size_t)i + 6 * b + a] = acc[u]; }   // (a product commutes: the mirrored entry has the same bits)
    else W.bp[6 * (size_t)i + a] = acc[u];
  }
}

// Hll / bl of the active landmarks: a thread per landmark, its rows (edge order) are contiguous in rowA
__device__ void win_accumulate_landmarks(const SeqWin& W) {
  for (int li = threadIdx.x; li < W.nact; li += kWinThreads) {
    double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
    for (int q = W.pt_start[li]; q < W.pt_start[li + 1]; q++) {
      const double* A = W.rowA + kRowA * (size_t)q;
      const double w = A[6], wr0 = A[7], wr1 = A[8];
#pragma unroll
      for (int a = 0; a < 3; a++) {
        g[a] += A[a] * wr0 + A[3 + a] * wr1;
#pragma unroll
        for (int b = 0; b < 3; b++) h[3 * a + b] += w * (A[a] * A[b] + A[3 + a] * A[3 + b]);
      }
    }
    double* o = W.HB + kRowH * (size_t)li;
#pragma unroll
    for (int i = 0; i < 9; i++) o[i] = h[i];
#pragma unroll
    for (int i = 0; i < 3; i++) o[9 + i] = g[i];
  }
}

// Cholesky of the reduced system in LDS (packed lower triangle), in place; diag receives L_kk.  Entry (i, j) receives its subtractions
// L(i, k) L(j, k) in ascending k, as the row-wise dot products of the envelope factorisation apply them; L(i, j) = s / L(j, j) by IEEE
// division, L(j, j) = sqrt(s).  Six columns (one camera) at a time -- two barriers per camera instead of two per column: every thread
// factorises the 6 x 6 diagonal block for itself (the same 21 words, the same operations: the same bits in every thread), then its
// rows' six entries of the panel, column by column; the trailing entries then take the six columns' subtractions in ascending k.
// Every entry sees the operations of the column-by-column form in the same order: identical bits.  The panel also goes to Lp
// (n x 7 doubles: an odd pitch in 8-byte words keeps the sixteen rows a half-wave reads apart on different LDS banks; read out of the
// packed triangle, whose rows start at i (i + 1) / 2, the trailing update spent most of its time in bank conflicts).
// (The sequential-order kernel's solve.  The cluster form, whose contract is a tolerance, has its own: win_cholesky_rhs, ba_window_cluster.hip.)
__device__ bool win_cholesky(double* __restrict__ S, double* __restrict__ diag, double* __restrict__ Lp, int n) {
  const int tid = threadIdx.x;
  constexpr int NT = kWinThreads;
  bool ok = true;
  for (int k0 = 0; k0 < n && ok; k0 += 6) {
    double Ld[21], dg[6];    // the diagonal block's factor (lower, packed) and its L_kk
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
      for (int c = 0; c <= a; c++) {
        double v = S[tri(k0 + a, k0 + c)];
#pragma unroll
        for (int k = 0; k < c; k++) v -= Ld[a * (a + 1) / 2 + k] * Ld[c * (c + 1) / 2 + k];
        if (a == c) {
          if (!(v > 0)) ok = false;              // uniform: every thread computes the same word
          dg[a] = sqrt(v);
          Ld[a * (a + 1) / 2 + a] = v;
        } else {
          Ld[a * (a + 1) / 2 + c] = v / dg[c];
        }
      }
    }
    if (!ok) break;
    // (no barrier here: the panel reads rows below the block and writes them and Lp, which the previous step's update has finished with
    //  behind its closing barrier; the block's own factor is written once everybody has read the block -- behind the panel's barrier)
    for (int i = k0 + 6 + tid; i < n; i += NT) {
      double* row = S + tri(i, k0);
      double l[6];
#pragma unroll
      for (int c = 0; c < 6; c++) {
        double v = row[c];
#pragma unroll
        for (int k = 0; k < c; k++) v -= l[k] * Ld[c * (c + 1) / 2 + k];
        l[c] = v / dg[c];
      }
#pragma unroll
      for (int c = 0; c < 6; c++) { row[c] = l[c]; Lp[7 * i + c] = l[c]; }
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int a = 0; a < 6; a++) {
        diag[k0 + a] = dg[a];
#pragma unroll
        for (int c = 0; c < a; c++) S[tri(k0 + a, k0 + c)] = Ld[a * (a + 1) / 2 + c];
      }
    }
    const int tx = tid & 15, ty = tid >> 4;
    for (int i = k0 + 6 + ty; i < n; i += NT / 16) {
      const double* ri = Lp + 7 * i;
      const double li0 = ri[0], li1 = ri[1], li2 = ri[2], li3 = ri[3], li4 = ri[4], li5 = ri[5];
      double* Si = S + tri(i, 0);
      for (int j = k0 + 6 + tx; j <= i; j += 16) {
        const double* rj = Lp + 7 * j;
        double v = Si[j];
        v -= li0 * rj[0]; v -= li1 * rj[1]; v -= li2 * rj[2]; v -= li3 * rj[3]; v -= li4 * rj[4]; v -= li5 * rj[5];
        Si[j] = v;
      }
    }
    __syncthreads();
  }
  return ok;
}
// forward substitution: y(i) = (b(i) - sum_{j < i} L(i, j) y(j)) / L(i, i), the subtractions in ascending j; then backward:
// x(i) /= L(i, i); x(j) -= L(i, j) x(i) for j < i, i descending.  ONE wave (the caller's wave 0), a camera's six unknowns per step:
// every lane forms the six values for itself, then applies them to its rows in the order of the one-at-a-time form.
__device__ void win_substitute(const double* __restrict__ S, const double* __restrict__ diag, double* __restrict__ rhs, int n) {
  const int lane = threadIdx.x & 63;
  for (int k0 = 0; k0 < n; k0 += 6) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double y[6];
#pragma unroll
    for (int a = 0; a < 6; a++) {
      double v = rhs[k0 + a];
#pragma unroll
      for (int c = 0; c < a; c++) v -= S[tri(k0 + a, k0 + c)] * y[c];
      y[a] = v / diag[k0 + a];
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 6) { double yv = y[0]; yv = lane == 1 ? y[1] : yv; yv = lane == 2 ? y[2] : yv; yv = lane == 3 ? y[3] : yv; yv = lane == 4 ? y[4] : yv; yv = lane == 5 ? y[5] : yv; rhs[k0 + lane] = yv; }
    for (int r = k0 + 6 + lane; r < n; r += 64) {
      const double* rr = S + tri(r, k0);
      double v = rhs[r];
#pragma unroll
      for (int a = 0; a < 6; a++) v -= rr[a] * y[a];
      rhs[r] = v;
    }
  }
  for (int k0 = n - 6; k0 >= 0; k0 -= 6) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double x6[6];
#pragma unroll
    for (int a = 5; a >= 0; a--) {
      double v = rhs[k0 + a];
#pragma unroll
      for (int c = 5; c > a; c--) v -= S[tri(k0 + c, k0 + a)] * x6[c];
      x6[a] = v / diag[k0 + a];
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 6) { double xv = x6[0]; xv = lane == 1 ? x6[1] : xv; xv = lane == 2 ? x6[2] : xv; xv = lane == 3 ? x6[3] : xv; xv = lane == 4 ? x6[4] : xv; xv = lane == 5 ? x6[5] : xv; rhs[k0 + lane] = xv; }
    for (int j = lane; j < k0; j += 64) {
      double v = rhs[j];
#pragma unroll
      for (int a = 5; a >= 0; a--) v -= S[tri(k0 + a, j)] * x6[a];
      rhs[j] = v;
    }
  }
}

// solve(lambda), first half (block_solver.hpp:381-439): Dinv = (Hll + lambda I)^-1 per landmark, then landmark by landmark, per landmark
// every (edge, edge) pair of free cameras: Hschur(i1, i2) -= (W1 Dinv) W2^T, bschur(i1) -= W1 Dinv bl.  S and rhs live in LDS and start
// as Hpp + lambda I / bp.  The landmarks stream through LDS in chunks of whole landmarks: their Hll | bl and their W rows arrive by the
// register pipeline above, Dinv / Dinv bl are formed in place (and stored for the back substitution), W Dinv / W Dinv bl are formed
// in LDS -- they never exist in global memory --, and the chunk's pairs, listed by block, are applied: the 36 entries of a block's run
// are 36 work items; a block appears in ONE run per chunk and the chunks follow each other behind barriers, so every entry of S
// receives its subtractions in landmark order -- the order of g2o's loop.  rhs(6 i + a) likewise walks camera i's rows of the chunk.
__device__ void win_schur(const SeqWin& W, double* S, double* rhs, double* stage, double lambda) {
  const int tid = threadIdx.x, n = 6 * W.nfree;
  double* __restrict__ Wb = stage;                                    // [C][18]
  double* __restrict__ Db = Wb + (size_t)W.C * kRowW;                 // [C][24]
  double* __restrict__ Hl = Db + (size_t)W.C * kRowD;                 // [C][12]  Hll | bl  ->  Dinv | Dinv bl
  int32_t* ints = reinterpret_cast<int32_t*>(Hl + (size_t)W.C * kRowH);
  for (int i = tid; i < n * (n + 1) / 2; i += kWinThreads) S[i] = 0.0;
  __syncthreads();
  for (int t = tid; t < 21 * W.nfree; t += kWinThreads) {
    const int i = t / 21, e = t - 21 * i;
    int a = 0, r = e; while (r > a) { r -= a + 1; a++; }
    const int b = r;
    S[tri(6 * i + a, 6 * i + b)] = W.Hpp[36 * (size_t)i + 6 * a + b] + (a == b ? lambda : 0.0);
  }
  for (int t = tid; t < n; t += kWinThreads) rhs[t] = W.bp[t];
  if (W.n_sc == 0) { __syncthreads(); return; }
  struct Desc { int r0, nr, ioff, ni, nu, np, la, nlm; };
  const Desc* descs = reinterpret_cast<const Desc*>(W.sc_desc);
  ChunkRegs<8, 6> pre;               // W rows: C * 18 <= 5 per thread; Hll | bl: C * 12 <= 3 per thread; ints <= 6 per thread
  Desc dsc = descs[0], nxt = descs[W.n_sc > 1 ? 1 : 0];      // the descriptor of chunk c + 1 is in registers a chunk before its loads go out
  pre.load_d(0, W.rowW + kRowW * (size_t)dsc.r0, dsc.nr * kRowW);
  pre.load_d(5, W.HB + kRowH * (size_t)dsc.la, dsc.nlm * kRowH);
  pre.load_i(W.sc_ints + dsc.ioff, dsc.ni);
  unsigned long long tp = __builtin_amdgcn_s_memtime();
  auto lap2 = [&](int slot) { if (W.prof && tid == 0) { const unsigned long long t = __builtin_amdgcn_s_memtime(); W.prof[slot] += t - tp; tp = t; } };
  for (int c = 0; c < W.n_sc; c++) {
    const Desc cur = dsc;
    lds_barrier();
    lap2(11);
    store_d<0, 5>(pre, Wb, cur.nr * kRowW);
    store_d<5, 8>(pre, Hl, cur.nlm * kRowH);
    store_i(pre, ints, cur.ni);
    if (c + 1 < W.n_sc) {
      dsc = nxt;
      pre.load_d(0, W.rowW + kRowW * (size_t)dsc.r0, dsc.nr * kRowW);
      pre.load_d(5, W.HB + kRowH * (size_t)dsc.la, dsc.nlm * kRowH);
      pre.load_i(W.sc_ints + dsc.ioff, dsc.ni);
      if (c + 2 < W.n_sc) nxt = descs[c + 2];
    }
    lds_barrier();
    lap2(12);
    const int32_t* crange = ints;
    const int32_t* crows = crange + W.nfree + 1;
    const int32_t* rowlm = crows + cur.nr;
    const int32_t* runs = rowlm + cur.nr;
    const int32_t* pairs = runs + cur.nu;
    if (tid < cur.nlm) {             // Dinv, Dinv bl of the chunk's landmarks, in place
      double* h = Hl + kRowH * tid;
      double D[9], Di[9], d3[3];
#pragma unroll
      for (int i = 0; i < 9; i++) D[i] = h[i];
      const double g[3] = {h[9], h[10], h[11]};
      D[0] += lambda; D[4] += lambda; D[8] += lambda;
      inv3(D, Di);
      mat3_vec(Di, g, d3);
      double* o = W.DD + kRowH * (size_t)(cur.la + tid);
#pragma unroll
      for (int i = 0; i < 9; i++) { h[i] = Di[i]; o[i] = Di[i]; }
#pragma unroll
      for (int i = 0; i < 3; i++) { h[9 + i] = d3[i]; o[9 + i] = d3[i]; }
    }
    lds_barrier();
    lap2(13);
    // W Dinv (18) and W Dinv bl (6) of every row: three entries of a thread at a time, operands first (each alone is two dependent LDS
    // round trips for five flops)
    for (int e0 = tid; e0 < cur.nr * kRowD; e0 += 3 * kWinThreads) {
      double w0[3], w1[3], w2[3], h0[3], h1[3], h2[3];
#pragma unroll
      for (int u = 0; u < 3; u++) {
        const int e = min(e0 + u * kWinThreads, cur.nr * kRowD - 1);
        const int row = e / kRowD, j = e - kRowD * row;
        const double* h = Hl + kRowH * rowlm[row];
        const int a = j < 18 ? j / 3 : j - 18;
        const double* W1 = Wb + kRowW * row + 3 * a;
        w0[u] = W1[0]; w1[u] = W1[1]; w2[u] = W1[2];
        if (j < 18) { const int b = j - 3 * a; h0[u] = h[b]; h1[u] = h[3 + b]; h2[u] = h[6 + b]; }
        else { h0[u] = h[9]; h1[u] = h[10]; h2[u] = h[11]; }
      }
#pragma unroll
      for (int u = 0; u < 3; u++) {
        const int e = e0 + u * kWinThreads;
        if (e < cur.nr * kRowD) Db[e] = w0[u] * h0[u] + w1[u] * h1[u] + w2[u] * h2[u];
      }
    }
    lds_barrier();
    lap2(14);
    for (int t = tid; t < n; t += kWinThreads) {
      const int i = t / 6, a = t - 6 * i;
      double sacc = rhs[t];
      const int q1 = crange[i + 1];
      for (int q = crange[i]; q < q1; q += 4) {                       // (four steps' operands together; a step beyond the range subtracts +0.0)
        double term[4];
#pragma unroll
        for (int j = 0; j < 4; j++) { const bool in = q + j < q1; const double v = Db[kRowD * (in ? crows[q + j] : 0) + 18 + a]; term[j] = in ? v : 0.0; }
#pragma unroll
        for (int j = 0; j < 4; j++) sacc -= term[j];
      }
      rhs[t] = sacc;
    }
    lap2(3);
    if (6 * (cur.nu - 1) >= kWinThreads / 2) {
      // many short runs (a window of many cameras): a work item = row a of a block's run -- its three W Dinv values meet all six
      // columns of W2 (b <= a on a diagonal block)
      for (int t = tid; t < 6 * (cur.nu - 1); t += kWinThreads) {
        const int ru = t / 6, a = t - 6 * ru;
        const int rw = runs[ru], i1 = rw & 255, i2 = (rw >> 8) & 255, q0 = rw >> 16, q1 = runs[ru + 1] >> 16;
        const int nb = i1 == i2 ? a + 1 : 6;
        double* Srow = S + tri(6 * i1 + a, 6 * i2);
        double sv[6];
#pragma unroll
        for (int b = 0; b < 6; b++) sv[b] = b < nb ? Srow[b] : 0.0;
        for (int q = q0; q < q1; q++) {
          const int pr = pairs[q];
          const double* WD = Db + kRowD * (pr & 0xffff) + 3 * a;
          const double* W2 = Wb + kRowW * (pr >> 16);
          const double d0 = WD[0], d1 = WD[1], d2 = WD[2];
#pragma unroll
          for (int b = 0; b < 6; b++) sv[b] -= d0 * W2[3 * b] + d1 * W2[3 * b + 1] + d2 * W2[3 * b + 2];
        }
#pragma unroll
        for (int b = 0; b < 6; b++) if (b < nb) Srow[b] = sv[b];
      }
    } else {
      // few long runs (two or three cameras): a work item = one entry (a, b) of a block's run, its pairs two at a time
      for (int t = tid; t < 36 * (cur.nu - 1); t += kWinThreads) {
        const int ru = t / 36, ab = t - 36 * ru, a = ab / 6, b = ab - 6 * a;
        const int rw = runs[ru], i1 = rw & 255, i2 = (rw >> 8) & 255, q0 = rw >> 16, q1 = runs[ru + 1] >> 16;
        if (i1 == i2 && b > a) continue;
        const int idx = tri(6 * i1 + a, 6 * i2 + b);
        double sacc = S[idx];
        for (int q = q0; q < q1; q += 2) {
          double term[2];
#pragma unroll
          for (int j = 0; j < 2; j++) {
            const bool in = q + j < q1;
            const int pr = in ? pairs[q + j] : 0;
            const double* WD = Db + kRowD * (pr & 0xffff) + 3 * a;
            const double* W2 = Wb + kRowW * (pr >> 16) + 3 * b;
            const double v = WD[0] * W2[0] + WD[1] * W2[1] + WD[2] * W2[2];
            term[j] = in ? v : 0.0;
          }
          sacc -= term[0];
          sacc -= term[1];
        }
        S[idx] = sacc;
      }
    }
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------ the kernel
__global__ void __launch_bounds__(kWinThreads) k_ba_window(const SeqWin* __restrict__ wins, const volatile int* __restrict__ stop) {
  extern __shared__ double lds[];
  constexpr int NT = kWinThreads;
  const SeqWin& W = wins[blockIdx.x];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int n = 6 * W.nfree, nl = 3 * W.nact;
  double* S = lds;                                  // packed lower triangle of the reduced camera system, n (n + 1) / 2
  double* rhs = S + (size_t)n * (n + 1) / 2;        // bschur -> x_p                                          [n]
  double* diag = rhs + n;                           // L_kk                                                   [n]
  double* ctl = diag + n;                           // control words shared by the workgroup                  [64]
  double* seqbuf = ctl + 64 + 128 * (wave & 1);     // wave_sequential_sum's buffer (waves 0 and 1 use it)    [2][128]
  double* stage = ctl + 64 + 256;                   // streaming area of the chunked passes                   [stage_doubles]
  dvm_ba_stats* const st = W.stats;                 // written by thread 0 only
  if (tid == 0) win_stats_zero(st);
  // g2o's buildStructure reallocates _x: "the last successful solve" starts as zeros
  for (int i = tid; i < n + nl; i += NT) W.x[i] = 0.0;
  // the trial state starts as a copy (fixed cameras and unobserved landmarks never change)
  for (int i = tid; i < 7 * W.P; i += NT) W.poses_t[i] = W.poses[i];
  for (int i = tid; i < 3 * W.L; i += NT) W.pts_t[i] = W.pts[i];
  double* poses = W.poses; double* poses_t = W.poses_t; double* pts = W.pts; double* pts_t = W.pts_t;
  __syncthreads();

  double lambda = -1, ni = 2, currentChi = 0, chi_last = 0;
  int nBad = 0, it_done = 0, trials_total = 0, stop_reason = 0;
  unsigned long long tprev = __builtin_amdgcn_s_memtime();
  auto lap = [&](int slot) {        // phase timing: thread 0 between barriers
    if (W.prof && tid == 0) { const unsigned long long t = __builtin_amdgcn_s_memtime(); W.prof[slot] += t - tprev; tprev = t; }
  };
  for (int it = 0; it < W.iterations; it++) {
    if (tid == 0) ctl[0] = (stop && *stop) ? 1.0 : 0.0;
    __syncthreads();
    if (ctl[0] != 0.0) break;
    // computeActiveErrors + robust chi2 + buildSystem at the accepted state.  (From the second iteration on g2o recomputes the chi2
    // of the state the last accepted trial has just evaluated: same state, same sums, same bits -- only the Jacobians are new.)
    lap(15);
    win_edge_pass<true, PoseCamPinhole>(W, poses, pts);
    __syncthreads();
    lap(0);
    if (it == 0) {
      if (wave == 0) { const double c = wave_sequential_sum(W.e_rho, W.E, seqbuf); if (tid == 0) ctl[1] = c; }
    }
    win_accumulate_landmarks(W);
    __syncthreads();
    lap(1);
    win_accumulate_cameras(W, stage);
    __syncthreads();
    lap(2);
    if (it == 0) {
      currentChi = ctl[1];
      if (tid == 0) st->chi2_initial = currentChi;
      // computeLambdaInit: tau * max |diagonal| over all active vertices (a maximum has no order)
      double mx = 0;
      for (int i = tid; i < n; i += NT) mx = fmax(mx, fabs(W.Hpp[36 * (size_t)(i / 6) + 7 * (i % 6)]));
      for (int i = tid; i < nl; i += NT) mx = fmax(mx, fabs(W.HB[kRowH * (size_t)(i / 3) + 4 * (i % 3)]));
      for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
      __syncthreads();
      if ((tid & 63) == 0) ctl[8 + wave] = mx;
      __syncthreads();
      mx = ctl[8];
      for (int w2 = 1; w2 < NT / 64; w2++) mx = fmax(mx, ctl[8 + w2]);
      lambda = 1e-5 * mx;
      ni = 2; nBad = 0;
    }
    const double iniChi = currentChi;
    double tempChi = currentChi, rho = 0;
    int qmax = 0;
    bool stopped = false;
    do {
      // ---- solve(lambda): Dinv, Schur complement, reduced right-hand side (one streamed pass)
      lap(3);
      win_schur(W, S, rhs, stage, lambda);
      lap(4);
      // ---- Cholesky + substitution of the reduced system (win_cholesky / win_substitute: the column-by-column operation order)
      const bool ok = win_cholesky(S, diag, ctl + 64, n);       // (Lp: the streaming area is idle during the solve)
      lap(5);
      if (ok) {
        if (wave == 0) win_substitute(S, diag, rhs, n);
        __syncthreads();
        lap(6);
        for (int i = tid; i < n; i += NT) W.x[i] = rhs[i];
        // xl = Dinv (bl - W^T xp): per landmark, its free-camera rows in order, per row the six camera components in order
        for (int li = tid; li < W.nact; li += NT) {
          const double* hb = W.HB + kRowH * (size_t)li;
          double c0 = hb[9], c1 = hb[10], c2 = hb[11];
          for (int q = W.f_start[li]; q < W.f_start[li + 1]; q++) {
            const int i = W.f_cam[q];
            const double* Wk = W.rowW + kRowW * (size_t)q;
#pragma unroll
            for (int a = 0; a < 6; a++) {
              const double xa = rhs[6 * i + a];
              c0 -= Wk[3 * a] * xa; c1 -= Wk[3 * a + 1] * xa; c2 -= Wk[3 * a + 2] * xa;
            }
          }
          const double c[3] = {c0, c1, c2};
          double xl[3];
          mat3_vec(W.DD + kRowH * (size_t)li, c, xl);
          W.x[n + 3 * (size_t)li] = xl[0]; W.x[n + 3 * (size_t)li + 1] = xl[1]; W.x[n + 3 * (size_t)li + 2] = xl[2];
        }
      }
      __syncthreads();
      lap(7);
      // ---- the update is applied and the errors evaluated whether or not the solve succeeded (g2o: x then still holds the last
      // successful solve, optimization_algorithm_levenberg.cpp:107-127); computeScale's terms x_j (lambda x_j + b_j)
      for (int i = tid; i < W.nfree; i += NT) {
        const int p = W.free_pose[i];
        se3_oplus(poses + 7 * (size_t)p, W.x + 6 * (size_t)i, poses_t + 7 * (size_t)p);
      }
      for (int t = tid; t < nl; t += NT) {
        const int l = W.act_pt[t / 3];
        pts_t[3 * (size_t)l + t % 3] = pts[3 * (size_t)l + t % 3] + W.x[n + t];
      }
      for (int j = tid; j < n; j += NT) { const double xj = W.x[j]; W.terms[j] = xj * (lambda * xj + W.bp[j]); }
      for (int j = tid; j < nl; j += NT) { const double xj = W.x[n + j]; W.terms[n + j] = xj * (lambda * xj + W.HB[kRowH * (size_t)(j / 3) + 9 + j % 3]); }
      __syncthreads();
      lap(8);
      win_edge_pass<false, PoseCamPinhole>(W, poses_t, pts_t);
      __syncthreads();
      lap(9);
      if (wave == 0) { const double c = wave_sequential_sum(W.e_rho, W.E, seqbuf); if (tid == 0) ctl[1] = c; }
      if (wave == 1) { const double c = wave_sequential_sum(W.terms, n + nl, seqbuf); if (tid == 64) ctl[2] = c; }
      __syncthreads();
      lap(10);
      // ---- the decision, taken by every thread on the same words (optimization_algorithm_levenberg.cpp:113-147)
      tempChi = ok ? ctl[1] : 1.7976931348623157e308;
      rho = currentChi - tempChi;
      const double scale = ctl[2] + 1e-3;
      rho /= scale;
      if (rho > 0 && isfinite(tempChi)) {
        double alpha = 1. - f64_cube(2 * rho - 1);
        alpha = (2. / 3. < alpha) ? 2. / 3. : alpha;            // std::min(alpha, 2/3) and std::max(1/3, alpha) as the C++ library defines
        lambda *= (1. / 3. < alpha) ? alpha : 1. / 3.;          // them (a NaN alpha passes the first and loses the second; fmin / fmax differ)
        ni = 2;
        currentChi = tempChi;
        double* sw = poses; poses = poses_t; poses_t = sw;      // discardTop(): the trial state becomes the state
        sw = pts; pts = pts_t; pts_t = sw;
        // (the other buffer's fixed cameras / inactive landmarks are the same values: both started as copies of the input)
      } else {
        lambda *= ni;
        ni *= 2;                                               // pop(): the state stays
      }
      qmax++;
      trials_total++;
      if (tid == 0) ctl[0] = (stop && *stop) ? 1.0 : 0.0;
      __syncthreads();
      stopped = ctl[0] != 0.0;
      __syncthreads();
    } while (rho < 0 && qmax < 10 && !stopped);
    it_done++;
    chi_last = currentChi;
    if (tid == 0 && it < 64) { st->trials_per_iter[it] = qmax; st->chi2_per_iter[it] = currentChi; st->lambda_per_iter[it] = lambda; }
    if (qmax == 10 || rho == 0) { stop_reason = 1; break; }
    if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
    if (nBad >= 3) { stop_reason = 2; break; }
  }
  __syncthreads();
  // No iteration ran (iterations == 0, or the stop word was already up at the first poll): no edge pass has written e_chi2 / e_rho, and the
  // caller downloads them (Optimizer_shim's LocalBundleAdjustment erases observations on chi2 > 5.991).  Evaluate the edges at the
  // unchanged input state, so that what leaves is the chi2 OF the state that leaves -- never the previous tenant of the buffer.
  if (it_done == 0) {
    win_edge_pass<false, PoseCamPinhole>(W, poses, pts);
    __syncthreads();
    if (wave == 0) { const double c = wave_sequential_sum(W.e_rho, W.E, seqbuf); if (tid == 0) { st->chi2_initial = c; chi_last = c; } }
    __syncthreads();
  }
  // results: the accepted state (the buffers may have been swapped any number of times), depth signs at that state
  for (int i = tid; i < 7 * W.P; i += NT) W.out_poses[i] = poses[i];
  for (int i = tid; i < 3 * W.L; i += NT) W.out_pts[i] = pts[i];
  for (int k = tid; k < W.E; k += NT) {
    const double* T = poses + 7 * (size_t)W.e_pose[k];
    const double* X = pts + 3 * (size_t)W.e_point[k];
    double R[9], Xc[3];
    quat_to_R(T + 3, R);
    mat3_vec(R, X, Xc);
    W.e_depth[k] = (Xc[2] + T[2]) > 0.0 ? 1 : 0;
  }
  if (tid == 0) {
    st->iterations = it_done; st->total_trials = trials_total; st->chi2_final = chi_last; st->lambda_final = lambda; st->stop_reason = stop_reason;
  }
}

}  // namespace dvm

using namespace dvm;

// K windows -> ONE launch of k_ba_window.  normalize_input: a fresh graph (SE3Quat's constructor normalises the quaternions:
// dvm_ba_optimize_windows) or the state a previous optimize() of the same graph left, taken as it is (ba_solver.cpp's window mode).
int ba_windows_seq(int device, const dvm_ba_window* windows, int K, const volatile uint8_t* stop_flag, dvm_ba_stats* stats, bool normalize_input) {
  if (K < 0 || (K && !windows)) { set_error("dvm_ba_optimize_windows: null windows"); return DVM_ERR_INVALID; }
  if (K == 0) return DVM_OK;
  int rc = dvm_set_device(device);
  if (rc != DVM_OK) return rc;
  WinCall call(windows, K, stop_flag);
  std::vector<SeqBuild> B(K);
  for (int k = 0; k < K; k++) if ((rc = build_window_seq(windows[k], B[k], normalize_input)) != DVM_OK) return rc;
  call.mark(1);
  int* stop_dev = nullptr;
  if ((rc = call.arm(&stop_dev)) != DVM_OK) return rc;

  Stage st;
  struct Slots { int poses, pts, free_pose, act_pt, e_pose, e_point, e_obs, e_info, lpos, fpos, pt_start, f_start, f_cam, hc_ints, sc_desc, sc_ints,
                     poses_t, pts_t, rowB, rowA, rowW, erho, Hpp, bp, HB, DD, x, terms; };
  std::vector<Slots> sl(K);
  auto I32 = [&](const std::vector<int32_t>& v) { return st.in(v.empty() ? nullptr : v.data(), v.size() * 4); };
  auto F64 = [&](const std::vector<double>& v) { return st.in(v.empty() ? nullptr : v.data(), v.size() * 8); };
  for (int k = 0; k < K; k++) {                     // inputs: the state and g2o's graph structure as index arrays
    const SeqBuild& b = B[k]; const WinGraph& g = b.g; Slots& s = sl[k];
    s.poses = F64(g.poses);
    s.pts = st.in(g.L ? windows[k].points : nullptr, 24 * (size_t)g.L);
    s.free_pose = I32(g.free_pose); s.act_pt = I32(g.act_pt); s.e_pose = I32(g.e_pose); s.e_point = I32(g.e_point);
    s.e_obs = F64(g.e_obs); s.e_info = F64(g.e_info);
    s.lpos = I32(b.lpos); s.fpos = I32(b.fpos); s.pt_start = I32(b.pt_start); s.f_start = I32(b.f_start); s.f_cam = I32(b.f_cam);
    s.hc_ints = I32(b.hc_ints); s.sc_desc = I32(b.sc_desc); s.sc_ints = I32(b.sc_ints);
  }
  std::vector<SeqWin> views(K);
  const int views_slot = st.in(views.data(), sizeof(SeqWin) * (size_t)K);   // filled in below, once layout() has placed everything
  call.add_outputs(st);
  for (int k = 0; k < K; k++) {                     // working memory
    const SeqBuild& b = B[k]; Slots& s = sl[k];
    const size_t E = b.g.E, F = b.F, n = 6 * (size_t)b.g.nfree, nl = 3 * (size_t)b.g.nact;
    s.poses_t = st.scratch(56 * (size_t)b.g.P); s.pts_t = st.scratch(24 * (size_t)b.g.L);
    s.rowB = st.scratch(8 * kRowB * E); s.rowA = st.scratch(8 * kRowA * E); s.rowW = st.scratch(8 * kRowW * F);
    s.erho = st.scratch(8 * E);
    s.Hpp = st.scratch(288 * (size_t)b.g.nfree); s.bp = st.scratch(8 * n); s.HB = st.scratch(8 * kRowH * (size_t)b.g.nact); s.DD = st.scratch(8 * kRowH * (size_t)b.g.nact);
    s.x = st.scratch(8 * (n + nl)); s.terms = st.scratch(8 * (n + nl));
  }
  call.mark(2);
  if ((rc = st.layout()) != DVM_OK) return rc;
  call.mark(3);
  size_t lds_doubles = 0;
  for (int k = 0; k < K; k++) {
    const SeqBuild& b = B[k]; const WinGraph& g = b.g; const Slots& s = sl[k]; SeqWin& v = views[k];
    std::memset(&v, 0, sizeof(v));
    v.P = g.P; v.L = g.L; v.E = g.E; v.nfree = g.nfree; v.nact = g.nact; v.iterations = windows[k].iterations;
    v.C = b.C; v.C2 = b.C2; v.n_sc = b.n_sc; v.n_hc = b.n_hc;
    v.fx = windows[k].cam.fx; v.fy = windows[k].cam.fy; v.cx = windows[k].cam.cx; v.cy = windows[k].cam.cy; v.delta = windows[k].cam.huber_delta;
    v.poses = st.ptr<double>(s.poses); v.pts = st.ptr<double>(s.pts); v.poses_t = st.ptr<double>(s.poses_t); v.pts_t = st.ptr<double>(s.pts_t);
    v.free_pose = st.ptr<int32_t>(s.free_pose); v.act_pt = st.ptr<int32_t>(s.act_pt);
    v.e_pose = st.ptr<int32_t>(s.e_pose); v.e_point = st.ptr<int32_t>(s.e_point); v.e_obs = st.ptr<double>(s.e_obs); v.e_info = st.ptr<double>(s.e_info);
    v.lpos = st.ptr<int32_t>(s.lpos); v.fpos = st.ptr<int32_t>(s.fpos); v.pt_start = st.ptr<int32_t>(s.pt_start); v.f_start = st.ptr<int32_t>(s.f_start);
    v.f_cam = st.ptr<int32_t>(s.f_cam);
    v.hc_ints = st.ptr<int32_t>(s.hc_ints); v.sc_desc = st.ptr<int32_t>(s.sc_desc); v.sc_ints = st.ptr<int32_t>(s.sc_ints);
    v.rowB = st.ptr<double>(s.rowB); v.rowA = st.ptr<double>(s.rowA); v.rowW = st.ptr<double>(s.rowW); v.e_rho = st.ptr<double>(s.erho);
    v.Hpp = st.ptr<double>(s.Hpp); v.bp = st.ptr<double>(s.bp); v.HB = st.ptr<double>(s.HB); v.DD = st.ptr<double>(s.DD);
    v.x = st.ptr<double>(s.x); v.terms = st.ptr<double>(s.terms);
    call.fill(st, k, v);
    const size_t n = 6 * (size_t)g.nfree;
    lds_doubles = std::max(lds_doubles, n * (n + 1) / 2 + 2 * n + 64 + 256 + (size_t)b.stage_doubles);
  }
  call.mark(4);
  if ((rc = st.upload()) != DVM_OK) return rc;
  call.mark(5);
  // dynamic LDS: the packed reduced system of the largest window, rhs / diagonal, control words and the streaming area
  const size_t lds_bytes = sizeof(double) * lds_doubles;
  if (lds_bytes > 160 * 1024) { set_error("dvm_ba_optimize_windows: a window needs more than 160 KB of LDS"); return DVM_ERR_CAPACITY; }
  DVM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ba_window), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  // on the staging stream of the calling thread (upload -> kernel -> download is one in-order chain there; the legacy NULL stream would
  // also order this launch against every other thread's staging stream: dvm_ba_optimize_batch's workers serialised on it)
  hipLaunchKernelGGL(k_ba_window, dim3(K), dim3(kWinThreads), lds_bytes, st.stream(), st.ptr<SeqWin>(views_slot), stop_dev);
  DVM_HIP(hipGetLastError());
  if ((rc = call.wait(st, 1)) != DVM_OK) return rc;
  static const char* names[16] = {"edge pass + Jacobians", "Hll / bl", "Hpp / bp (streamed)", "schur: rhs chain", "Schur (streamed)", "Cholesky", "forward / backward", "landmark back-sub",
                                  "oplus + scale terms", "edge pass chi2", "sequential sums", "schur: runs + wait", "schur: store + prefetch", "schur: Dinv", "schur: W Dinv", "decision + rest"};
  call.finish(stats, names, -1);
  return DVM_OK;
}
