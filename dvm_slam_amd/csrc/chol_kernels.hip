// dvm_slam_amd/csrc/chol_kernels.hip -- the sparse tile Cholesky of a TileSystem (tile_system.h) for gfx950, FP64.
//
// The solver of the bundle adjustment's reduced camera system (ba_kernels.hip builds it, ba_solver.cpp drives it) and of the pose graph's
// normal equations (pg_kernels.hip, pg_solver.cpp).  No kernel here knows either problem: they take tiles, schedules and flags.
//   k_chol_diag / k_chol_trsm / k_chol_update / k_chol_trsm_update / k_chol_pair   blocked dense Cholesky on v_mfma_f64_16x16x4, one launch
//                          (or a few) per level of the elimination tree
//   k_chol_backsolve       L^T x = y
//   k_chol_flow            the whole factorisation and solve as one dataflow launch
//   tile_launch_cholesky_solve   picks the form from the TileSystem's members
// Every sum has a fixed order: results are run-to-run deterministic.  The level launches give the same bits on every path (level in one
// launch, slices with the diagonal tiles + update, diag + fused solve/update, one launch per phase, diagonal tiles in or out of the level), and
// so does the flow form.  Two forms sum in an order of their own and agree with those to rounding only: k_chol_pair on its two columns, and
// the back substitution's panel solve of the raw root columns (n_root_raw) against a launched one (tests/test_gpu_tile_solve.py holds all this).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "tile_system.h"

namespace dvm {

// ----------------------------------------------------------------------------------------- K10
// Tile Cholesky of the lower triangle of S (row-major, leading dim ldS), NB = 64, over n1 = n_pad + 1 rows: the
// extra row carries bschur^T, so after the factorisation row n_pad holds y^T with L y = bschur (forward
// substitution for free).  The tile columns are processed LEVEL BY LEVEL of the elimination tree (ba_ordering.h):
// per level one k_chol_diag launch (a workgroup per column: block Cholesky + its inverse), one k_chol_trsm launch
// (all strips of the level as GEMMs with the inverses) and one k_chol_update launch (a workgroup per trailing tile,
// summing its contributing columns in a fixed order: deterministic, no atomics).
constexpr int NB = 64;

__device__ __forceinline__ double bcast_lane(double v, int src_lane) {  // src_lane must be wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
  return __hiloint2double(hi, lo);
}

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef double v2f64 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) v2f64 lds_v2f64;
constexpr int LP = NB + 1;  // LDS pitch (doubles) of a 64x64 block

// Diagonal step kb: Cholesky factor L of the 64x64 block AND its inverse, one workgroup (4 waves).
// The block is processed as four 16-column panels:
//   A. wave 0: the panel (diagonal 16x16 sub-block and all rows below it) row-per-lane in registers, column
//      broadcasts by v_readlane -- the only strictly sequential part (4 x 16 columns instead of 64); the rows below
//      the diagonal are solved by the same instruction stream, and so is the sub-block's INVERSE: the lanes that have
//      no row left (16 / 32 / 48 of them in panels 1 / 2 / 3) carry the rows of the identity, which the panel turns
//      into the columns of the inverse
//   C. trailing sub-blocks:      A_ij -= X_i * X_j^T               (v_mfma_f64_16x16x4_f64, waves 0..2)
// then Linv by block forward substitution, Linv_ij = -Linv_ii * sum_k L_ik Linv_kj, again on MFMA: the
// C/D register layout of the f64 MFMA (row = (lane>>4) + 4*reg, col = lane&15) is exactly its B-operand
// layout for k-step = reg, so the running sum feeds the next product without touching LDS.
// The assembly runs beside the panels on the other waves, ordered by the panels' barriers alone: sub-block 0 (the one panel
// without idle lanes) is inverted by wave 3 beside panel 1, block (1, 0) follows beside panel 2, blocks (2, 0), (2, 1) and the
// three sums of block row 3 beside panel 3.  The tail after the last panel is four MFMAs per block of row 3, one block per
// wave, and the 16-byte store of L^-1.
#ifdef DVM_CHOL_DEBUG
__device__ long long g_chol_dbg[32];
#define DVM_STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_chol_dbg[i] = __builtin_readcyclecounter(); } while (0)
#define DVM_STAMPW(i, w) do { if (blockIdx.x == 0 && threadIdx.x == 64 * (w)) g_chol_dbg[i] = __builtin_readcyclecounter(); } while (0)
#else
#define DVM_STAMP(i) do { } while (0)
#define DVM_STAMPW(i, w) do { } while (0)
#endif
typedef __attribute__((address_space(3))) double lds_f64;
// LDS of one tile factorisation (laid out by the caller, see k_chol_diag): Bm = the tile (rows beyond the matrix: identity), Li = where
// L^-1 goes; Pcol / Iv / Id are scratch (Id must hold the 16x16 identity).
struct DiagLds {
  lds_f64 (*Pcol)[NB];
  lds_f64 (*Iv)[16][17];
  lds_f64* Id;
  lds_f64* Bm;
  lds_f64* Li;
};
// One 64x64 tile in LDS: on return (all threads, behind a barrier) Li holds L^-1 -- every 16x16 block at or below the diagonal;
// the blocks above it are NOT written -- and Bm the blocks of L below the diagonal blocks.  256 threads.
// Hook: what waves 1..3 do for the CALLER beside the last panel, while wave 0 is in the column chain (k_chol_flow: the chain strip of the
// NEXT step travels global -> LDS under the factorisation): hook.begin() before, hook.end() behind their own work there.  NoDiagHook: no code.
struct NoDiagHook { static constexpr bool on = false; __device__ void begin() {} __device__ void end() {} };
template <class Hook>
__device__ __forceinline__ void chol_diag_tile(const DiagLds& D, int* __restrict__ fail, Hook& hook) {
  lds_f64 (*const Pcol)[NB] = D.Pcol;
  lds_f64 (*const Iv)[16][17] = D.Iv;
  lds_f64* const Id = D.Id;
  lds_f64* const Bm = D.Bm;
  lds_f64* const Li = D.Li;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  DVM_STAMP(1);
  const int lr = lane & 15, lq = lane >> 4;
  // inverse of the 16x16 diagonal sub-block bb by one wave: column `lane` of the inverse by forward substitution, L_it straight
  // from LDS (uniform address = broadcast read).  Only sub-block 0 needs it (beside panel 1): the inverses of sub-blocks 1..3
  // fall out of wave 0's own panel, see "identity rows" below.
  auto invert_block = [&](int bb) {
    const int ob = 16 * bb;
    // 1 / L_ii from the L_ii the panel left in the tile (d * rsqrt(d)): one division, lane i's, instead of a store per column there
    const double rl = 1.0 / Bm[(ob + (lane & 15)) * LP + ob + (lane & 15)];
    double y[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
      double s0 = (lane == i) ? 1.0 : 0.0, s1 = 0.0;
#pragma unroll
      for (int t = 0; t < i; t++) {
        const double l = Bm[(ob + i) * LP + ob + t];
        if (t & 1) s1 = __builtin_fma(-l, y[t], s1); else s0 = __builtin_fma(-l, y[t], s0);
      }
      y[i] = (s0 + s1) * bcast_lane(rl, i);
    }
    if (lane < 16) {
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const double v = (lane <= i) ? y[i] : 0.0;
        Iv[bb][lane][i] = v;
        Li[(ob + i) * LP + ob + lane] = v;
      }
    }
  };
  // (The factor of the diagonal tile itself is NOT written back: nothing reads it -- the strips below are solved with L^-1, the
  //  back substitution uses L^-1 and the strips.  S keeps the tile as the Schur complement left it.)
  // L^-1 block (i, j), i > j:  -Iv_i * sum_{k = j .. i - 1} L_ik Linv_kj  (blocks (k, j), k < i, must be in Li already), one wave;
  // the C/D register layout of the f64 MFMA is its B-operand layout for k-step = reg, so the running sum feeds the product
  // with Iv_i without touching LDS
  auto linv_sum = [&](int i, int j) {
    double4_t t = {0, 0, 0, 0};
    for (int k = j; k < i; k++) {
#pragma unroll
      for (int kk = 0; kk < 16; kk += 4)
        t = __builtin_amdgcn_mfma_f64_16x16x4f64(Bm[(16 * i + lr) * LP + 16 * k + kk + lq],
                                                 k == j ? Iv[j][lr][kk + lq] : Li[(16 * k + kk + lq) * LP + 16 * j + lr], t, 0, 0, 0);
    }
    return t;
  };
  auto linv_finish = [&](int i, int j, double4_t t) {
    double4_t r4 = {0, 0, 0, 0};
#pragma unroll
    for (int st = 0; st < 4; st++) r4 = __builtin_amdgcn_mfma_f64_16x16x4f64(Iv[i][4 * st + lq][lr], t[st], r4, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; r++) Li[(16 * i + lq + 4 * r) * LP + 16 * j + lr] = -r4[r];
  };
  auto linv_block = [&](int i, int j) { linv_finish(i, j, linv_sum(i, j)); };
  // the inverse of diagonal sub-block bb, which wave 0's panel left in Iv, into its place in Li (for the final store), one wave
  auto copy_inverse = [&](int bb) {
#pragma unroll
    for (int q = 0; q < 4; q++) Li[(16 * bb + lq + 4 * q) * LP + 16 * bb + lr] = Iv[bb][lr][lq + 4 * q];
  };
  // trailing update of sub-block (i, j) with the columns of panel bs:  A_ij -= X_i X_j^T, one wave
  auto trail = [&](int bs, int i, int j) {
    const int oi = 16 * i, oj = 16 * j, os = 16 * bs;
    double4_t acc = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 16; k += 4)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Bm[(oi + lr) * LP + os + k + lq], Bm[(oj + lr) * LP + os + k + lq], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; r++) Bm[(oi + lq + 4 * r) * LP + oj + lr] -= acc[r];
  };
  // block row 3 of L^-1: its three sums are formed beside the last panel (one per wave 1..3), only the product with Iv_3 -- four
  // MFMAs -- is left for the tail
  double4_t t3a = {0, 0, 0, 0};
  for (int b = 0; b < 4; b++) {
    const int o = 16 * b, nrows = NB - o;
    DVM_STAMP(2 + 3 * b);
    if (Hook::on && b == 3 && wave != 0) hook.begin();
    if (wave == 0) {
      // ---- A: the whole 16-column PANEL (diagonal sub-block + every row below it) in registers, lane = panel row;
      // the rows below the diagonal sub-block ride along in the same instructions (no separate triangular solve).
      // Right-looking: a finished column j updates every later column c of every row, a_c -= L_ij * L_cj.  The factor
      // L_cj is the same for all lanes: column j is published to LDS once and read back with uniform-address (broadcast)
      // reads -- except for c = j + 1, the next pivot column, which gets it by v_readlane.  The 16 columns are ONE
      // straight-line stream written by tools/gen_chol_panel.py (chol_panel.inc): this wave owns its SIMD and issues in order,
      // nothing overlaps, so the panel costs the sum of its instructions' issue times (5.3 cycles an FP64 operation, 8.3
      // when it needs the previous one, ~20 the rsq, ~30 a store behind an exec-mask round trip) -- the stream carries
      // nothing the factorisation does not need (no sqrt for L_jj, which nobody reads; one positivity test per panel; the
      // 1 / L_jj store from every lane) and a filler between any two dependent chain steps.  Cycle stamps per panel,
      // 2.4 GHz: 7 400 with every L_cj by v_readlane, 5 850 as the rolled loop the compiler scheduled (366 / column),
      // 3 850-4 150 now (250 / column); chain alone (no updates, no LDS) 2 600.
      double a[16];
      // IDENTITY ROWS: panels 1..3 have 16, 32, 48 lanes without a row.  Sixteen of them carry the rows of the identity: the
      // panel turns a row a_i below the diagonal sub-block into a_i L^-T, so the row e_i comes out as row i of L^-T = column i of
      // the sub-block's inverse -- by the very instructions that factorise the panel, none added: the lane's source and
      // destination pointers differ, that is all.  (Before: a second wave inverted the sub-block from LDS, 2 800 cycles beside
      // the next panel or, for the last one, 1 300 cycles behind this wave.)
      const int idl = lane - nrows;                          // 0..15 in panels 1..3: this lane carries e_idl
      const bool has_row = lane < nrows, is_id = b >= 1 && idl >= 0 && idl < 16;
      const lds_f64* const src = has_row ? Bm + (o + lane) * LP + o : Id + 16 * (idl & 15);
#pragma unroll
      for (int c = 0; c < 16; c++) a[c] = ((has_row || is_id) && (lane >= 16 || c <= lane)) ? src[c] : 0.0;
      bool bad = false;
      double d0 = bcast_lane(a[0], 0);          // pivot a_00, wave-uniform
#include "chol_panel.inc"
      // rows of L back to Bm; identity lanes: Iv_b[column idl][row c] = (L^-1)_{c, idl} (exact zeros above the diagonal, c < idl)
      lds_f64* const dst = has_row ? Bm + (o + lane) * LP + o : &Iv[b][idl & 15][0];
      if (has_row || is_id) {
#pragma unroll
        for (int c = 0; c < 16; c++) dst[c] = (lane < 16 && c > lane) ? 0.0 : a[c];
      }
      // (write-through: inside k_chol_flow other workgroups -- other XCDs -- read the flag before the launch ends: a plain store stayed in this
      //  XCD's L2 and the back substitution wrote x of a failed solve, now and then)
      if (bad && lane == 0) __hip_atomic_store(fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (b >= 1) {
      // beside the panel, no flags (everything is ordered by the panels' barriers): first the trailing updates of the PREVIOUS
      // panel that the current one does not need (sub-blocks right of its block column, see C below), then the pieces of L^-1
      // whose inputs are final: panel 1 -- wave 3 inverts sub-block 0; panel 2 -- wave 1 assembles block (1, 0); panel 3 --
      // blocks (2, 0), (2, 1) and the sums of block row 3, one per wave
      if (b == 1) {
        if (wave == 1) trail(0, 2, 2); else if (wave == 2) { trail(0, 3, 2); trail(0, 3, 3); } else invert_block(0);
      } else if (b == 2) {
        if (wave == 1) linv_block(1, 0);
        else if (wave == 2) copy_inverse(1);
        else trail(1, 3, 3);
      } else {
        if (wave == 3) { linv_block(2, 0); t3a = linv_sum(3, 0); }
        else if (wave == 1) { linv_block(2, 1); t3a = linv_sum(3, 1); }
        else { t3a = linv_sum(3, 2); copy_inverse(2); }
      }
    }
    if (Hook::on && b == 3 && wave != 0) hook.end();
    DVM_STAMP(3 + 3 * b);
    if (b == 3) { DVM_STAMPW(18, 1); DVM_STAMPW(19, 2); DVM_STAMPW(20, 3); }
    __syncthreads();
    DVM_STAMP(4 + 3 * b);
    if (b < 3) {
      // ---- C: trailing sub-blocks.  Only the next panel's block column (i, b + 1), i > b, is on the critical path: one wave
      // each, one round; the sub-blocks right of it are updated beside the next panel (A above) -- same operands, same order per
      // sub-block (panel b's contribution lands before panel b + 1's, a barrier in between), same bits.
      if (wave >= 1 && b + wave < 4) trail(b, b + wave, b + 1);
      __syncthreads();
    }
  }
  // tail: only L^-1 block row 3 is left (Iv_3 and block rows 0..2 were finished beside the last panel)
  DVM_STAMP(14);
  if (wave >= 1) linv_finish(3, wave == 3 ? 0 : wave, t3a);
  else copy_inverse(3);
  DVM_STAMP(15);
  __syncthreads();
}

__device__ __forceinline__ void chol_diag_tile(const DiagLds& D, int* __restrict__ fail) { NoDiagHook h; chol_diag_tile(D, fail, h); }

__global__ void __launch_bounds__(256) k_chol_diag(double* __restrict__ S, int ldS, int n1, const int32_t* __restrict__ cols,
                                                  int* __restrict__ fail, double* __restrict__ Linv_all) {
  DVM_STAMP(0);
  const int kb = cols[blockIdx.x];
  // One LDS block, laid out by hand: everything that is read with CONSTANT (wave-uniform) addresses sits in the first 64 KB,
  // where a ds instruction's 16-bit offset field reaches it -- left to the compiler, Li / Iv / Pcol landed above 64 KB and every
  // such address became a v_mov of a literal parked in an AGPR (hundreds of them in the kernel's prologue).
  __shared__ __attribute__((aligned(16))) double smem[16 * NB + 4 * 16 * 17 + 16 * 16 + 2 * NB * LP];
  lds_f64* const lds = (lds_f64*)smem;
  lds_f64 (*const Pcol)[NB] = (lds_f64 (*)[NB])lds;                                   // the panel's finished columns, one row per column: broadcast source for the updates
  lds_f64 (*const Iv)[16][17] = (lds_f64 (*)[16][17])(lds + 16 * NB);                // inverses of the diagonal sub-blocks, TRANSPOSED: Iv[b][column][row]
  lds_f64* const Id = lds + 16 * NB + 4 * 16 * 17;                            // 16x16 identity: the rows the idle lanes of a panel carry
  lds_f64* const Bm = Id + 16 * 16;
  lds_f64* const Li = Bm + NB * LP;
  const int tid = threadIdx.x;
  const int k0 = kb * NB;
  const int kw = min(NB, n1 - k0);
  {
    // the whole tile with 8 independent 16-byte loads per thread, issued back to back (a load per loop iteration behind a
    // branch serialised 16 global round trips: ~13 of the kernel's 27 us); rows beyond the matrix are clamped and replaced
    double2 v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int r = 8 * i + (tid >> 5), c = 2 * (tid & 31);
      v[i] = *reinterpret_cast<const double2*>(S + (size_t)(k0 + min(r, kw - 1)) * ldS + k0 + c);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int r = 8 * i + (tid >> 5), c = 2 * (tid & 31);
      const bool in = r < kw;
      // rows beyond the matrix: identity.  (What lands ABOVE the diagonal is never read: the panel masks the upper triangle of
      // its diagonal sub-block, everything else works on blocks at or below the diagonal.)
      Bm[r * LP + c] = in ? v[i].x : (r == c ? 1.0 : 0.0);
      Bm[r * LP + c + 1] = in ? v[i].y : (r == c + 1 ? 1.0 : 0.0);
    }
  }
  Id[tid] = (tid >> 4) == (tid & 15) ? 1.0 : 0.0;
  __syncthreads();
  const DiagLds D = {Pcol, Iv, Id, Bm, Li};
  chol_diag_tile(D, fail);
  DVM_STAMP(16);
  double* Lo = Linv_all + (size_t)kb * NB * NB;
#pragma unroll
  for (int k = 0; k < 8; k++) {            // 16-byte stores: a wave writes 1 KB per instruction
    const int r = 8 * k + (tid >> 5), c = 2 * (tid & 31);
    const bool lower = (c >> 4) <= (r >> 4);     // the 16x16 blocks above the diagonal were never written in LDS: zeros from here
    const double2 v = lower ? make_double2(Li[r * LP + c], Li[r * LP + c + 1]) : make_double2(0.0, 0.0);
    *reinterpret_cast<double2*>(Lo + r * NB + c) = v;
  }
  DVM_STAMP(17);
}
// x of tile column kb, row t (value v) into the compact solution vector: a camera tile holds per_tile unknowns of dof rows; a tile of kept
// landmarks (kb >= ncamt, TileSystem::kept_list) 21 landmarks of 3 rows, whose x lives behind the cameras' at 3 * landmark
__device__ __forceinline__ void write_x(double* __restrict__ x, int kb, int t, double v, int nfree, int per_tile, int dof, int ncamt, int nkept,
                                        const int32_t* __restrict__ kept_list) {
  if (nkept > 0 && kb >= ncamt) {
    const int j = (kb - ncamt) * 21 + t / 3;
    if (t < 63 && j < nkept) x[dof * (size_t)nfree + 3 * (size_t)kept_list[j] + t % 3] = v;
    return;
  }
  const int cam = kb * per_tile + t / dof;
  if (t < per_tile * dof && cam < nfree) x[dof * (size_t)cam + t % dof] = v;
}
// The TOP PAIR of the elimination order in one workgroup (BaTileSchedule::pair_a / pair_b): column A, whose only tiles below
// the diagonal are (B, A) and the rhs row, and the root column B.  As separate launches this is diag(A) -> panel solve + update
// -> diag(B) -> two hops of the back substitution: five dependent kernels whose tiles travel through memory between them
// (~34 us of an iteration's solve at 500 keyframes, and the WHOLE solve of a local-BA window of <= 20 free keyframes).  Here
// the three tiles and the two rhs pieces are loaded once, everything else happens in LDS:
//   L_A, L_A^-1 (chol_diag_tile) ; X = (B,A) L_A^-T (MFMA, only the k-blocks L_A^-1 has) ; (B,B) -= X X^T (MFMA, lower blocks) ;
//   L_B, L_B^-1 ; y_A = L_A^-1 r_A, y_B = L_B^-1 (r_B - X y_A), x_B = L_B^-T y_B, x_A = L_A^-T (y_A - X^T x_B).
// Four tile buffers (BmA -> X, raw (B,A) -> L_B^-1, BmB, L_A^-1) = 133 KB of the CU's 160 KB.  Nothing but x leaves: no one
// else reads these columns' factor (their descendants need x_A / x_B, which go to xrow like any other column's).
__global__ void __launch_bounds__(256) k_chol_pair(const double* __restrict__ S, int ldS, int n_pad, int kbA, int kbB, int nfree, int per_tile,
                                                  int dof, double* __restrict__ xrow, double* __restrict__ x, int* __restrict__ fail,
                                                  int ncamt, int nkept, const int32_t* __restrict__ kept_list) {
  __shared__ __attribute__((aligned(16))) double smem[16 * NB + 4 * 16 * 17 + 16 * 16 + 4 * NB * LP + 10 * NB];
  lds_f64* const lds = (lds_f64*)smem;
  lds_f64 (*const Pcol)[NB] = (lds_f64 (*)[NB])lds;
  lds_f64 (*const Iv)[16][17] = (lds_f64 (*)[16][17])(lds + 16 * NB);
  lds_f64* const Id = lds + 16 * NB + 4 * 16 * 17;
  lds_f64* const T1 = Id + 16 * 16;          // tile (A,A): L_A; then X = L(B,A)
  lds_f64* const T2 = T1 + NB * LP;          // tile (B,A) as the Schur complement left it; then L_B^-1
  lds_f64* const T3 = T2 + NB * LP;          // tile (B,B)
  lds_f64* const T4 = T3 + NB * LP;          // L_A^-1
  lds_f64* const vr0 = T4 + NB * LP;         // r_A -> y_A -> (y_A - X^T x_B)
  lds_f64* const vr1 = vr0 + NB;             // r_B -> y_B
  lds_f64* const vx0 = vr1 + NB;
  lds_f64* const vx1 = vx0 + NB;
  lds_f64* const vt = vx1 + NB;              // a product's result before it is combined
  lds_f64* const part = vt + NB;             // [4][NB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int a0 = kbA * NB, b0 = kbB * NB;
  {
    double2 va[8], vb[8], vc[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int r = 8 * i + (tid >> 5), c = 2 * (tid & 31);
      va[i] = *reinterpret_cast<const double2*>(S + (size_t)(a0 + r) * ldS + a0 + c);
      vb[i] = *reinterpret_cast<const double2*>(S + (size_t)(b0 + r) * ldS + a0 + c);
      vc[i] = *reinterpret_cast<const double2*>(S + (size_t)(b0 + r) * ldS + b0 + c);
    }
    double rv = 0;
    if (tid < 2 * NB) rv = S[(size_t)n_pad * ldS + (tid < NB ? a0 + tid : b0 + tid - NB)];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int r = 8 * i + (tid >> 5), c = 2 * (tid & 31);
      T1[r * LP + c] = va[i].x; T1[r * LP + c + 1] = va[i].y;
      T2[r * LP + c] = vb[i].x; T2[r * LP + c + 1] = vb[i].y;
      T3[r * LP + c] = vc[i].x; T3[r * LP + c + 1] = vc[i].y;
    }
    if (tid < NB) vr0[tid] = rv; else if (tid < 2 * NB) vr1[tid - NB] = rv;
  }
  Id[tid] = (tid >> 4) == (tid & 15) ? 1.0 : 0.0;
  __syncthreads();
  // the 16x16 blocks above the diagonal of an inverse are never written by chol_diag_tile: zeroed, so that what follows can
  // treat it as a full matrix
  auto zero_upper = [&](lds_f64* M) {
    for (int i = tid; i < 6 * 256; i += 256) {
      const int blk = i >> 8, e = i & 255;
      const int bi = blk < 3 ? 0 : blk < 5 ? 1 : 2, bj = blk < 3 ? blk + 1 : blk < 5 ? blk - 1 : 3;
      M[(16 * bi + (e >> 4)) * LP + 16 * bj + (e & 15)] = 0.0;
    }
  };
  // out[c] = sum_k M[c][k] v[k]   (TR: sum_k M[k][c] v[k]), in a fixed order: 16 terms per thread, then the four quarters
  auto matvec = [&](const lds_f64* M, bool TR, const lds_f64* v, lds_f64* out) {
    const int c = tid & 63, q = tid >> 6;
    double sacc = 0;
#pragma unroll
    for (int kk = 0; kk < 16; kk++) {
      const int k = 16 * q + kk;
      sacc += (TR ? M[k * LP + c] : M[c * LP + k]) * v[k];
    }
    part[q * NB + c] = sacc;
    __syncthreads();
    if (tid < NB) out[tid] = (part[tid] + part[NB + tid]) + (part[2 * NB + tid] + part[3 * NB + tid]);
    __syncthreads();
  };
  const DiagLds DA = {Pcol, Iv, Id, T1, T4};
  chol_diag_tile(DA, fail);
  zero_upper(T4);
  __syncthreads();
  // X = (B,A) L_A^-T: wave w takes block row w; column block bj only needs the k-blocks 0..bj (L_A^-1 is lower triangular)
  {
    double4_t xb[4];
#pragma unroll
    for (int bj = 0; bj < 4; bj++) {
      double4_t acc = {0, 0, 0, 0};
      for (int k = 0; k < 16 * (bj + 1); k += 4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(T2[(16 * wave + lr) * LP + k + lq], T4[(16 * bj + lr) * LP + k + lq], acc, 0, 0, 0);
      xb[bj] = acc;
    }
#pragma unroll
    for (int bj = 0; bj < 4; bj++)
#pragma unroll
      for (int r = 0; r < 4; r++) T1[(16 * wave + lq + 4 * r) * LP + 16 * bj + lr] = xb[bj][r];
  }
  __syncthreads();
  matvec(T4, false, vr0, vr0);                 // y_A = L_A^-1 r_A   (in place: every thread has read v before the first barrier)
  matvec(T1, false, vr0, vt);                  // X y_A
  if (tid < NB) vr1[tid] -= vt[tid];
  // (B,B) -= X X^T, the ten blocks at or below the diagonal dealt over the waves
  {
    const int bis[10] = {0, 1, 1, 2, 2, 2, 3, 3, 3, 3}, bjs[10] = {0, 0, 1, 0, 1, 2, 0, 1, 2, 3};
    for (int t = wave; t < 10; t += 4) {
      const int bi = bis[t], bj = bjs[t];
      double4_t acc = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < NB; k += 4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(T1[(16 * bi + lr) * LP + k + lq], T1[(16 * bj + lr) * LP + k + lq], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; r++) T3[(16 * bi + lq + 4 * r) * LP + 16 * bj + lr] -= acc[r];
    }
  }
  __syncthreads();
  const DiagLds DB = {Pcol, Iv, Id, T3, T2};
  chol_diag_tile(DB, fail);
  zero_upper(T2);
  __syncthreads();
  matvec(T2, false, vr1, vr1);                 // y_B
  matvec(T2, true, vr1, vx1);                  // x_B = L_B^-T y_B
  matvec(T1, true, vx1, vt);                   // X^T x_B
  if (tid < NB) vr0[tid] -= vt[tid];
  __syncthreads();
  matvec(T4, true, vr0, vx0);                  // x_A = L_A^-T (y_A - X^T x_B)
  // g2o's linear solver leaves _x untouched when the factorisation fails (see k_chol_backsolve)
  const bool good = __hip_atomic_load(fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
  if (tid < 2 * NB) {
    const int t = tid & 63, kb = tid < NB ? kbA : kbB;
    const double v = tid < NB ? vx0[t] : vx1[t];
    __hip_atomic_store(xrow + kb * NB + t, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (good) write_x(x, kb, t, v, nfree, per_tile, dof, ncamt, nkept, kept_list);
  }
}

#ifdef DVM_CHOL_DEBUG
extern "C" int dvm_debug_chol_stamps(long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_chol_dbg), sizeof(long long) * 32); }
#endif


// Panel solve of step kb: strip i (64 rows below the diagonal block) becomes X = A_ik * Linv_kk^T
// (a 64x64x64 product on v_mfma_f64_16x16x4_f64) -- the triangular solve as a GEMM, IN PLACE.  One workgroup per 16-ROW
// slice of the strip (grid = 4 x strips), each wave one 16x16 block of it: an f64 MFMA occupies its SIMD for 64 cycles, so a
// whole tile on one workgroup is 1.7 us of matrix pipe alone.  The split is by rows only: a workgroup reads and overwrites
// nothing but its own rows (a split by columns would let one workgroup overwrite A entries another is still reading).
constexpr int QP = 66;   // LDS pitch (doubles): conflict-free for the MFMA operand reads
// (xrow_tag != null on the first solve launch of a factorisation: workgroup 0 also fills the back substitution's hand-off
// slots with kXTag -- see k_chol_backsolve)
constexpr unsigned long long kXTag = 0x7FF8DEADBEEF0002ull;   // a NaN payload no arithmetic produces
__device__ __forceinline__ void tag_xrow(double* __restrict__ xrow, int n) {
  for (int i = threadIdx.x; i < n; i += 256) xrow[i] = __longlong_as_double((long long)kXTag);
}
__global__ void __launch_bounds__(256) k_chol_trsm(double* __restrict__ S, int ldS, int n1,
                                                   const double* __restrict__ Linv_all, const int32_t* __restrict__ strips,
                                                   double* __restrict__ xrow_tag, int n_tag) {
  __shared__ double Ai[16 * QP];
  __shared__ double Li[NB * QP];
  const int tid = threadIdx.x;
  if (xrow_tag && blockIdx.x == 0) tag_xrow(xrow_tag, n_tag);
  const int st = blockIdx.x >> 2, qi = (blockIdx.x & 3) * 16;
  const int kb = strips[2 * st + 1];
  const int k0 = kb * NB;
  const int r0 = strips[2 * st] * NB;  // tile row of a structurally non-zero strip of column kb
  const int rw = min(NB, n1 - r0);
  if (qi >= rw) return;
  const double* Lk = Linv_all + (size_t)kb * NB * NB;
  {
    double2 l[8];
#pragma unroll
    for (int i = 0; i < 8; i++) l[i] = *reinterpret_cast<const double2*>(Lk + (8 * i + (tid >> 5)) * NB + 2 * (tid & 31));
    const int r = tid >> 4, c = 4 * (tid & 15);
    const double* src = S + (size_t)(r0 + min(qi + r, rw - 1)) * ldS + k0 + c;
    const double2 a0 = *reinterpret_cast<const double2*>(src), a1 = *reinterpret_cast<const double2*>(src + 2);
    const bool in = qi + r < rw;
    Ai[r * QP + c] = in ? a0.x : 0.0; Ai[r * QP + c + 1] = in ? a0.y : 0.0;
    Ai[r * QP + c + 2] = in ? a1.x : 0.0; Ai[r * QP + c + 3] = in ? a1.y : 0.0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      Li[(8 * i + (tid >> 5)) * QP + 2 * (tid & 31)] = l[i].x;
      Li[(8 * i + (tid >> 5)) * QP + 2 * (tid & 31) + 1] = l[i].y;
    }
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  const int wj = wave * 16;
  const int lr = lane & 15, lk = lane >> 4;
  double4_t acc = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < NB; k += 4)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ai[lr * QP + k + lk], Li[(wj + lr) * QP + k + lk], acc, 0, 0, 0);
  const int kw = min(NB, n1 - k0);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = qi + lk + 4 * r, col = wj + lr;
    if (row < rw && col < kw) S[(size_t)(r0 + row) * ldS + k0 + col] = acc[r];
  }
}

// Trailing update A_ij -= sum_k A_ik A_jk^T for one 32x32 QUADRANT of a 64x64 tile (ti >= tj) and the columns k of the
// current level that reach it (contrib[c0..c1), ascending: fixed summation order).  grid = 4 x targets; 4 waves, each one
// 16x16 block of the quadrant (v_mfma_f64_16x16x4_f64: A operand: lane l holds A[l&15][l>>4]; B operand: B[l>>4][l&15];
// C/D: 4 doubles per lane, col = l&15, row = (l>>4) + 4*reg).  The half strips of contributor c+1 travel global ->
// registers while contributor c is on the matrix pipe.
__global__ void __launch_bounds__(256) k_chol_update(double* __restrict__ S, int ldS, int n1,
                                                     const int32_t* __restrict__ targets, const int32_t* __restrict__ contrib) {
  __shared__ double Ai[32 * QP];
  __shared__ double Aj[32 * QP];
  const int tg = blockIdx.x >> 2, qi = (blockIdx.x & 2) * 16, qj = (blockIdx.x & 1) * 32;
  const int ti = targets[4 * tg], tj = targets[4 * tg + 1];
  const int c0 = targets[4 * tg + 2], c1 = targets[4 * tg + 3];
  if (ti == tj && qj > qi) return;   // strictly upper quadrant of a diagonal tile
  const int i0 = ti * NB + qi, j0 = tj * NB + qj;
  const int iw = min(32, n1 - i0), jw = min(32, n1 - j0);
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wi = (wave >> 1) * 16, wj = (wave & 1) * 16;
  double4_t acc = {0, 0, 0, 0};
  const int lr = lane & 15, lk = lane >> 4;
  // thread t owns elements (row 4k + t / 64, column t % 64), k = 0..7: every load instruction covers 4 full rows
  const int pr = tid >> 6, pc = tid & 63;
  // the target's own entries are fetched first: they are only needed at the very end, where the load used to be one more
  // dependent round trip behind the last product
  double tgt[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = wi + lk + 4 * r, col = wj + lr;
    tgt[r] = (row < iw && col < jw && (i0 + row) >= (j0 + col)) ? S[(size_t)(i0 + row) * ldS + j0 + col] : 0.0;
  }
  // Three contributors in flight: a contributor's half strips travel global -> registers while the two before it are
  // staged / on the matrix pipe.  With one in flight every contributor cost a full L2 round trip (~2.2 us against 0.43 us of
  // MFMA): the leaf level, where a separator tile collects up to ten columns, took 22 us.
  double ra0[8], rb0[8], ra1[8], rb1[8], ra2[8], rb2[8];
  auto fetch = [&](int c, double* ra, double* rb) {
    const int k0 = contrib[c] * NB;
    const double* ga = S + (size_t)(i0 + pr) * ldS + k0 + pc;
    const double* gb = S + (size_t)(j0 + pr) * ldS + k0 + pc;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      ra[k] = (4 * k + pr < iw) ? ga[(size_t)4 * k * ldS] : 0.0;
      rb[k] = (4 * k + pr < jw) ? gb[(size_t)4 * k * ldS] : 0.0;
    }
  };
  auto step = [&](int c, double* ra, double* rb) {
    if (c > c0) __syncthreads();          // the previous contributor's MFMAs have read Ai / Aj
#pragma unroll
    for (int k = 0; k < 8; k++) { Ai[(4 * k + pr) * QP + pc] = ra[k]; Aj[(4 * k + pr) * QP + pc] = rb[k]; }
    __syncthreads();
    if (c + 3 < c1) fetch(c + 3, ra, rb);
#pragma unroll
    for (int k = 0; k < NB; k += 4)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ai[(wi + lr) * QP + k + lk], Aj[(wj + lr) * QP + k + lk], acc, 0, 0, 0);
  };
  fetch(c0, ra0, rb0);
  if (c0 + 1 < c1) fetch(c0 + 1, ra1, rb1);
  if (c0 + 2 < c1) fetch(c0 + 2, ra2, rb2);
  for (int c = c0; c < c1; c += 3) {
    step(c, ra0, rb0);
    if (c + 1 < c1) step(c + 1, ra1, rb1);
    if (c + 2 < c1) step(c + 2, ra2, rb2);
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = wi + lk + 4 * r, col = wj + lr;
    if (row < iw && col < jw && (i0 + row) >= (j0 + col)) S[(size_t)(i0 + row) * ldS + j0 + col] = tgt[r] - acc[r];
  }
}

// k_chol_trsm and k_chol_update of one level in ONE launch.  Workgroups [0, n_trsm) are the panel solve's 16-row slices,
// the others the update's 32x32 quadrants; a quadrant waits for the slices of the strips it multiplies instead of a kernel
// boundary (4.8 + 5.5 us per level as two launches, each mostly boundary + load latency: ~1.7 us of boundary and one round
// trip less per level).  Hand-off (MI355X_MICROARCH.md, valid forms): the slice is written with 8-byte agent-scope
// (write-through) stores, drained (s_waitcnt vmcnt(0)) before its flag is raised to the solve's sequence number; the reader
// polls the flags with relaxed agent-scope loads on a few lanes and reads the strips with agent-scope loads (no L1, and the
// XCD's L2 cannot hold these lines yet: nothing in this launch reads a strip before its flag).  No deadlock: the launcher
// only uses this kernel when the whole grid is resident at once; a wait is bounded anyway and flags the trial as failed.
//
// kDiag: the level's k_chol_diag launch is folded in as well.  Every slice workgroup factors its column's diagonal tile ITSELF
// (chol_diag_tile in its own LDS: the 12 workgroups of a column with three strips do the same work and get the same bits) while
// its 16 strip rows are already on their way from memory, and multiplies by the L^-1 it finds in LDS: the level loses a kernel
// boundary and the L^-1 store -> load round trip (~2.5 us of ~19); the column's first slice workgroup stores L^-1 for the back
// substitution afterwards, off the critical path.  86 KB of LDS: one workgroup per CU, so the launcher uses it for levels of
// <= 256 workgroups (slices + quadrants, or the slices alone with the update as a second launch).
template <bool kDiag>
__global__ void __launch_bounds__(256) k_chol_trsm_update(double* __restrict__ S, int ldS, int n1, double* __restrict__ Linv_all,
                                                          const int32_t* __restrict__ strips, int strip_base, int n_trsm,
                                                          const int32_t* __restrict__ targets, const int32_t* __restrict__ contrib,
                                                          const int32_t* __restrict__ contrib_strip, int32_t* __restrict__ flags,
                                                          int gen, int gen_pub, int* __restrict__ fail, double* __restrict__ xrow_tag, int n_tag) {
  // trsm: Ai (16 rows) + Li (64 rows); update: Ai + Aj (32 rows each); kDiag: the layout of k_chol_diag (Ai over Pcol / Iv)
  __shared__ __attribute__((aligned(16))) double smem[kDiag ? 16 * NB + 4 * 16 * 17 + 16 * 16 + 2 * NB * LP : 16 * QP + NB * QP];
  const int tid = threadIdx.x;
  if (xrow_tag && blockIdx.x == 0) tag_xrow(xrow_tag, n_tag);
  if (kDiag && (int)blockIdx.x < n_trsm) {
    const int st = blockIdx.x >> 2, sl = blockIdx.x & 3, qi = sl * 16;
    const int kb = strips[2 * st + 1];
    const int k0 = kb * NB;
    const int r0 = strips[2 * st] * NB;
    const int rw = min(NB, n1 - r0);
    if (qi < rw) {
      lds_f64* const lds = (lds_f64*)smem;
      lds_f64 (*const Pcol)[NB] = (lds_f64 (*)[NB])lds;
      lds_f64 (*const Iv)[16][17] = (lds_f64 (*)[16][17])(lds + 16 * NB);
      lds_f64* const Id = lds + 16 * NB + 4 * 16 * 17;
      lds_f64* const Bm = Id + 16 * 16;
      lds_f64* const Li = Bm + NB * LP;
      const int kw = min(NB, n1 - k0);
      // this slice's 16 strip rows: in flight during the whole factorisation
      const int sr = tid >> 4, sc = 4 * (tid & 15);
      const double* src = S + (size_t)(r0 + min(qi + sr, rw - 1)) * ldS + k0 + sc;
      const double2 a0 = *reinterpret_cast<const double2*>(src), a1 = *reinterpret_cast<const double2*>(src + 2);
      {
        double2 v[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const int r = 8 * i + (tid >> 5), c = 2 * (tid & 31);
          v[i] = *reinterpret_cast<const double2*>(S + (size_t)(k0 + min(r, kw - 1)) * ldS + k0 + c);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const int r = 8 * i + (tid >> 5), c = 2 * (tid & 31);
          const bool in = r < kw;
          Bm[r * LP + c] = in ? v[i].x : (r == c ? 1.0 : 0.0);
          Bm[r * LP + c + 1] = in ? v[i].y : (r == c + 1 ? 1.0 : 0.0);
        }
      }
      Id[tid] = (tid >> 4) == (tid & 15) ? 1.0 : 0.0;
      __syncthreads();
      const DiagLds D = {Pcol, Iv, Id, Bm, Li};
      chol_diag_tile(D, fail);                    // (ends behind a barrier: Pcol / Iv are free)
      lds_f64* const Ai = lds;
      {
        const bool in = qi + sr < rw;
        Ai[sr * QP + sc] = in ? a0.x : 0.0; Ai[sr * QP + sc + 1] = in ? a0.y : 0.0;
        Ai[sr * QP + sc + 2] = in ? a1.x : 0.0; Ai[sr * QP + sc + 3] = in ? a1.y : 0.0;
      }
      __syncthreads();
      const int wave = tid >> 6, lane = tid & 63;
      const int wj = wave * 16;
      const int lr = lane & 15, lk = lane >> 4;
      double4_t acc = {0, 0, 0, 0};
      // X = A L^-T: column block `wave` of X needs the k-blocks 0..wave of L^-1 (the blocks above its diagonal were never written in
      // LDS; in the stored L^-1 they are zeros, so the products left out here are the exact zeros the two-launch form adds)
      for (int k = 0; k < 16 * (wave + 1); k += 4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ai[lr * QP + k + lk], Li[(wj + lr) * LP + k + lk], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = qi + lk + 4 * r, col = wj + lr;
        if (row < rw && col < kw) __hip_atomic_store(S + (size_t)(r0 + row) * ldS + k0 + col, acc[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) __hip_atomic_store(flags + 4 * (strip_base + st) + sl, gen_pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // L^-1 for the back substitution: the first slice of the column's first strip (a level lists a column's strips together)
      if (sl == 0 && (st == 0 || strips[2 * (st - 1) + 1] != kb)) {
        double* Lo = Linv_all + (size_t)kb * NB * NB;
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const int r = 8 * k + (tid >> 5), c = 2 * (tid & 31);
          const bool lower = (c >> 4) <= (r >> 4);
          const double2 v = lower ? make_double2(Li[r * LP + c], Li[r * LP + c + 1]) : make_double2(0.0, 0.0);
          *reinterpret_cast<double2*>(Lo + r * NB + c) = v;
        }
      }
      return;
    }
    if (tid == 0) __hip_atomic_store(flags + 4 * (strip_base + st) + sl, gen_pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if ((int)blockIdx.x < n_trsm) {
    double* Ai = smem;
    double* Li = smem + 16 * QP;
    const int st = blockIdx.x >> 2, sl = blockIdx.x & 3, qi = sl * 16;
    const int kb = strips[2 * st + 1];
    const int k0 = kb * NB;
    const int r0 = strips[2 * st] * NB;
    const int rw = min(NB, n1 - r0);
    if (qi < rw) {
      const double* Lk = Linv_all + (size_t)kb * NB * NB;
      {
        double2 l[8];
#pragma unroll
        for (int i = 0; i < 8; i++) l[i] = *reinterpret_cast<const double2*>(Lk + (8 * i + (tid >> 5)) * NB + 2 * (tid & 31));
        const int r = tid >> 4, c = 4 * (tid & 15);
        const double* src = S + (size_t)(r0 + min(qi + r, rw - 1)) * ldS + k0 + c;
        const double2 a0 = *reinterpret_cast<const double2*>(src), a1 = *reinterpret_cast<const double2*>(src + 2);
        const bool in = qi + r < rw;
        Ai[r * QP + c] = in ? a0.x : 0.0; Ai[r * QP + c + 1] = in ? a0.y : 0.0;
        Ai[r * QP + c + 2] = in ? a1.x : 0.0; Ai[r * QP + c + 3] = in ? a1.y : 0.0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
          Li[(8 * i + (tid >> 5)) * QP + 2 * (tid & 31)] = l[i].x;
          Li[(8 * i + (tid >> 5)) * QP + 2 * (tid & 31) + 1] = l[i].y;
        }
      }
      __syncthreads();
      const int wave = tid >> 6, lane = tid & 63;
      const int wj = wave * 16;
      const int lr = lane & 15, lk = lane >> 4;
      double4_t acc = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < NB; k += 4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ai[lr * QP + k + lk], Li[(wj + lr) * QP + k + lk], acc, 0, 0, 0);
      const int kw = min(NB, n1 - k0);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = qi + lk + 4 * r, col = wj + lr;
        if (row < rw && col < kw) __hip_atomic_store(S + (size_t)(r0 + row) * ldS + k0 + col, acc[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this thread's part of the slice has reached the coherence point
    }
    __syncthreads();
    if (tid == 0) __hip_atomic_store(flags + 4 * (strip_base + st) + sl, gen_pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // gen_pub == gen (debug switch: see the launcher)
    return;
  }
  double* Ai = smem;
  double* Aj = smem + 32 * QP;
  const int bx = blockIdx.x - n_trsm;
  const int tg = bx >> 2, qi = (bx & 2) * 16, qj = (bx & 1) * 32;
  const int ti = targets[4 * tg], tj = targets[4 * tg + 1];
  const int c0 = targets[4 * tg + 2], c1 = targets[4 * tg + 3];
  if (ti == tj && qj > qi) return;   // strictly upper quadrant of a diagonal tile
  const int i0 = ti * NB + qi, j0 = tj * NB + qj;
  const int iw = min(32, n1 - i0), jw = min(32, n1 - j0);
  const int wave = tid >> 6, lane = tid & 63;
  const int wi = (wave >> 1) * 16, wj = (wave & 1) * 16;
  double4_t acc = {0, 0, 0, 0};
  const int lr = lane & 15, lk = lane >> 4;
  const int pr = tid >> 6, pc = tid & 63;
  double tgt[4];                       // the target's own entries: nothing in this launch writes them, fetched before the wait
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = wi + lk + 4 * r, col = wj + lr;
    tgt[r] = (row < iw && col < jw && (i0 + row) >= (j0 + col)) ? S[(size_t)(i0 + row) * ldS + j0 + col] : 0.0;
  }
  // the slices this quadrant multiplies: rows [qi, qi + 32) of strip (ti, k) and rows [qj, qj + 32) of strip (tj, k) for every
  // contributing column k -- four flags per contributor, one lane each
  for (int f = tid; f < 4 * (c1 - c0); f += 256) {
    const int c = c0 + (f >> 2), side = (f >> 1) & 1, half = f & 1;
    const int32_t* flag = flags + 4 * contrib_strip[2 * c + side] + ((side ? qj : qi) >> 4) + half;
    for (int spins = 0; __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != gen; spins++) {
      __builtin_amdgcn_s_sleep(1);
      if (spins > (1 << 18)) { *fail = 2; break; }          // never hang the device: give up, the trial is rejected
    }
  }
  __syncthreads();
  double ra0[8], rb0[8], ra1[8], rb1[8], ra2[8], rb2[8];
  auto fetch = [&](int c, double* ra, double* rb) {
    const int k0 = contrib[c] * NB;
    const double* ga = S + (size_t)(i0 + pr) * ldS + k0 + pc;
    const double* gb = S + (size_t)(j0 + pr) * ldS + k0 + pc;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      ra[k] = (4 * k + pr < iw) ? __hip_atomic_load(ga + (size_t)4 * k * ldS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
      rb[k] = (4 * k + pr < jw) ? __hip_atomic_load(gb + (size_t)4 * k * ldS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    }
  };
  auto step = [&](int c, double* ra, double* rb) {
    if (c > c0) __syncthreads();          // the previous contributor's MFMAs have read Ai / Aj
#pragma unroll
    for (int k = 0; k < 8; k++) { Ai[(4 * k + pr) * QP + pc] = ra[k]; Aj[(4 * k + pr) * QP + pc] = rb[k]; }
    __syncthreads();
    if (c + 3 < c1) fetch(c + 3, ra, rb);
#pragma unroll
    for (int k = 0; k < NB; k += 4)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ai[(wi + lr) * QP + k + lk], Aj[(wj + lr) * QP + k + lk], acc, 0, 0, 0);
  };
  fetch(c0, ra0, rb0);
  if (c0 + 1 < c1) fetch(c0 + 1, ra1, rb1);
  if (c0 + 2 < c1) fetch(c0 + 2, ra2, rb2);
  for (int c = c0; c < c1; c += 3) {
    step(c, ra0, rb0);
    if (c + 1 < c1) step(c + 1, ra1, rb1);
    if (c + 2 < c1) step(c + 2, ra2, rb2);
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = wi + lk + 4 * r, col = wj + lr;
    if (row < iw && col < jw && (i0 + row) >= (j0 + col)) S[(size_t)(i0 + row) * ldS + j0 + col] = tgt[r] - acc[r];
  }
}

// Backward substitution L^T x = y (y = row n_pad of S) in PULL form, ALL tile columns in one launch:
//   x_k = Linv_kk^T (y_k - sum_{i in struct(k)} L(i,k)^T x_i);  the x_i belong to ancestors of k in the elimination tree.
// One workgroup per tile column.  A workgroup takes a ticket and processes the ticket-th column in root-first order, so
// every column it has to wait for is held by a workgroup that is already running (no deadlock whatever the dispatch
// order); x_i travels through `xrow` as 64 data-tagged words: the slots are filled with kXTag by the first solve launch of the
// factorisation, the producer overwrites them with 8-byte agent-scope (write-through) stores and every consumer lane waits
// for ITS word to change -- no flag, no drain in front of a flag (the back substitution of the BASELINE problem: 25.8 -> 20.7 us).
// Eight dependent launches of ~5 us each before (one per level) -> one launch with a ~2 us hop per level.
// The result goes to row space (xrow, for the descendants) and, compacted to dof doubles per unknown, to x.
__global__ void __launch_bounds__(256) k_chol_backsolve(const double* __restrict__ S, int ldS, int n_pad, int nfree, int per_tile, int dof,
                                                        const int32_t* __restrict__ cols, int ncols, const double* __restrict__ y,
                                                        double* __restrict__ xrow, double* __restrict__ x,
                                                        const double* __restrict__ Linv_all,
                                                        const int32_t* __restrict__ colstrip_off,
                                                        const int32_t* __restrict__ colstrips, int32_t* __restrict__ sync, int gen,
                                                        int* __restrict__ fail, int n_raw, int ncamt, int nkept, const int32_t* __restrict__ kept_list) {
  __shared__ double yk[NB];
  __shared__ double xi[NB];
  __shared__ double part[4][NB];
  __shared__ int s_col, s_ticket;
  const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
  if (tid == 0) {
    const int t = __hip_atomic_fetch_add(sync, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == ncols - 1) __hip_atomic_store(sync, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // every ticket is taken
    s_col = cols[ncols - 1 - t];     // `cols` lists leaves first
    s_ticket = t;
  }
  __syncthreads();
  const int kb = s_col;
  const int k0 = kb * NB;
  if (k0 >= n_pad) return;                       // the rhs tile itself (never in the list; defensive)
  if (tid < NB) yk[tid] = y[k0 + tid];
  // Everything that does not depend on an ancestor's x is fetched BEFORE waiting for it: this column's Linv tile and the
  // strip tile of the first dependency (then always the next strip's tile while the current one is waited for / applied);
  // the hop per level shrinks from flag + three dependent tile loads to flag + 64 doubles of x.
  const double* Lk = Linv_all + (size_t)kb * NB * NB;
  double lk[16];
#pragma unroll
  for (int r = 0; r < 16; r++) lk[r] = Lk[(16 * q + r) * NB + c];
  if (s_ticket < n_raw) {
    // a column of the last level: nothing but the rhs row hangs below it, and the factorisation left that row unsolved (the
    // launcher skipped the level's k_chol_trsm: 5 us for one 64 x 64 matrix-vector product per column) -- y_k = Linv_kk r here
    __shared__ double Pm[NB][NB + 1];
    __syncthreads();                               // yk (= r) is in LDS
#pragma unroll
    for (int r = 0; r < 16; r++) Pm[16 * q + r][c] = lk[r] * yk[c];
    __syncthreads();
    double s = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) s += Pm[c][16 * q + j];
    part[q][c] = s;
    __syncthreads();
    if (tid < NB) yk[tid] = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    __syncthreads();
  }
  const int s_beg = colstrip_off[kb], s_end = colstrip_off[kb + 1];
  double tl[16];
  auto fetch_tile = [&](int s) {
    const int i0 = colstrips[s] * NB;
    if (i0 >= n_pad) return;
#pragma unroll
    for (int r = 0; r < 16; r++) tl[r] = S[(size_t)(i0 + 16 * q + r) * ldS + k0 + c];
  };
  // (round 5: the ancestors nearest the ROOT first -- their x is the first to arrive; in ascending order the column's parent, whose x
  //  arrives last, blocked every other product behind it: ~16 us a hop on a column with 40 strips.  A changed summation order.)
  if (s_beg < s_end) fetch_tile(s_end - 1);
  for (int s = s_end - 1; s >= s_beg; s--) {
    const int it = colstrips[s], i0 = it * NB;
    if (i0 >= n_pad) { if (s > s_beg) fetch_tile(s - 1); continue; }   // the rhs row is not an unknown
    if (tid < NB) {   // every lane waits for its own word of x_i: the data is its own flag
      double v = __hip_atomic_load(xrow + i0 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int spins = 0; (unsigned long long)__double_as_longlong(v) == kXTag; spins++) {
        __builtin_amdgcn_s_sleep(1);
        if (spins > (1 << 22)) { *fail = 2; break; }     // never hang the device: give up, the trial is rejected
        v = __hip_atomic_load(xrow + i0 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      xi[tid] = v;
    }
    __syncthreads();
    double u = 0;
#pragma unroll
    for (int r = 0; r < 16; r++) u += tl[r] * xi[16 * q + r];
    if (s > s_beg) fetch_tile(s - 1);
    part[q][c] = u;
    __syncthreads();
    if (tid < NB) yk[tid] -= (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
  }
  __syncthreads();
  // (Linv^T y)[c] = sum_r Linv[r][c] y[r]  (Linv is zero above the diagonal); 4 row-quarters per column
  double s = 0;
#pragma unroll
  for (int r = 0; r < 16; r++) s += lk[r] * yk[16 * q + r];
  part[q][c] = s;
  __syncthreads();
  if (tid < NB) {   // one wave
    const double v = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    __hip_atomic_store(xrow + k0 + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // replaces the tag: the word is the hand-off
    // g2o's linear solver leaves _x untouched when the factorisation fails (linear_solver_eigen.h:89-112): x keeps the last
    // successful solve's values, which the LM loop then applies all the same (optimization_algorithm_levenberg.cpp:111-127)
    if (__hip_atomic_load(fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) write_x(x, kb, tid, v, nfree, per_tile, dof, ncamt, nkept, kept_list);
  }
}

// ----------------------------------------------------------------------------------------- flow
// The WHOLE reduced solve -- tile factorisation and back substitution -- as ONE persistent launch (round 5).  The level launches above pay a
// kernel boundary (or two) per elimination-tree level and run a level's trailing update to completion before the next diagonal tile
// starts; on a reduced system whose tree is a long chain (a loop-closed map: 37 levels at 500 keyframes) that is 43 us a level.  Here
// every structurally non-zero tile of a camera column is a TASK (BaTileSchedule::flow_tasks), taken by the workgroups through a ticket:
//   diagonal tile (k, k): gathers its updates LEFT-LOOKING -- tgt = S(k,k), then per level that updates it acc = sum over that level's
//     columns m of X(k,m) X(k,m)^T and tgt -= acc, the order and association of the level launches: same bits --, factorises
//     (chol_diag_tile) and publishes L_k^-1;
//   strip tile (i, k): gathers its updates the same way, waits for L_k^-1 and publishes X(i,k) = T L_k^-T in place;
//   then one task per camera column of the back substitution (k_chol_backsolve's body, root first).
// A task waits only for tasks BEFORE it in the list (a tile's contributors are columns of lower levels, its own diagonal tile is listed
// first, the back substitution comes last), so the workgroups that hold tickets always make progress: no residency assumption, no
// deadlock whatever else runs on the chip.  Hand-off: the payload is stored write-through (sc1: 16-byte buffer stores, or 8-byte
// agent-scope stores straight from the MFMA accumulators), drained by every storing wave, then ONE lane raises the tile's flag to the
// solve's sequence number; the consumer polls that word relaxed and reads the payload with sc1 loads (MI355X_MICROARCH.md, valid forms).
// What this buys: no kernel boundaries, and the trailing update of a column overlaps the factorisation of the next diagonal tile --
// the chain per level is [last contribution -> factorise -> L^-1 -> first strip], not [everything of the level].
#ifdef DVM_FLOW_DEBUG
// per task: [0] start, [1] gather done, [2] L^-1 there (strip) / tile in LDS (diagonal), [3] computed, [4] published, [5] wall-clock ticks
// thread 0 spent in flow_wait, [6] workgroup, [7] XCC id.  wall_clock64: 100 MHz.
__device__ long long g_flow_dbg[4096 * 8];
#define DVM_FSTMP(t, i) do { if (threadIdx.x == 0 && (t) < 4096) g_flow_dbg[(t) * 8 + (i)] = (long long)wall_clock64(); } while (0)
extern "C" int dvm_debug_flow_stamps(long long* out, int n) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_flow_dbg), sizeof(long long) * (size_t)n); }
#else
#define DVM_FSTMP(t, i) do { } while (0)
#endif
// k_chol_flow's hook into the factorisation (chol_diag_tile): the gathered chain strip T(p, k) into LDS under the last panel
struct FlowTHook {
  static constexpr bool on = true;
  const int32_t* flags;        // the two "half gathered" words of the chain strip (null: no chain parent)
  int gen;
  __amdgpu_buffer_rsrc_t rS;
  int toff, ldS;               // byte offset of the tile in S
  double* Xb;                  // LDS, pitch QP
  int* s_flag;                 // LDS word: 1 = the tile is (being) loaded
  int* fv;                     // the look's register (per thread)
  typedef unsigned int v4u32_ __attribute__((ext_vector_type(4)));
  // begin (waves 1..3, top of the last panel): wave 3 issues the loads of the strip's two flags
  __device__ __forceinline__ void begin() {
    *fv = gen;
    if (flags && threadIdx.x >= 192 && threadIdx.x < 194) *fv = __hip_atomic_load(flags + (threadIdx.x - 192), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // end (behind their own work there): wave 3 says whether both halves are gathered (LDS word: 2 = not decided yet, 0 / 1); the three
  // waves then move the tile, 2048 chunks of 16 bytes over 192 threads, global -> registers -> LDS
  __device__ __forceinline__ void end() {
    if (threadIdx.x >= 192) {
      const bool ok = __all(*fv == gen) && flags != nullptr;
      if (threadIdx.x == 192) *reinterpret_cast<volatile int*>(s_flag) = ok ? 1 : 0;
    }
    int f;
    while ((f = *reinterpret_cast<volatile int*>(s_flag)) == 2) __builtin_amdgcn_s_sleep(1);
    if (f == 0) return;
    const int q0 = (int)threadIdx.x - 64;
    v4u32_ v[11];
#pragma unroll
    for (int j = 0; j < 11; j++) {
      const int q = min(q0 + 192 * j, 2047);
      v[j] = __builtin_amdgcn_raw_buffer_load_b128(rS, toff + (int)(((size_t)(q >> 5) * ldS + 2 * (q & 31)) * 8), 0, 16);
    }
#pragma unroll
    for (int j = 0; j < 11; j++) {
      const int q = q0 + 192 * j;
      if (q < 2048) {
        double2 d;
        d.x = __hiloint2double((int)v[j].y, (int)v[j].x); d.y = __hiloint2double((int)v[j].w, (int)v[j].z);
        *reinterpret_cast<double2*>(Xb + (q >> 5) * 66 + 2 * (q & 31)) = d;
      }
    }
  }
};
struct FlowArgs {
  double* S; int ldS, n1, n_pad;
  double* Linv_all;
  const int32_t *tasks, *fc, *colinfo;
  int n_factor, n_back;
  int32_t* flags; int nstrips, ntiles;
  int gen, gen_pub; int* fail;            // gen_pub == gen (test switch DVM_BA_DEBUG_BREAK_FLOW: X flags nobody waits for)
  const int32_t* cols; double* xrow; double* x;
  const int32_t *colstrip_off, *colstrips, *colstrip_id;
  int nfree, per_tile, dof;
  int ncamt, nkept; const int32_t* kept_list;
};
typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));
// bounded wait of ONE lane for a word to reach the solve's sequence number; a timeout marks the trial (fail = 2: the host repeats it with
// the level launches) and lets everybody run out: once the mark is up nobody waits any more
__device__ __forceinline__ void flow_wait_raw(const int32_t* flag, int gen, int* __restrict__ fail) {
  for (int spins = 0; __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != gen; spins++) {
    __builtin_amdgcn_s_sleep(1);
    if ((spins & 255) == 255 && __hip_atomic_load(fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 2) return;
    if (spins > (1 << 19)) { __hip_atomic_store(fail, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
  }
}
#ifdef DVM_FLOW_DEBUG
__device__ __forceinline__ void flow_wait_dbg(const int32_t* flag, int gen, int* __restrict__ fail, long long* wacc) {
  const long long w0 = (long long)wall_clock64();
  flow_wait_raw(flag, gen, fail);
  *wacc += (long long)wall_clock64() - w0;
}
#define flow_wait(f, g, x) flow_wait_dbg(f, g, x, &s_wacc)
#else
#define flow_wait(f, g, x) flow_wait_raw(f, g, x)
#endif
__device__ __forceinline__ double2 u4_to_d2(v4u32 v) {
  return make_double2(__hiloint2double((int)v.y, (int)v.x), __hiloint2double((int)v.w, (int)v.z));
}
__device__ __forceinline__ v4u32 d2_to_u4(double a, double b) {
  return v4u32{(unsigned)__double2loint(a), (unsigned)__double2hiint(a), (unsigned)__double2loint(b), (unsigned)__double2hiint(b)};
}
// One contributor's products for the NS blocks a wave owns: acc[s] += A_s B_s^T over the 64 columns of the strips in LDS.  Branch-free and
// unrolled by 16 columns with the operands of a chunk read before its MFMAs, so that the LDS latency of chunk n + 1 sits under the matrix
// pipe of chunk n (with a test per slot inside the loop the compiler read, waited and multiplied one block at a time: ~2.5x the pipe time).
template <int NS, bool SHARE_B>
__device__ __forceinline__ void flow_mma(const double* __restrict__ Ai, const double* __restrict__ Bp, const int (&arow)[3], const int (&brow)[3], int lr, int lk,
                                         double4_t (&acc)[3]) {
  const double* pa[NS];
  const double* pb[NS];
#pragma unroll
  for (int s = 0; s < NS; s++) { pa[s] = Ai + (arow[s] + lr) * QP + lk; pb[s] = Bp + (brow[s] + lr) * QP + lk; }
#pragma unroll
  for (int kk = 0; kk < NB; kk += 16) {
    double a[NS][4], b[NS][4];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int s = 0; s < NS; s++) {
        a[s][j] = pa[s][kk + 4 * j];
        if (!SHARE_B || s == 0) b[s][j] = pb[s][kk + 4 * j];
      }
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int s = 0; s < NS; s++) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][j], b[SHARE_B ? 0 : s][j], acc[s], 0, 0, 0);
  }
}
__global__ void __launch_bounds__(256) k_chol_flow(FlowArgs A) {
  constexpr int kCholLds = 16 * NB + 4 * 16 * 17 + 16 * 16 + 2 * NB * LP;      // the factorisation's block (also the gather buffers Ai / Aj)
  __shared__ __attribute__((aligned(16))) double smem[kCholLds + NB * QP];     // + the chain strip T -> X (119 KB: one workgroup per CU either way)
  __shared__ int s_ticket, s_ready[2];
#ifdef DVM_FLOW_DEBUG
  __shared__ long long s_wacc;
#endif
  static_assert(2 * NB * QP <= 16 * NB + 4 * 16 * 17 + 16 * 16 + 2 * NB * LP, "the gather buffers live inside the factorisation's LDS block");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int ldS = A.ldS;
  const int F_L = 2 * A.nstrips, F_P = F_L + A.ntiles, F_T = F_P + A.ntiles;      // flag spaces: X halves | L^-1 | PRE | gathered halves of chain strips
  int32_t* const tagged = A.flags + F_T + 2 * A.nstrips;
  int32_t* const ticket = tagged + 1;
  const int ntotal = A.n_factor + A.n_back;
  // buffer descriptors (wave-uniform inputs only): S and the L^-1 tiles, for the 16-byte sc1 loads / stores
  const auto rS = __builtin_amdgcn_make_buffer_rsrc(A.S, 0, (int)min((size_t)ldS * ldS * sizeof(double), (size_t)0x7FFFFFF0), 0x00020000);
  const auto rL = __builtin_amdgcn_make_buffer_rsrc(A.Linv_all, 0, (int)((size_t)A.ntiles * NB * NB * sizeof(double)), 0x00020000);
  double* const Ai = smem;
  double* const Aj = smem + NB * QP;
  const int crow = tid >> 5, ccol = 2 * (tid & 31);      // 16-byte chunk of a 64-double row: instruction i covers rows 8 i + crow
  for (;;) {
    __syncthreads();                       // the previous task is through with the LDS block and s_ticket
    if (tid == 0) {
      const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (t == ntotal + (int)gridDim.x - 1) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the last draw of the launch: every workgroup draws one ticket beyond the list
      s_ticket = t;
    }
    __syncthreads();
    const int t = s_ticket;
    if (t >= ntotal) return;
#ifdef DVM_FLOW_DEBUG
    if (tid == 0) s_wacc = 0;
    if (tid == 0 && t < 4096) g_flow_dbg[t * 8 + 7] = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15;   // (XCC_ID register: best effort)
#endif
    DVM_FSTMP(t, 0);
    if (t == 0) {
      // the back substitution's hand-off slots: tags (write-through), published before anybody may poll them
      for (int i = tid; i < A.n_pad; i += 256) __hip_atomic_store(reinterpret_cast<unsigned long long*>(A.xrow) + i, kXTag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) __hip_atomic_store(tagged, A.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (t < A.n_factor) {
      // ------------------------------------------------------------------------------------------ a tile (or half tile) of the factor
      const int32_t* T = A.tasks + 8 * (size_t)t;
      const int kind = T[0], ti = T[1], tj = T[2], half = T[3], c0 = T[4], c1 = T[5], self = T[6];
      const bool slice = kind == 1 || kind == 4;
      const int i0 = ti * NB + (slice ? 32 * half : 0), j0 = tj * NB;
      const int rw = min(slice ? 32 : NB, A.n1 - i0);      // rows of the region that exist (the rhs row: one)
#ifdef DVM_FLOW_DEBUG
      if (tid == 0 && t < 4096) g_flow_dbg[t * 8 + 6] = (long long)blockIdx.x | ((long long)kind << 12) | ((long long)ti << 16) | ((long long)tj << 32) | ((long long)(c1 - c0) << 48);
#endif
      // the 16x16 blocks this wave owns (slot s): a slice -- column block `wave` of its two block rows; a diagonal tile -- its ten lower
      // blocks dealt 3 3 2 2.  arow / brow: first row of the block's A / B operand in the LDS buffers (= the block's position in the region)
      int arow[3], brow[3];
      bool son[3];
#pragma unroll
      for (int s = 0; s < 3; s++) {
        if (slice) { arow[s] = 16 * s; brow[s] = 16 * wave; son[s] = s < 2 && 16 * s < rw; }
        else {
          const int b = wave < 2 ? 3 * wave + s : 6 + 2 * (wave - 2) + s;          // index into the row-major list of lower blocks
          son[s] = wave < 2 || s < 2;
          const int bi = b < 1 ? 0 : b < 3 ? 1 : b < 6 ? 2 : 3;
          arow[s] = 16 * bi; brow[s] = 16 * (b - bi * (bi + 1) / 2);
        }
      }
      double4_t tgt[3], acc[3];
#pragma unroll
      for (int s = 0; s < 3; s++) {
        acc[s] = double4_t{0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = arow[s] + lk + 4 * r, col = brow[s] + lr;
          const double* p = A.S + (size_t)(i0 + min(row, rw - 1)) * ldS + j0 + col;
          tgt[s][r] = (son[s] && row < rw) ? *p : 0.0;
        }
      }
      // ---- gather: three contributors in flight (global -> registers), one in LDS under the matrix pipe.  A contributor's three flags
      // (its A half, both halves of B) are looked at by three lanes at once, and the look for contributor c + 3 is issued before step
      // c's products and read behind them: a poll is a ~1 us trip to the coherence point, which three in a row on one lane in front of
      // a barrier put on every step (4.4 us a contributor measured, 1.3 us of it matrix pipe).
      v4u32 g0[12], g1[12], g2[12];
      bool l0 = false, l1 = false, l2 = false;
      int rc = 0;
      auto flag_of = [&](int c, int f) -> const int32_t* {      // f = 0: the A operand's half; 1, 2: the halves of B
        const int32_t* e = A.fc + 4 * (size_t)c;
        return f == 0 ? A.flags + 2 * e[1] + (slice ? half : 0) : A.flags + 2 * e[2] + (f - 1);
      };
      auto wait_block = [&](int c) {
        if (tid < 3) flow_wait(flag_of(c, tid), A.gen, A.fail);
        __syncthreads();
      };
      auto fetch = [&](int c, v4u32 (&g)[12]) {
        const int m0 = A.fc[4 * (size_t)c] * NB;
        if (slice) {
#pragma unroll
          for (int i = 0; i < 4; i++) g[i] = __builtin_amdgcn_raw_buffer_load_b128(rS, (int)(((size_t)(i0 + min(8 * i + crow, rw - 1)) * ldS + m0 + ccol) * 8), 0, 16);
#pragma unroll
          for (int i = 0; i < 8; i++) g[4 + i] = __builtin_amdgcn_raw_buffer_load_b128(rS, (int)(((size_t)(j0 + 8 * i + crow) * ldS + m0 + ccol) * 8), 0, 16);
        } else {
#pragma unroll
          for (int i = 0; i < 8; i++) g[i] = __builtin_amdgcn_raw_buffer_load_b128(rS, (int)(((size_t)(i0 + 8 * i + crow) * ldS + m0 + ccol) * 8), 0, 16);
        }
      };
      // chk: the step before this one looked at the flags of contributor c + 2 (result in s_ready): its loads go into that step's registers (gp)
      auto step = [&](int c, v4u32 (&g)[12], bool& l, v4u32 (&gp)[12], bool& lp, bool chk) {
        if (!l) { wait_block(c); fetch(c, g); }
        __syncthreads();                   // the product before this one has read Ai / Aj (and s_ready is written)
        if (chk) { lp = s_ready[(rc - 1) & 1] != 0; if (lp) fetch(c + 2, gp); }
        if (slice) {
#pragma unroll
          for (int i = 0; i < 4; i++) *reinterpret_cast<double2*>(Ai + (8 * i + crow) * QP + ccol) = 8 * i + crow < rw ? u4_to_d2(g[i]) : make_double2(0.0, 0.0);
#pragma unroll
          for (int i = 0; i < 8; i++) *reinterpret_cast<double2*>(Aj + (8 * i + crow) * QP + ccol) = u4_to_d2(g[4 + i]);
        } else {
#pragma unroll
          for (int i = 0; i < 8; i++) *reinterpret_cast<double2*>(Ai + (8 * i + crow) * QP + ccol) = u4_to_d2(g[i]);
        }
        const bool look = c + 3 < c1;
        int fv = A.gen;
        if (look && tid < 3) fv = __hip_atomic_load(flag_of(c + 3, tid), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        // (wave-uniform choice of the straight-line form: a slice owns two blocks with one B operand -- the rhs row: one --, a diagonal
        //  tile three or two blocks a wave)
        if (slice) { if (son[1]) flow_mma<2, true>(Ai, Aj, arow, brow, lr, lk, acc); else flow_mma<1, true>(Ai, Aj, arow, brow, lr, lk, acc); }
        else if (son[2]) flow_mma<3, false>(Ai, Ai, arow, brow, lr, lk, acc);
        else flow_mma<2, false>(Ai, Ai, arow, brow, lr, lk, acc);
        if (look) {
          if (wave == 0) { const bool ok = __all(fv == A.gen); if (tid == 0) s_ready[rc & 1] = ok ? 1 : 0; }
          rc++;
        }
        if (A.fc[4 * (size_t)c + 3]) {     // the level's last contributor: the level launch subtracts its sum here
#pragma unroll
          for (int s = 0; s < 3; s++) { tgt[s] -= acc[s]; acc[s] = double4_t{0, 0, 0, 0}; }
        }
      };
      {
        // the first three contributors: nine flags, nine lanes, one look
        int fv = A.gen;
        if (tid < 9 && c0 + tid / 3 < c1) fv = __hip_atomic_load(flag_of(c0 + tid / 3, tid % 3), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (wave == 0) {
          const unsigned long long bad = __ballot(fv != A.gen);
          if (tid == 0) { s_ready[0] = (int)(bad & 0x1FF); }
        }
        __syncthreads();
        const int bad = s_ready[0];
        __syncthreads();
        l0 = c0 < c1 && (bad & 7) == 0; l1 = c0 + 1 < c1 && (bad & 0x38) == 0; l2 = c0 + 2 < c1 && (bad & 0x1C0) == 0;
        if (l0) fetch(c0, g0);
        if (l1) fetch(c0 + 1, g1);
        if (l2) fetch(c0 + 2, g2);
      }
      {
        bool chk = false;
        for (int c = c0; c < c1; c += 3) {
          step(c, g0, l0, g2, l2, chk); chk = c + 3 < c1;
          if (c + 1 < c1) { step(c + 1, g1, l1, g0, l0, chk); chk = c + 4 < c1; }
          if (c + 2 < c1) { step(c + 2, g2, l2, g1, l1, chk); chk = c + 5 < c1; }
        }
      }
      if (c0 < c1) __syncthreads();        // everybody is through with Ai / Aj
      DVM_FSTMP(t, 1);
      if (kind == 4) {
        // ---- a half of a chain strip: T in place (the chain's workgroup solves it), flag
#pragma unroll
        for (int s = 0; s < 2; s++)
          if (son[s]) {
#pragma unroll
            for (int r = 0; r < 4; r++) Ai[(arow[s] + lk + 4 * r) * QP + brow[s] + lr] = tgt[s][r];
          }
        __syncthreads();
        DVM_FSTMP(t, 2);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int r = 8 * i + crow;
          if (r < rw) __builtin_amdgcn_raw_buffer_store_b128(d2_to_u4(Ai[r * QP + ccol], Ai[r * QP + ccol + 1]), rS, (int)(((size_t)(i0 + r) * ldS + j0 + ccol) * 8), 0, 16);
        }
        DVM_FSTMP(t, 3);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_store(A.flags + F_T + 2 * self + half, A.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else if (slice) {
        // ---- X = T L^-T (block (bi, bj) needs the k-blocks 0..bj of L^-1: it is lower triangular), published in place, flag
#pragma unroll
        for (int s = 0; s < 2; s++)
          if (son[s]) {
#pragma unroll
            for (int r = 0; r < 4; r++) Ai[(arow[s] + lk + 4 * r) * QP + brow[s] + lr] = tgt[s][r];
          }
        if (tid == 0) flow_wait(A.flags + F_L + tj, A.gen, A.fail);
        __syncthreads();
        DVM_FSTMP(t, 2);
#pragma unroll
        for (int i = 0; i < 8; i++) g0[i] = __builtin_amdgcn_raw_buffer_load_b128(rL, (int)(((size_t)tj * NB * NB + (8 * i + crow) * NB + ccol) * 8), 0, 16);
#pragma unroll
        for (int i = 0; i < 8; i++) *reinterpret_cast<double2*>(Aj + (8 * i + crow) * QP + ccol) = u4_to_d2(g0[i]);
        __syncthreads();
        // the eight blocks cost 4 (bj + 1) MFMAs each: dealt so that every wave issues 20 -- waves 0, 1: column blocks 3 and 0 of block
        // row `wave`; waves 2, 3: column blocks 2 and 1 of block row `wave - 2`
        const int xbi = wave & 1, xbj0 = wave < 2 ? 3 : 2, xbj1 = wave < 2 ? 0 : 1;
        double4_t x0 = {0, 0, 0, 0}, x1 = {0, 0, 0, 0};
        if (16 * xbi < rw) {
          for (int kk = 0; kk < 16 * (xbj0 + 1); kk += 4)
            x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(Ai[(16 * xbi + lr) * QP + kk + lk], Aj[(16 * xbj0 + lr) * QP + kk + lk], x0, 0, 0, 0);
          for (int kk = 0; kk < 16 * (xbj1 + 1); kk += 4)
            x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(Ai[(16 * xbi + lr) * QP + kk + lk], Aj[(16 * xbj1 + lr) * QP + kk + lk], x1, 0, 0, 0);
        }
        __syncthreads();                   // T has been read: X takes its place (staging for the 16-byte stores)
        if (16 * xbi < rw) {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            Ai[(16 * xbi + lk + 4 * r) * QP + 16 * xbj0 + lr] = x0[r];
            Ai[(16 * xbi + lk + 4 * r) * QP + 16 * xbj1 + lr] = x1[r];
          }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int r = 8 * i + crow;
          if (r < rw) __builtin_amdgcn_raw_buffer_store_b128(d2_to_u4(Ai[r * QP + ccol], Ai[r * QP + ccol + 1]), rS, (int)(((size_t)(i0 + r) * ldS + j0 + ccol) * 8), 0, 16);
        }
        DVM_FSTMP(t, 3);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // every storing wave drains before the flag
        __syncthreads();
        if (tid == 0) __hip_atomic_store(A.flags + 2 * self + half, A.gen_pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else if (kind == 2) {
        // ---- PRE: the sum of the levels before the last one back in place (lower blocks), flag
#pragma unroll
        for (int s = 0; s < 3; s++)
          if (son[s]) {
#pragma unroll
            for (int r = 0; r < 4; r++) Ai[(arow[s] + lk + 4 * r) * QP + brow[s] + lr] = tgt[s][r];
          }
        __syncthreads();
        DVM_FSTMP(t, 2);
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const int r = 8 * i + crow;
          if ((ccol >> 4) <= (r >> 4)) __builtin_amdgcn_raw_buffer_store_b128(d2_to_u4(Ai[r * QP + ccol], Ai[r * QP + ccol + 1]), rS, (int)(((size_t)(i0 + r) * ldS + j0 + ccol) * 8), 0, 16);
        }
        DVM_FSTMP(t, 3);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_store(A.flags + F_P + tj, A.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        // ---- DIAG: a leaf's diagonal tile (no contributor: tgt = S), and then UP THE TREE along the chain: factorise k; solve the chain
        // strip (p, k) with the L_k^-1 that is in LDS; publish L_k^-1 and X(p, k); take what PRE left of (p, p), add X X^T -- the last
        // contributor of p's last level --, subtract; k = p.  (The factor of a diagonal tile itself is not written back, as in k_chol_diag.)
        lds_f64* const lds = (lds_f64*)smem;
        lds_f64 (*const Pcol)[NB] = (lds_f64 (*)[NB])lds;
        lds_f64 (*const Iv)[16][17] = (lds_f64 (*)[16][17])(lds + 16 * NB);
        lds_f64* const Id = lds + 16 * NB + 4 * 16 * 17;
        lds_f64* const Bm = Id + 16 * 16;
        lds_f64* const Li = Bm + NB * LP;
        double* const Xb = smem + kCholLds;   // T -> X of the chain strip, pitch QP
        int k = tj;
        for (;;) {
          const int p = A.colinfo[8 * k], cstrip = A.colinfo[8 * k + 1];
#pragma unroll
          for (int s = 0; s < 3; s++)
            if (son[s]) {
#pragma unroll
              for (int r = 0; r < 4; r++) Bm[(arow[s] + lk + 4 * r) * LP + brow[s] + lr] = tgt[s][r];
            }
          Id[tid] = (tid >> 4) == (tid & 15) ? 1.0 : 0.0;
          if (tid == 0) s_ready[0] = 2;     // (the hook's word: not decided yet)
          __syncthreads();
          v4u32 tq[8];
          const int toff = p >= 0 ? (int)(((size_t)p * NB * ldS + (size_t)k * NB) * 8) : 0;
          DVM_FSTMP(3500 + k, 0);
          // the chain strip T(p, k): its two halves are looked at from INSIDE the factorisation (wave 3, beside the last panel), and if
          // they are there the tile travels into Xb under that panel and the tail
          int hook_fv = 0;
          FlowTHook hook;
          hook.flags = p >= 0 ? A.flags + F_T + 2 * cstrip : nullptr; hook.gen = A.gen; hook.rS = rS; hook.toff = toff; hook.ldS = ldS;
          hook.Xb = Xb; hook.s_flag = &s_ready[0]; hook.fv = &hook_fv;
          const DiagLds D = {Pcol, Iv, Id, Bm, Li};
          chol_diag_tile(D, A.fail, hook);
          const bool tpre = s_ready[0] == 1;
#ifdef DVM_FLOW_DEBUG
          if (tid == 0) g_flow_dbg[(3500 + k) * 8 + 6] = tpre ? 1 : 0;
#endif
          DVM_FSTMP(3500 + k, 1);
          const bool fold_root = p < 0 && A.colinfo[8 * k + 5] != 0;
          if (!fold_root) {
#pragma unroll
            for (int q = 0; q < 8; q++) {
              const int r = 8 * q + crow;
              const bool lower = (ccol >> 4) <= (r >> 4);      // the blocks above the diagonal were never written in LDS: zeros from here
              __builtin_amdgcn_raw_buffer_store_b128(d2_to_u4(lower ? Li[r * LP + ccol] : 0.0, lower ? Li[r * LP + ccol + 1] : 0.0), rL, (int)(((size_t)k * NB * NB + r * NB + ccol) * 8), 0, 16);
            }
          }
          if (fold_root) {
            // a ROOT column (only the rhs row hangs below it): nobody else needs its factor.  y = L^-1 r and x = L^-T y right here, from
            // the L^-1 in LDS -- the sums of k_chol_backsolve's n_raw branch and of its last step, term for term (the blocks of L^-1 above
            // the diagonal, never written in LDS, are the zeros the stored tile has)
            double* const yk = Xb;
            double* const part = Xb + NB;
            if (tid == 0) flow_wait(A.flags + F_T + 2 * cstrip, A.gen, A.fail);
            __syncthreads();
            const int c = tid & 63, q = tid >> 6, k0 = k * NB;
            if (tid < NB) yk[tid] = __hip_atomic_load(A.S + (size_t)A.n_pad * ldS + k0 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            double sy = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) sy += (q <= (c >> 4) ? Li[c * LP + 16 * q + j] : 0.0) * yk[16 * q + j];
            part[q * NB + c] = sy;
            __syncthreads();
            if (tid < NB) yk[tid] = (part[tid] + part[NB + tid]) + (part[2 * NB + tid] + part[3 * NB + tid]);
            __syncthreads();
            double sx = 0;
#pragma unroll
            for (int r = 0; r < 16; r++) sx += ((c >> 4) <= q ? Li[(16 * q + r) * LP + c] : 0.0) * yk[16 * q + r];
            __syncthreads();
            part[q * NB + c] = sx;
            __syncthreads();
            if (tid < NB) {
              const double v = (part[tid] + part[NB + tid]) + (part[2 * NB + tid] + part[3 * NB + tid]);
              __hip_atomic_store(A.xrow + k0 + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              if (__hip_atomic_load(A.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) write_x(A.x, k, tid, v, A.nfree, A.per_tile, A.dof, A.ncamt, A.nkept, A.kept_list);
            }
            DVM_FSTMP(3500 + k, 4);
            break;
          }
          // L_k^-1 is what this column's other strips wait for: out at once (drain, flag), whatever the chain waits for next
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __syncthreads();
          if (tid == 0) __hip_atomic_store(A.flags + F_L + k, A.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (p < 0) break;                // the chain ends here (the root, or a column that is not its parent's last contributor)
          if (!tpre) {
            if (tid < 2) flow_wait(A.flags + F_T + 2 * cstrip + tid, A.gen, A.fail);
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 8; i++) tq[i] = __builtin_amdgcn_raw_buffer_load_b128(rS, toff + (int)(((size_t)(8 * i + crow) * ldS + ccol) * 8), 0, 16);
#pragma unroll
            for (int i = 0; i < 8; i++) *reinterpret_cast<double2*>(Xb + (8 * i + crow) * QP + ccol) = u4_to_d2(tq[i]);
          }
          const bool cont = A.colinfo[8 * k + 6] != 0;          // k is p's chain child: this workgroup goes on to p
          const int pmode = A.colinfo[8 * p + 2], lc0 = A.colinfo[8 * p + 3], lc1 = A.colinfo[8 * p + 4];
          if (cont && pmode >= 2 && tid == 0) flow_wait(A.flags + F_P + p, A.gen, A.fail);      // (long there: PRE runs levels ahead)
          __syncthreads();
          // what PRE left of (p, p): on its way while the strip is solved
          const int pi0 = p * NB;
#pragma unroll
          for (int s = 0; s < 3; s++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
              const int row = arow[s] + lk + 4 * r, col = brow[s] + lr;
              const double* q = A.S + (size_t)(pi0 + row) * ldS + pi0 + col;
              tgt[s][r] = (!son[s] || !cont) ? 0.0 : pmode >= 2 ? __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *q;
              acc[s][r] = 0.0;
            }
          }
          DVM_FSTMP(3500 + k, 2);
          // X = T L_k^-T: wave w takes block row w (4 + 8 + 12 + 16 MFMAs: L^-1 is lower triangular)
          double4_t xr[4];
#pragma unroll
          for (int bj = 0; bj < 4; bj++) {
            double4_t x4 = {0, 0, 0, 0};
#pragma unroll
            for (int kk = 0; kk < 16 * (bj + 1); kk += 4)
              x4 = __builtin_amdgcn_mfma_f64_16x16x4f64(Xb[(16 * wave + lr) * QP + kk + lk], Li[(16 * bj + lr) * LP + kk + lk], x4, 0, 0, 0);
            xr[bj] = x4;
          }
          __syncthreads();                 // T has been read: X takes its place
#pragma unroll
          for (int bj = 0; bj < 4; bj++)
#pragma unroll
            for (int r = 0; r < 4; r++) Xb[(16 * wave + lk + 4 * r) * QP + 16 * bj + lr] = xr[bj][r];
          __syncthreads();
#pragma unroll
          for (int i = 0; i < 8; i++) {
            const int r = 8 * i + crow;
            __builtin_amdgcn_raw_buffer_store_b128(d2_to_u4(Xb[r * QP + ccol], Xb[r * QP + ccol + 1]), rS, toff + (int)(((size_t)r * ldS + ccol) * 8), 0, 16);
          }
          DVM_FSTMP(3500 + k, 3);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // X has left (every storing wave): its flags go up before anything else --
          __syncthreads();                                     // the next chain strip's gather is waiting for them
          if (tid < 2) __hip_atomic_store(A.flags + 2 * cstrip + tid, A.gen_pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (!cont) break;     // not the parent's chain child: the parent belongs to a sibling's workgroup, which gathers this strip
          // p's other children (the contributors of its last level before the chain child, ascending): their strips (p, m) come from
          // memory like any gathered contributor, one at a time -- there are one or two
          for (int c = lc0; c < lc1; c++) {
            const int32_t* e = A.fc + 4 * (size_t)c;
            if (tid < 2) flow_wait(A.flags + 2 * e[1] + tid, A.gen, A.fail);
            __syncthreads();               // (also: the product before this one has read Ai)
#pragma unroll
            for (int i = 0; i < 8; i++) tq[i] = __builtin_amdgcn_raw_buffer_load_b128(rS, (int)(((size_t)(pi0 + 8 * i + crow) * ldS + (size_t)e[0] * NB + ccol) * 8), 0, 16);
#pragma unroll
            for (int i = 0; i < 8; i++) *reinterpret_cast<double2*>(Ai + (8 * i + crow) * QP + ccol) = u4_to_d2(tq[i]);
            __syncthreads();
            if (son[2]) flow_mma<3, false>(Ai, Ai, arow, brow, lr, lk, acc);
            else flow_mma<2, false>(Ai, Ai, arow, brow, lr, lk, acc);
          }
          // the chain child's product, the last of p's last level: acc += X X^T, tgt -= acc
          if (son[2]) flow_mma<3, false>(Xb, Xb, arow, brow, lr, lk, acc);
          else flow_mma<2, false>(Xb, Xb, arow, brow, lr, lk, acc);
#pragma unroll
          for (int s = 0; s < 3; s++) { tgt[s] -= acc[s]; acc[s] = double4_t{0, 0, 0, 0}; }
          __syncthreads();                 // Xb / Ai have been read: Bm may be written
          DVM_FSTMP(3500 + k, 4);
          k = p;
        }
      }
      DVM_FSTMP(t, 4);
#ifdef DVM_FLOW_DEBUG
      if (tid == 0 && t < 4096) g_flow_dbg[t * 8 + 5] = s_wacc;
#endif
      continue;
    }
    // -------------------------------------------------------------------------------------------- back substitution of one column
    {
      double* const yk = smem;                 // [NB]
      double* const xi = smem + NB;            // [NB]
      double (*const part)[NB] = (double (*)[NB])(smem + 2 * NB);   // [4][NB]
      const int c = tid & 63, q = tid >> 6;
      const int kb = A.cols[A.n_back - 1 - (t - A.n_factor)];      // `cols` lists leaves first
      const int k0 = kb * NB;
      if (A.colinfo[8 * kb + 5]) continue;      // a root column: solved by the chain's workgroup the moment it was factored
      const int s_beg = A.colstrip_off[kb], s_end = A.colstrip_off[kb + 1];
#ifdef DVM_FLOW_DEBUG
      if (tid == 0 && t < 4096) g_flow_dbg[t * 8 + 6] = (long long)blockIdx.x | (3ll << 12) | ((long long)kb << 16);
#endif
      // one lane per flag: the column's L^-1, the tags, and both halves of each of its strips (the rhs row: one half)
      if (tid == 0) flow_wait(tagged, A.gen, A.fail);
      if (tid == 1) flow_wait(A.flags + F_L + kb, A.gen, A.fail);
      for (int f = tid; f < 2 * (s_end - s_beg); f += 256) {
        const int s = s_beg + (f >> 1);
        if ((f & 1) == 0 || A.colstrips[s] * NB < A.n_pad) flow_wait(A.flags + 2 * A.colstrip_id[s] + (f & 1), A.gen, A.fail);
      }
      __syncthreads();
      DVM_FSTMP(t, 1);
      auto ld = [](const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
      if (tid < NB) yk[tid] = ld(A.S + (size_t)A.n_pad * ldS + k0 + tid);
      const double* Lk = A.Linv_all + (size_t)kb * NB * NB;
      double lkk[16];
#pragma unroll
      for (int r = 0; r < 16; r++) lkk[r] = ld(Lk + (16 * q + r) * NB + c);
      double tl[16];
      auto fetch_tile = [&](int s) {
        const int r0 = A.colstrips[s] * NB;
        if (r0 >= A.n_pad) return;
#pragma unroll
        for (int r = 0; r < 16; r++) tl[r] = ld(A.S + (size_t)(r0 + 16 * q + r) * ldS + k0 + c);
      };
      // ancestors nearest the root first: their x is the first to arrive, the parent's the last (see k_chol_backsolve)
      if (s_beg < s_end) fetch_tile(s_end - 1);
      for (int s = s_end - 1; s >= s_beg; s--) {
        const int r0 = A.colstrips[s] * NB;
        if (r0 >= A.n_pad) { if (s > s_beg) fetch_tile(s - 1); continue; }   // the rhs row is not an unknown
        if (tid < NB) {   // every lane waits for its own word of x_i: the data is its own flag
          double v = ld(A.xrow + r0 + tid);
          for (int spins = 0; (unsigned long long)__double_as_longlong(v) == kXTag; spins++) {
            __builtin_amdgcn_s_sleep(1);
            if (spins > (1 << 19) || ((spins & 255) == 255 && __hip_atomic_load(A.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 2)) {
              __hip_atomic_store(A.fail, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              break;
            }
            v = ld(A.xrow + r0 + tid);
          }
          xi[tid] = v;
        }
        __syncthreads();
        double u = 0;
#pragma unroll
        for (int r = 0; r < 16; r++) u += tl[r] * xi[16 * q + r];
        if (s > s_beg) fetch_tile(s - 1);
        part[q][c] = u;
        __syncthreads();
        if (tid < NB) yk[tid] -= (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
      }
      __syncthreads();
      double sum = 0;
#pragma unroll
      for (int r = 0; r < 16; r++) sum += lkk[r] * yk[16 * q + r];
      part[q][c] = sum;
      __syncthreads();
      if (tid < NB) {
        const double v = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
        __hip_atomic_store(A.xrow + k0 + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // replaces the tag: the word is the hand-off
        // (g2o's linear solver leaves _x untouched when the factorisation fails: see k_chol_backsolve)
        if (__hip_atomic_load(A.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) write_x(A.x, kb, tid, v, A.nfree, A.per_tile, A.dof, A.ncamt, A.nkept, A.kept_list);
      }
      DVM_FSTMP(t, 4);
    }
  }
}

constexpr int kDiagLevelMaxWGs = 256;    // k_chol_trsm_update<true>: 86 KB of LDS, one workgroup per CU
constexpr int kFusedLevelMaxWGs = 512;   // 2 workgroups per CU on 256 CUs (3 fit: 41 KB of LDS each); the leaf level of the BASELINE problem (536) measured the same fused or not
void tile_launch_cholesky_solve(hipStream_t s, const TileSystem& T, int* d_fail, int solve_seq, TileSolveTrace* trace) {
  if (trace) *trace = TileSolveTrace{};
  if (T.nfree == 0) return;
  const int n1 = T.n_pad + 1;
  if (trace) trace->nlevels = std::min<int>(T.nlevels, TileSolveTrace::kMaxLevels);
  auto took = [&](int h, TileLevelPath p) { if (trace && h < TileSolveTrace::kMaxLevels) trace->path[h] = p; };
  if (T.flow && T.flow_tasks && T.flow_flags) {     // the whole solve as one persistent launch of tile tasks (k_chol_flow)
    FlowArgs A;
    A.S = T.S; A.ldS = T.ldS; A.n1 = n1; A.n_pad = T.n_pad; A.Linv_all = T.Linv;
    A.tasks = T.flow_tasks; A.fc = T.flow_contrib; A.colinfo = T.flow_col;
    A.n_factor = T.n_flow_tasks; A.n_back = T.h_level_off[T.nlevels - 1];
    A.flags = T.flow_flags; A.nstrips = T.n_strips_total; A.ntiles = T.n_tiles_total;
    // test switch: the strips publish a sequence number nobody waits for, so every wait on them gives up (bounded), the trial is marked
    // (fail = 2) and the caller repeats it with one launch per phase (tests/test_gpu_ba_flow.py)
    static const bool break_flow = std::getenv("DVM_BA_DEBUG_BREAK_FLOW") != nullptr;
    A.gen = solve_seq; A.gen_pub = break_flow ? -1 : solve_seq; A.fail = d_fail;
    A.cols = T.cols; A.xrow = T.xrow; A.x = T.x; A.colstrip_off = T.colstrip_off; A.colstrips = T.colstrips; A.colstrip_id = T.colstrip_id;
    A.nfree = T.nfree; A.per_tile = T.per_tile; A.dof = T.dof; A.ncamt = T.ncamt; A.nkept = T.nkept; A.kept_list = T.kept_list;
    const int wgs = std::max(1, std::min(A.n_factor + A.n_back, T.flow_wgs > 0 ? T.flow_wgs : 256));
    hipLaunchKernelGGL(k_chol_flow, dim3(wgs), dim3(256), 0, s, A);
    if (trace) trace->flow = 1;
    return;
  }
  // test switch: the slices publish a sequence number nobody waits for, so every wait times out and the caller's retry path
  // (one launch per phase) has to produce the result (tests/test_gpu_ba.py)
  static const bool break_handoff = std::getenv("DVM_BA_DEBUG_BREAK_HANDOFF") != nullptr;
  const bool diag_in_level = T.diag_in_level != 0;   // (A/B switch DVM_BA_NO_DIAG_IN_LEVEL, read by dvm_ba_set_problem)
  double* tag = T.xrow;   // the first launch that solves strips also re-arms the back substitution's hand-off slots (no strips: no waits)
  int root_level = T.nlevels - 1;          // the last level that is launched (see the break below), where n_root_raw applies
  if (root_level >= 1 && T.h_level_off[root_level + 1] - T.h_level_off[root_level] == 1 && T.h_strip_off[root_level + 1] == T.h_strip_off[root_level] &&
      T.h_tgt_off[root_level + 1] == T.h_tgt_off[root_level]) root_level--;
  // the top pair of the elimination order (two single-column levels: root_level - 1 and root_level) goes to k_chol_pair
  const bool pair = T.pair_ok && root_level >= 1;
  for (int h = 0; h < T.nlevels; h++) {
    if (pair && h == root_level - 1) break;
    const int nc = T.h_level_off[h + 1] - T.h_level_off[h], ns = T.h_strip_off[h + 1] - T.h_strip_off[h];
    const int nt = T.h_tgt_off[h + 1] - T.h_tgt_off[h];
    // the root of the elimination tree is the tile of the augmented rhs row: its "factorisation" (one scalar) is never
    // used -- row n_pad already holds y = L^-1 b once the last camera level is done -- so that level is not launched
    if (h == T.nlevels - 1 && nc == 1 && ns == 0 && nt == 0) break;
    const bool raw_root = ns > 0 && nt == 0 && T.n_root_raw > 0 && h == root_level;   // the back substitution solves these rhs strips itself
    // the whole level -- factorisation of the diagonal tiles included -- as one launch (k_chol_trsm_update<true>): one workgroup
    // per CU, so only while slices + quadrants fit the chip at once; else the slices alone that way and the update behind them
    const bool all = nt > 0 && 4 * (ns + nt) <= kDiagLevelMaxWGs;
    if (diag_in_level && !raw_root && ns > 0 && T.contrib_strip && T.strip_flags && 4 * ns <= kDiagLevelMaxWGs) {
      hipLaunchKernelGGL(k_chol_trsm_update<true>, dim3(4 * (ns + (all ? nt : 0))), dim3(256), 0, s, T.S, T.ldS, n1, T.Linv,
                         T.strips + 2 * (size_t)T.h_strip_off[h], T.h_strip_off[h], 4 * ns, T.targets + 4 * (size_t)T.h_tgt_off[h], T.contrib,
                         T.contrib_strip, T.strip_flags, solve_seq, break_handoff ? -1 : solve_seq, d_fail, tag, T.n_pad);
      tag = nullptr;
      if (nt > 0 && !all) hipLaunchKernelGGL(k_chol_update, dim3(4 * nt), dim3(256), 0, s, T.S, T.ldS, n1, T.targets + 4 * (size_t)T.h_tgt_off[h], T.contrib);
      took(h, all ? kPathLevelOneLaunch : kPathSlicesDiagUpdate);
      continue;
    }
    hipLaunchKernelGGL(k_chol_diag, dim3(nc), dim3(256), 0, s, T.S, T.ldS, n1, T.cols + T.h_level_off[h], d_fail, T.Linv);
    // solve + update of the level as ONE launch when every workgroup of it is resident at once (a quadrant then never waits
    // for a slice that has no compute unit to run on): 41 KB of LDS per workgroup = 3 per CU
    if (ns > 0 && nt > 0 && 4 * (ns + nt) <= kFusedLevelMaxWGs && T.contrib_strip && T.strip_flags) {
      hipLaunchKernelGGL(k_chol_trsm_update<false>, dim3(4 * (ns + nt)), dim3(256), 0, s, T.S, T.ldS, n1, T.Linv, T.strips + 2 * (size_t)T.h_strip_off[h],
                         T.h_strip_off[h], 4 * ns, T.targets + 4 * (size_t)T.h_tgt_off[h], T.contrib, T.contrib_strip, T.strip_flags, solve_seq,
                         break_handoff ? -1 : solve_seq, d_fail, tag, T.n_pad);
      tag = nullptr;
      took(h, kPathDiagFused);
      continue;
    }
    took(h, raw_root ? kPathRawRoot : kPathDiagTrsmUpdate);
    if (raw_root) continue;
    if (ns > 0) { hipLaunchKernelGGL(k_chol_trsm, dim3(4 * ns), dim3(256), 0, s, T.S, T.ldS, n1, T.Linv, T.strips + 2 * (size_t)T.h_strip_off[h], tag, T.n_pad); tag = nullptr; }
    if (nt > 0) hipLaunchKernelGGL(k_chol_update, dim3(4 * nt), dim3(256), 0, s, T.S, T.ldS, n1, T.targets + 4 * (size_t)T.h_tgt_off[h], T.contrib);
  }
  // y = L^-1 b is row n_pad of S (the augmented rhs row): the back substitution reads it in place; one launch for all
  // camera tile columns (levels 0 .. nlevels - 2; level nlevels - 1 is the rhs tile alone: not an unknown)
  int ncols = T.h_level_off[T.nlevels - 1];
  int n_raw = T.n_root_raw;
  if (pair) {
    // (the slots of xrow that the remaining columns wait on were tagged by the first strip launch above; these two are written for good)
    hipLaunchKernelGGL(k_chol_pair, dim3(1), dim3(256), 0, s, T.S, T.ldS, T.n_pad, T.pair_a, T.pair_b, T.nfree, T.per_tile, T.dof, T.xrow, T.x, d_fail, T.ncamt, T.nkept, T.kept_list);
    ncols -= 2;          // `cols` lists the levels in order: the pair's columns are its last two entries
    n_raw = 0;
    if (trace) trace->pair = 1;
  }
  if (trace) trace->backsolve_cols = std::max(ncols, 0);
  if (ncols > 0)
    hipLaunchKernelGGL(k_chol_backsolve, dim3(ncols), dim3(256), 0, s, T.S, T.ldS, T.n_pad, T.nfree, T.per_tile, T.dof, T.cols, ncols,
                       T.S + (size_t)T.n_pad * T.ldS, T.xrow, T.x, T.Linv, T.colstrip_off, T.colstrips, reinterpret_cast<int32_t*>(T.ytmp),
                       solve_seq, d_fail, n_raw, T.ncamt, T.nkept, T.kept_list);
}

}  // namespace dvm
