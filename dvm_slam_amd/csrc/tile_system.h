// dvm_slam_amd/csrc/tile_system.h -- the tiled reduced system and its solve (kernels + launcher: chol_kernels.hip).
//
// A symmetric positive definite system in 64-row tiles, lower triangle, with the right-hand side as an augmented row: what the bundle
// adjustment's Schur complement (ba_kernels.hip) and the pose graph's normal equations (pg_kernels.hip) write, and what the sparse tile
// Cholesky factors and solves.  Whoever sets a system up (ba_solver.cpp, pg_solver.cpp) fills the members from a BaTileSchedule (ba_ordering.h);
// a member left at zero / null switches the form of the solve it belongs to off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dvm {

// first row of camera i (elimination order) in the tiled reduced system: 10 whole cameras per 64-row tile
__host__ __device__ inline int ba_row(int i) { return (i / 10) * 64 + (i % 10) * 6; }

struct TileSystem {
  // ---- matrix and solution.  Unknown block i (elimination order, ba_ordering.h) owns rows (i / per_tile) * 64 + (i % per_tile) * dof (cameras:
  // ba_row(i)); the rows of a tile behind its blocks are identity padding; n_pad = 64 * tiles of unknowns; row n_pad carries the right-hand
  // side (augmented row), so ldS = n_pad + 64.
  double* S;                // [ldS][ldS] dense lower triangle + augmented rhs row
  int32_t ldS, n_pad;
  int32_t per_tile, dof;    // unknown blocks per 64-row tile and their size: (10, 6) cameras, (9, 7) Sim3 vertices
  double* x;                // the solution, compact: [dof * nfree], behind it 3 per landmark (bundle adjustment: [6*nfree + 3*L])
  double* xrow;             // [n_pad] solution in row space (back substitution reads its ancestors here)
  double* Linv;             // [ldS/64][64*64] inverses of the factored diagonal blocks
  double* ytmp;             // [n_pad + 64] doubles, used as int32 words: [0] ticket, [1 + k] hand-off flag of tile column k
                            // of the one-launch back substitution; must be zeroed once after allocation
  // ---- structure
  const int32_t* nz_tiles;  // (i, j) pairs of the structurally non-zero tiles (n_nz of them): cleared before every trial
  int32_t n_nz;
  // level schedule of the tile Cholesky (columns of one elimination-tree height are independent):
  const int32_t* cols;      // columns by level                                  (host offsets h_level_off)
  const int32_t* strips;    // (row tile, column) pairs by level                 (h_strip_off)
  const int32_t* targets;   // (ti, tj, c0, c1) trailing tiles by level          (h_tgt_off)
  const int32_t* contrib;   // contributing columns of each target, ascending
  const int32_t* contrib_strip;  // per contribution: indices (into strips) of the two strips it multiplies
  const int32_t* colstrip_off;  // [ntiles+1] device
  const int32_t* colstrips;     // per column: its strip rows
  const int32_t* colstrip_id;   // per colstrips entry: index of that strip
  int32_t nlevels;
  const int32_t *h_level_off, *h_strip_off, *h_tgt_off;  // HOST arrays [nlevels+1]
  // ---- in-launch hand-offs
  int32_t* strip_flags;     // [4 * strips]: hand-off flag of every 16-row slice of a strip (k_chol_trsm_update); zeroed once after
                            // allocation, compared with the solve's sequence number like the back substitution's flags
  // ---- FLOW form of the solve (k_chol_flow, ba_ordering.h): tile tasks taken through a ticket, factorisation + back substitution in ONE launch
  const int32_t* flow_tasks;    // [n_flow_tasks][8]
  const int32_t* flow_contrib;  // [..][4] flattened contributor lists (ba_ordering.h)
  const int32_t* flow_col;      // [tiles][8] chain links and diagonal-tile modes (ba_ordering.h)
  int32_t* flow_flags;          // [2 x strips] a 32-row half of X published | [tiles] L^-1 of a column | [tiles] T' of a diagonal tile (PRE) | [2 x strips] a
                                // half of a chain strip gathered | xrow tagged | ticket; compared with the solve's sequence number, zeroed once after allocation
  int32_t n_flow_tasks, n_strips_total, n_tiles_total;
  int32_t flow;                 // 1: tile_launch_cholesky_solve uses k_chol_flow (set by dvm_ba_set_problem; 0 after one of its waits timed out)
  int32_t flow_wgs;             // persistent workgroups to launch (compute units of the device)
  // ---- choices
  int32_t pair_a, pair_b;   // tile columns of the top pair (ba_ordering.h: BaTileSchedule::pair_a / pair_b) and pair_ok = 1, or pair_ok = 0
  int32_t pair_ok;
  int32_t diag_in_level;    // levels of <= 256 slice workgroups factor their diagonal tiles inside k_chol_trsm_update<true> (0: DVM_BA_NO_DIAG_IN_LEVEL)
  int32_t n_root_raw;       // columns of the last launched level whose only strip is the rhs row: their panel solve (one 64x64
                            // matrix-vector product each) is done by the back substitution itself, no k_chol_trsm launch (0: launch it)
  // ---- where solutions land.  The first ncamt tiles hold the nfree unknown blocks; a bundle adjustment's KEPT LANDMARKS (ba_kernels.h)
  // follow, 21 to a tile (3 x 21 rows + one of padding): kept landmark j = landmark kept_list[j], whose x is written behind the cameras'.
  int32_t nfree;            // unknown blocks
  int32_t ncamt, nkept;
  const int32_t* kept_list; // [nkept]
};

// Factorisation and solve of T on stream s: x (and xrow) hold the solution afterwards, *d_fail != 0 reports a non-positive pivot (x then
// keeps what it held) or, = 2, a hand-off wait that gave up (the caller repeats the trial with T.flow = 0 / T.strip_flags = null).
// solve_seq: a number > 0 that differs from call to call on this system (the hand-off flags compare against it)
void tile_launch_cholesky_solve(hipStream_t s, const TileSystem& T, int* d_fail, int solve_seq);

}  // namespace dvm
