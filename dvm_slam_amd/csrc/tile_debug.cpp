// dvm_slam_amd/csrc/tile_debug.cpp -- test hooks of the tile Cholesky (dvm_tile_solve_debug, dvm_tile_schedule_debug).
//
// A caller-given linear system goes through the solver exactly as the bundle adjustment and the pose graph hand theirs over: ba_tile_schedule
// on the tile mask, tile_system_fill (ba_solver.cpp) for the TileSystem, S written as the builders leave it, tile_launch_cholesky_solve.  No
// edge, camera or Levenberg-Marquardt step is involved; the form of the solve is chosen by argument, never by the environment.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/dvmslam_hip.h"
#include "ba_ordering.h"
#include "chain.h"
#include "orb_pipeline.h"  // set_error / hip_check / DVM_HIP
#include "tile_system.h"

using namespace dvm;

static_assert(kPathNone == DVM_TILE_PATH_NONE && kPathLevelOneLaunch == DVM_TILE_PATH_LEVEL_ONE_LAUNCH && kPathSlicesDiagUpdate == DVM_TILE_PATH_SLICES_DIAG_UPDATE &&
              kPathDiagFused == DVM_TILE_PATH_DIAG_FUSED && kPathDiagTrsmUpdate == DVM_TILE_PATH_DIAG_TRSM_UPDATE && kPathRawRoot == DVM_TILE_PATH_RAW_ROOT,
              "TileLevelPath (tile_system.h) and DVM_TILE_PATH_* (dvmslam_hip.h) name the same paths");

namespace {
struct DevPool final : TileArena {
  std::vector<void*> ptrs;
  ~DevPool() { for (void* p : ptrs) hipFree(p); }
  int alloc(void** p, size_t bytes) override {
    *p = nullptr;
    const int rc = hip_check(hipMalloc(p, std::max<size_t>(bytes, 1)), "hipMalloc(tile debug)");
    if (*p) ptrs.push_back(*p);
    return rc;
  }
  int upload(const void** p, const void* src, size_t bytes) override {
    void* q = nullptr;
    int rc = alloc(&q, bytes);
    if (rc == DVM_OK && bytes) rc = hip_check(hipMemcpy(q, src, bytes, hipMemcpyHostToDevice), "upload(tile debug)");
    *p = q;
    return rc;
  }
};

// schedule of a mask over the tiles of unknowns (lower triangle read); the tile of the augmented rhs row is added here
BaTileSchedule schedule_of(const std::vector<uint8_t>& mask, int nt) {
  std::vector<std::vector<char>> T(nt + 1, std::vector<char>(nt + 1, 0));
  for (int i = 0; i < nt; i++)
    for (int j = 0; j <= i; j++) T[i][j] = mask[(size_t)i * nt + j] ? 1 : 0;
  return ba_tile_schedule(T);
}

void describe(const BaTileSchedule& SC, int nt, int workgroups, dvm_tile_solve_info* info) {
  std::memset(info, 0, sizeof(*info));
  info->n_tiles = nt; info->levels = SC.nlevels; info->pair_a = SC.pair_a; info->pair_b = SC.pair_b; info->n_root_raw = SC.n_root_raw;
  info->flow_leaves = SC.flow_leaves; info->flow_tasks = (int32_t)(SC.flow_tasks.size() / 8);
  for (size_t k = 0; k + 1 < SC.flow_col.size() / 8; k++) info->roots += SC.flow_col[8 * k] < 0;
  info->flow_refusal = tile_flow_refusal(SC, 64 * SC.ntiles, workgroups);
  for (int h = 0; h < std::min(SC.nlevels, 64); h++) {
    info->level_nc[h] = SC.level_off[h + 1] - SC.level_off[h];
    info->level_ns[h] = SC.strip_off[h + 1] - SC.strip_off[h];
    info->level_nt[h] = SC.tgt_off[h + 1] - SC.tgt_off[h];
  }
}
}  // namespace

extern "C" int dvm_tile_schedule_debug(int n_tiles, const uint8_t* mask, int workgroups, dvm_tile_solve_info* info) {
  if (n_tiles < 1 || n_tiles > 256 || !mask || workgroups < 1 || !info) { set_error("dvm_tile_schedule_debug: bad arguments"); return DVM_ERR_INVALID; }
  const std::vector<uint8_t> m(mask, mask + (size_t)n_tiles * n_tiles);
  describe(schedule_of(m, n_tiles), n_tiles, workgroups, info);
  return DVM_OK;
}

extern "C" int dvm_tile_solve_debug(int device, int n_blocks, int dof, int per_tile, int n_kept, const int32_t* kept_list, int n_landmarks,
                                    const double* A, const double* b, const uint8_t* mask, const double* x_in, int form, int repeats,
                                    const double* A2, const double* b2, double* x, int32_t* fail, double* x2, int32_t* fail2,
                                    dvm_tile_solve_info* info) {
  const int all_forms = DVM_TILE_FORM_FLOW | DVM_TILE_FORM_NO_PAIR | DVM_TILE_FORM_NO_DIAG_IN_LEVEL | DVM_TILE_FORM_NO_ROOT_RAW | DVM_TILE_FORM_PER_PHASE;
  if (n_blocks < 1 || !((dof == 6 && per_tile == kCamsPerTile) || (dof == 7 && per_tile == kSim3PerTile)) || n_kept < 0 || n_landmarks < n_kept ||
      (n_kept > 0 && !kept_list) || !A || !b || !x_in || !x || !fail || !info || (form & ~all_forms) || repeats < 1 || repeats > 8 || (!A2) != (!b2)) {
    set_error("dvm_tile_solve_debug: bad arguments");
    return DVM_ERR_INVALID;
  }
  {
    std::vector<char> seen(n_landmarks, 0);    // every kept landmark writes its own three words of x
    for (int j = 0; j < n_kept; j++) {
      if (kept_list[j] < 0 || kept_list[j] >= n_landmarks || seen[kept_list[j]]) { set_error("dvm_tile_solve_debug: kept_list out of range or repeated"); return DVM_ERR_INVALID; }
      seen[kept_list[j]] = 1;
    }
  }
  const int ncamt = (n_blocks + per_tile - 1) / per_tile, nt = ncamt + (n_kept + 20) / 21;
  const size_t n = (size_t)dof * n_blocks + 3 * (size_t)n_kept, x_len = (size_t)dof * n_blocks + 3 * (size_t)n_landmarks;
  // unknown row -> row of the tiled system
  std::vector<int32_t> row(n);
  for (size_t r = 0; r < (size_t)dof * n_blocks; r++) row[r] = (int32_t)((r / dof / per_tile) * 64 + (r / dof % per_tile) * dof + r % dof);
  for (size_t r = 0; r < 3 * (size_t)n_kept; r++) row[(size_t)dof * n_blocks + r] = (int32_t)((ncamt + r / 63) * 64 + r % 63);
  // the tile mask: the caller's, which every non-zero of the systems must respect, or the non-zeros of A (and A2)
  std::vector<uint8_t> m((size_t)nt * nt, 0);
  if (mask) m.assign(mask, mask + (size_t)nt * nt);
  for (const double* M : {A, A2}) {
    if (!M) continue;
    for (size_t i = 0; i < n; i++)
      for (size_t j = 0; j <= i; j++) {
        if (M[i * n + j] == 0.0) continue;
        uint8_t& t = m[(size_t)(row[i] / 64) * nt + row[j] / 64];
        if (!t && mask) { set_error("dvm_tile_solve_debug: a non-zero of the matrix outside the tile mask"); return DVM_ERR_INVALID; }
        t = 1;
      }
  }
  int ndev = 0;
  { const int rc = need_any_device(&ndev); if (rc != DVM_OK) return rc; }
  if (device < 0 || device >= ndev) return DVM_ERR_INVALID;
  DVM_HIP(hipSetDevice(device));

  const BaTileSchedule SC = schedule_of(m, nt);
  DevPool D;
  TileSystem T{};
  int32_t why = 0;
  {
    const int rc = tile_system_fill(D, device, T, SC, n_blocks, per_tile, dof, ncamt, kept_list, n_kept, x_len, &why);
    if (rc != DVM_OK) return rc;
  }
  describe(SC, nt, T.flow_wgs, info);
  // the form, member by member
  if (form & DVM_TILE_FORM_FLOW) {
    if (why & (kFlowTooLarge | kFlowSeveralRoots | kFlowTooManyLeaves)) { set_error("dvm_tile_solve_debug: the flow form does not admit this system"); return DVM_ERR_INVALID; }
    T.flow = 1;
  } else {
    T.flow = 0;
  }
  T.pair_ok = SC.pair_a >= 0 && !(form & DVM_TILE_FORM_NO_PAIR);
  T.diag_in_level = !(form & DVM_TILE_FORM_NO_DIAG_IN_LEVEL);
  T.n_root_raw = (form & DVM_TILE_FORM_NO_ROOT_RAW) ? 0 : SC.n_root_raw;
  if (form & DVM_TILE_FORM_PER_PHASE) { T.strip_flags = nullptr; T.contrib_strip = nullptr; }

  // S as the builders leave it: zeros, the lower triangle of the matrix, identity on the padding rows, b in row n_pad, the corner that
  // keeps the last pivot positive
  const size_t ld = (size_t)T.ldS;
  auto image = [&](const double* M, const double* rhs) {
    std::vector<double> S(ld * ld, 0.0);
    for (size_t i = 0; i < n; i++)
      for (size_t j = 0; j <= i; j++) S[(size_t)row[i] * ld + row[j]] = M[i * n + j];
    std::vector<char> used((size_t)T.n_pad, 0);
    for (size_t i = 0; i < n; i++) used[row[i]] = 1;
    for (size_t r = 0; r < (size_t)T.n_pad; r++) if (!used[r]) S[r * ld + r] = 1.0;
    for (size_t i = 0; i < n; i++) S[(size_t)T.n_pad * ld + row[i]] = rhs[i];
    S[(size_t)T.n_pad * ld + T.n_pad] = 1e200;
    return S;
  };
  const std::vector<double> S1 = image(A, b), S2 = A2 ? image(A2, b2) : std::vector<double>();
  int* d_fail = nullptr;
  { void* p = nullptr; const int rc = D.alloc(&p, sizeof(int)); if (rc != DVM_OK) return rc; d_fail = static_cast<int*>(p); }
  DVM_HIP(tile_system_zero_flags(nullptr, T));
  int seq = 0;
  TileSolveTrace tr{};
  auto solve = [&](const std::vector<double>& S, double* x_out, int32_t* fail_out, TileSolveTrace* trace) {
    DVM_HIP(hipMemcpy(T.S, S.data(), S.size() * sizeof(double), hipMemcpyHostToDevice));
    DVM_HIP(hipMemcpy(T.x, x_in, x_len * sizeof(double), hipMemcpyHostToDevice));
    DVM_HIP(hipMemset(d_fail, 0, sizeof(int)));
    tile_launch_cholesky_solve(nullptr, T, d_fail, ++seq, trace);
    DVM_HIP(hipGetLastError());
    DVM_HIP(hipDeviceSynchronize());
    if (x_out) DVM_HIP(hipMemcpy(x_out, T.x, x_len * sizeof(double), hipMemcpyDeviceToHost));
    if (fail_out) { int f = 0; DVM_HIP(hipMemcpy(&f, d_fail, sizeof(int), hipMemcpyDeviceToHost)); *fail_out = f; }
    return (int)DVM_OK;
  };
  for (int r = 0; r < repeats; r++) {
    { const int rc = solve(S1, x + (size_t)r * x_len, fail + r, r == 0 ? &tr : nullptr); if (rc != DVM_OK) return rc; }
    if (A2 && r + 1 < repeats) { const int rc = solve(S2, x2 ? x2 + (size_t)r * x_len : nullptr, fail2 ? fail2 + r : nullptr, nullptr); if (rc != DVM_OK) return rc; }
  }
  info->traced_levels = tr.nlevels; info->used_pair = tr.pair; info->used_flow = tr.flow; info->backsolve_cols = tr.backsolve_cols;
  for (int h = 0; h < tr.nlevels; h++) info->level_path[h] = tr.path[h];
  return DVM_OK;
}
