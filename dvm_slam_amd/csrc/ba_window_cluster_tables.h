// dvm_slam_amd/csrc/ba_window_cluster_tables.h -- the index tables of the cluster form of the window optimizer (ba_window_cluster.hip).
// Pure host code, no HIP: checked on the CPU against a brute-force restatement (tools/check_ba_window_tables.cpp, run by
// tests/test_host_logic.py).  Packing the tables into page-locked memory is the launcher's (ClusterBuild::pack_fast).
#pragma once
#include <algorithm>
#include <utility>

#include "ba_window_common.h"

namespace dvm {

constexpr int kLpPitch = 9;            // pitch of win_cholesky_rhs's panel copy, (n + 1) rows: part of the LDS a window asks for

struct ClusterTables {
  WinGraph g;                          // (its e_* arrays leave build_window_fast in the camera-major order)
  int F = 0, nblk = 0, Fp = 0, stage_doubles = 0;     // rows of free cameras, blocks, F rounded up to 64 (the rows' pitch), LDS doubles behind the control words
  std::vector<int32_t> pt_start, f_cam, blk_ij;       // [nact + 1] a landmark's range of pt_edges, [F] free camera of the row, [nblk] i1 | i2 << 8
  std::vector<int32_t> e_orig, e_lm, cam_start, pt_edges, bp_start, bp_pairs;   // (layouts: ClusterWin); bp_pairs: (row1, row2) interleaved
  int cluster_waves = 8;              // 8 G: set by the call before the build (the Schur pass's schedule is per wave of the cluster)
  std::vector<int32_t> sched_start, sched_task;
  // scratch of build_window_fast, kept with the object: a pooled build touches no fresh pages from its second use on (32 windows
  // built by 16 threads spent 2.3 ms of a 9 ms call in the page faults of their ~2 MB of vectors each)
  std::vector<int32_t> t_by_lm, t_ep, t_ept, t_cnt, t_blk_of, t_cr, t_fill;
  std::vector<double> t_eo, t_ei;
};

// The cluster form's structure: edges sorted camera-major (free cameras in free-index order, a camera's edges by landmark, then the fixed
// cameras' edges), per landmark its edges in that order, per block of the reduced system its (row, row) pairs in landmark order
// (block_solver.hpp:381-439: edge k1 (outer) x edge k2 (inner), lower blocks; (k1, k1) on the diagonal).  b may have been used before.
// obs: see win_graph -- the per-edge measurements are then not the host's: e_obs / e_info stay empty, the gather kernel goes through e_orig.
inline int build_window_fast(const dvm_ba_window& w, ClusterTables& b, const dvm_ba_obs* obs = nullptr) {
  WinGraph& g = b.g;
  const int rc = win_graph(w, /*normalize=*/true, &g, obs);
  if (rc != DVM_OK) return rc;
  b.blk_ij.clear();
  const int E = g.E, nf = g.nfree, P = g.P;
  // rank of an edge's camera: free index, or nf + pose for a fixed camera; two stable counting sorts: by landmark, then by rank
  std::vector<int32_t>& by_lm = b.t_by_lm; std::vector<int32_t>& order = b.e_orig;
  by_lm.resize(E); order.resize(E);
  {
    std::vector<int32_t>& cnt = b.t_cnt;
    cnt.assign(g.nact + 1, 0);
    for (int k = 0; k < E; k++) cnt[g.lidx[g.e_point[k]] + 1]++;
    for (int i = 0; i < g.nact; i++) cnt[i + 1] += cnt[i];
    for (int k = 0; k < E; k++) by_lm[cnt[g.lidx[g.e_point[k]]]++] = k;
    std::vector<int32_t>& cr = b.t_cr;
    cr.assign(nf + P + 1, 0);
    auto rank = [&](int k) { const int i = g.pidx[g.e_pose[k]]; return i >= 0 ? i : nf + g.e_pose[k]; };
    for (int k = 0; k < E; k++) cr[rank(k) + 1]++;
    for (int i = 0; i < nf + P; i++) cr[i + 1] += cr[i];
    b.cam_start.assign(cr.begin(), cr.begin() + nf + 1);
    for (int j = 0; j < E; j++) { const int k = by_lm[j]; order[cr[rank(k)]++] = k; }
  }
  b.F = nf ? b.cam_start[nf] : 0;
  b.Fp = (b.F + 63) & ~63;
  std::vector<int32_t>& ep = b.t_ep; std::vector<int32_t>& ept = b.t_ept;
  std::vector<double>& eo = b.t_eo; std::vector<double>& ei = b.t_ei;
  ep.resize(E); ept.resize(E); eo.resize(obs ? 0 : 2 * (size_t)E); ei.resize(obs ? 0 : E);
  b.e_lm.resize(E);
  for (int j = 0; j < E; j++) {
    const int k = order[j];
    ep[j] = g.e_pose[k]; ept[j] = g.e_point[k];
    if (!obs) { eo[2 * (size_t)j] = g.e_obs[2 * (size_t)k]; eo[2 * (size_t)j + 1] = g.e_obs[2 * (size_t)k + 1]; ei[j] = g.e_info[k]; }
    b.e_lm[j] = g.lidx[ept[j]];
  }
  g.e_pose.swap(ep); g.e_point.swap(ept); g.e_obs.swap(eo); g.e_info.swap(ei);
  b.f_cam.resize(b.F);
  for (int i = 0; i < nf; i++) for (int j = b.cam_start[i]; j < b.cam_start[i + 1]; j++) b.f_cam[j] = i;
  // a landmark's edges, ascending sorted index (its free rows first)
  b.pt_start.assign(g.nact + 1, 0);
  for (int j = 0; j < E; j++) b.pt_start[b.e_lm[j] + 1]++;
  for (int i = 0; i < g.nact; i++) b.pt_start[i + 1] += b.pt_start[i];
  b.pt_edges.resize(E);
  { std::vector<int32_t>& fill = b.t_fill;
    fill.assign(b.pt_start.begin(), b.pt_start.end() - 1);
    for (int j = 0; j < E; j++) b.pt_edges[fill[b.e_lm[j]]++] = j; }
  // blocks and their pairs.  Within a landmark the free rows ascend with the camera: (q1, q2) with camera(q2) <= camera(q1) is q2 <= q1,
  // minus the off-diagonal pairs of two observations by the SAME camera (as the sequential-order form leaves them out)
  std::vector<int32_t>& blk_of = b.t_blk_of; std::vector<int32_t>& cnt = b.t_cnt;
  blk_of.assign((size_t)nf * nf, -1); cnt.clear();
  auto each_pair = [&](auto&& fn) {
    for (int li = 0; li < g.nact; li++) {
      const int q0 = b.pt_start[li];
      int qe = q0;
      while (qe < b.pt_start[li + 1] && b.pt_edges[qe] < b.F) qe++;
      for (int a1 = q0; a1 < qe; a1++)
        for (int a2 = q0; a2 <= a1; a2++) {
          const int r1 = b.pt_edges[a1], r2 = b.pt_edges[a2], i1 = b.f_cam[r1], i2 = b.f_cam[r2];
          if (i1 == i2 && r1 != r2) continue;
          fn(i1, i2, r1, r2);
        }
    }
  };
  each_pair([&](int i1, int i2, int, int) {
    int32_t& id = blk_of[(size_t)i1 * nf + i2];
    if (id < 0) { id = (int32_t)b.blk_ij.size(); b.blk_ij.push_back(i1 | (i2 << 8)); cnt.push_back(0); }
    cnt[id]++;
  });
  b.nblk = (int)b.blk_ij.size();
  b.bp_start.assign(b.nblk + 1, 0);
  for (int j = 0; j < b.nblk; j++) b.bp_start[j + 1] = b.bp_start[j] + cnt[j];
  b.bp_pairs.resize(2 * (size_t)b.bp_start[b.nblk]);
  { std::vector<int32_t>& fill = b.t_fill;
    fill.assign(b.bp_start.begin(), b.bp_start.end() - 1);
    each_pair([&](int i1, int i2, int r1, int r2) { const int at = fill[blk_of[(size_t)i1 * nf + i2]]++; b.bp_pairs[2 * (size_t)at] = r1; b.bp_pairs[2 * (size_t)at + 1] = r2; }); }
  // the Schur pass's schedule: tasks = the nf right-hand sides (a camera's rows, six sums) and the blocks (a block's pairs, 36 sums), each
  // done by one wave; cost ~ its rounds of 64 rows / pairs times the loads of a round, plus the reduction; longest first onto the least
  // loaded wave (ties: the lowest wave)
  {
    const int GW = std::max(b.cluster_waves, 1), nt = nf + b.nblk;
    std::vector<std::pair<int32_t, int32_t>> task(nt);          // (cost, id)
    // (weights per round 6 / 36 = the loads of a round, 25 / 100 for a task's fixed part: kernel 2.92 -> 2.78 ms for 32 windows; other
    //  weights -- diagonal blocks' coalesced rounds at 12 ... 80, the fixed part at 50 ... 300 -- measured within +-0.05 ms of it or worse)
    for (int i = 0; i < nf; i++) task[i] = {6 * ((b.cam_start[i + 1] - b.cam_start[i] + 63) / 64) + 25, i};
    for (int j = 0; j < b.nblk; j++) task[nf + j] = {36 * ((b.bp_start[j + 1] - b.bp_start[j] + 63) / 64) + 100, nf + j};
    std::stable_sort(task.begin(), task.end(), [](const std::pair<int32_t, int32_t>& x, const std::pair<int32_t, int32_t>& y) { return x.first > y.first; });
    std::vector<int64_t> load(GW, 0);
    std::vector<int32_t> owner(nt, 0), count(GW + 1, 0);
    for (int t = 0; t < nt; t++) {
      int w = 0;
      for (int k = 1; k < GW; k++) if (load[k] < load[w]) w = k;
      load[w] += task[t].first; owner[t] = w; count[w + 1]++;
    }
    for (int k = 0; k < GW; k++) count[k + 1] += count[k];
    b.sched_start.assign(count.begin(), count.end());
    b.sched_task.assign(std::max(nt, 1), 0);
    std::vector<int32_t> fill(count.begin(), count.end() - 1);
    for (int t = 0; t < nt; t++) b.sched_task[fill[owner[t]]++] = task[t].second;
  }
  // the waves' reduction buffers; during the solve the same area (from ctl + 64 on: 256 doubles of tree partials first) holds the panel copy
  // of win_cholesky_rhs, (n + 1) rows of kLpPitch doubles
  b.stage_doubles = std::max((kWinThreads / 64) * 4 * 36, kLpPitch * (6 * nf + 1) - 256 + 8);
  return DVM_OK;
}

}  // namespace dvm
