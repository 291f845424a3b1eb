// dvm_slam_amd/csrc/ba_window_seq_tables.h -- the index tables of the sequential-order window kernel (ba_window_seq.hip): g2o's incidence
// lists (block_solver.hpp:143-295) and the chunk tables the kernel streams by.  Pure host code, no HIP: checked on the CPU against a
// brute-force restatement (tools/check_ba_window_tables.cpp, run by tests/test_host_logic.py).
#pragma once
#include <algorithm>
#include <utility>

#include "ba_window_common.h"

namespace dvm {

constexpr int kWinIntCap = 6 * kWinThreads;   // ints of one chunk's index block (six per thread in flight)

struct SeqBuild {
  WinGraph g;
  int F = 0, nblk = 0, C = 128, C2 = 256, n_sc = 0, n_hc = 0, stage_doubles = 0;   // rows per Schur / Hessian chunk, chunks, LDS doubles of the staging area
  std::vector<int32_t> lpos, fpos;          // [E] row of the edge in landmark-major order over all edges / over free-camera edges (-1)
  std::vector<int32_t> pt_start, f_start;   // [nact + 1] a landmark's rows in rowA / in rowW
  std::vector<int32_t> f_cam;               // [F] free camera index of the row
  std::vector<int32_t> hc_ints, sc_desc, sc_ints;   // the chunks' int blocks and descriptors (layouts: SeqWin, ba_window_seq.hip)
  std::vector<int32_t> blk_ij;              // [nblk] i1 | i2 << 8 of the reduced system's blocks, in order of first appearance
};

// fills a fresh SeqBuild
inline int build_window_seq(const dvm_ba_window& w, SeqBuild& b, bool normalize) {
  WinGraph& g = b.g;
  const int rc = win_graph(w, normalize, &g);
  if (rc != DVM_OK) return rc;
  if (g.nfree > 24) { b.C = 32; b.C2 = 64; }              // the packed reduced system takes up to 130 KB of the 160: smaller streaming chunks (else 128 / 256)
  const int E = g.E, nf = g.nfree;
  // landmark-major order of the edges (a landmark's edges in input order): rowA's order; its free-camera subsequence: rowW's order
  b.pt_start.assign(g.nact + 1, 0);
  for (int k = 0; k < E; k++) b.pt_start[g.lidx[g.e_point[k]] + 1]++;
  for (int i = 0; i < g.nact; i++) b.pt_start[i + 1] += b.pt_start[i];
  std::vector<int32_t> pt_edges(E);
  b.lpos.resize(E);
  {
    std::vector<int32_t> pc(b.pt_start.begin(), b.pt_start.end() - 1);
    for (int k = 0; k < E; k++) { const int q = pc[g.lidx[g.e_point[k]]]++; pt_edges[q] = k; b.lpos[k] = q; }
  }
  b.fpos.assign(E, -1); b.f_start.assign(g.nact + 1, 0);
  std::vector<int32_t> f_edge;
  int maxdeg = 0;
  for (int li = 0; li < g.nact; li++) {
    for (int q = b.pt_start[li]; q < b.pt_start[li + 1]; q++) {
      const int k = pt_edges[q], i = g.pidx[g.e_pose[k]];
      if (i < 0) continue;
      b.fpos[k] = (int32_t)f_edge.size(); f_edge.push_back(k); b.f_cam.push_back(i);
    }
    b.f_start[li + 1] = (int32_t)f_edge.size();
    maxdeg = std::max(maxdeg, b.f_start[li + 1] - b.f_start[li]);
  }
  b.F = (int)f_edge.size();
  if (maxdeg > b.C) { set_error("dvm_ba_optimize_windows: a landmark with more free-camera observations than a streaming chunk holds (duplicate observations?)"); return DVM_ERR_CAPACITY; }
  // Hessian chunks: C2 consecutive edges; the free-camera ones among them listed per camera (ascending edge = the camera's own order)
  b.n_hc = nf ? (E + b.C2 - 1) / b.C2 : 0;
  b.hc_ints.assign((size_t)b.n_hc * (nf + 1 + b.C2), 0);
  for (int c = 0; c < b.n_hc; c++) {
    const int k0 = c * b.C2, k1 = std::min(E, k0 + b.C2);
    int32_t* rg = &b.hc_ints[(size_t)c * (nf + 1 + b.C2)];       // [range (nf + 1) | row slots, camera-major (<= C2)]
    for (int k = k0; k < k1; k++) { const int i = g.pidx[g.e_pose[k]]; if (i >= 0) rg[i + 1]++; }
    for (int i = 0; i < nf; i++) rg[i + 1] += rg[i];
    std::vector<int32_t> fill(rg, rg + nf);
    for (int k = k0; k < k1; k++) { const int i = g.pidx[g.e_pose[k]]; if (i >= 0) rg[nf + 1 + fill[i]++] = k - k0; }
  }
  // Schur chunks: whole landmarks -- at most C of them, at most C free rows, an int block of at most kWinIntCap --; per chunk the rows by
  // camera, the landmark of every row, and the (edge, edge) pairs of block_solver.hpp:381-439 -- landmark by landmark, per landmark edge k1
  // (outer) x edge k2 (inner), lower blocks only, (k1, k1) on the diagonal -- sorted by block (stable: a block's pairs stay in landmark order)
  std::vector<int32_t> blk_of((size_t)nf * nf, -1);
  int max_ints = 0;
  for (int li = 0; li < g.nact;) {
    const int r0 = b.f_start[li];
    int lj = li, npairs = 0;
    while (lj < g.nact && lj - li < b.C && b.f_start[lj + 1] - r0 <= b.C) {
      const int deg = b.f_start[lj + 1] - b.f_start[lj];
      const int np_new = npairs + deg * (deg + 1) / 2 + deg * (deg - 1) / 2 * 0;    // lower blocks incl. the diagonal: one pair per (k1, k2) with i2 <= i1
      const int rows_new = b.f_start[lj + 1] - r0;
      if (lj > li && nf + 1 + 2 * rows_new + 2 * (np_new + deg * deg) + 1 > kWinIntCap) break;   // (generous: duplicates of a camera add pairs)
      npairs = np_new; lj++;
    }
    if (lj == li) { set_error("dvm_ba_optimize_windows: a landmark does not fit a streaming chunk"); return DVM_ERR_CAPACITY; }
    const int r1 = b.f_start[lj], nr = r1 - r0;
    const int32_t ioff = (int32_t)b.sc_ints.size();
    b.sc_ints.resize(ioff + nf + 1 + 2 * nr, 0);
    int32_t* rg = &b.sc_ints[ioff];
    for (int r = r0; r < r1; r++) rg[b.f_cam[r] + 1]++;
    for (int i = 0; i < nf; i++) rg[i + 1] += rg[i];
    {
      std::vector<int32_t> fill(rg, rg + nf);
      for (int r = r0; r < r1; r++) b.sc_ints[ioff + nf + 1 + fill[b.f_cam[r]]++] = r - r0;
    }
    for (int l2 = li; l2 < lj; l2++)
      for (int r = b.f_start[l2]; r < b.f_start[l2 + 1]; r++) b.sc_ints[ioff + nf + 1 + nr + (r - r0)] = l2 - li;
    std::vector<std::pair<int32_t, int32_t>> pr;       // (block, slot1 | slot2 << 16)
    for (int l2 = li; l2 < lj; l2++)
      for (int q1 = b.f_start[l2]; q1 < b.f_start[l2 + 1]; q1++)
        for (int q2 = b.f_start[l2]; q2 < b.f_start[l2 + 1]; q2++) {
          const int i1 = b.f_cam[q1], i2 = b.f_cam[q2];
          if (i2 > i1 || (i2 == i1 && q2 != q1)) continue;
          int32_t& id = blk_of[(size_t)i1 * nf + i2];
          if (id < 0) { id = (int32_t)b.blk_ij.size(); b.blk_ij.push_back(i1 | (i2 << 8)); }
          pr.push_back({id, (q1 - r0) | ((q2 - r0) << 16)});
        }
    std::stable_sort(pr.begin(), pr.end(), [](const std::pair<int32_t, int32_t>& x, const std::pair<int32_t, int32_t>& y) { return x.first < y.first; });
    int nruns = 0;
    for (size_t j = 0; j < pr.size(); j++)
      if (j == 0 || pr[j].first != pr[j - 1].first) { b.sc_ints.push_back(b.blk_ij[pr[j].first] | ((int32_t)j << 16)); nruns++; }   // (i1 | i2 << 8 | first pair << 16)
    b.sc_ints.push_back((int32_t)pr.size() << 16);       // sentinel: where the last run ends
    for (const auto& q : pr) b.sc_ints.push_back(q.second);
    const int ni = (int)b.sc_ints.size() - ioff;
    if (ni > kWinIntCap || pr.size() >= 65536) { set_error("dvm_ba_optimize_windows: the index block of a chunk exceeds its capacity"); return DVM_ERR_CAPACITY; }
    max_ints = std::max(max_ints, ni);
    const int32_t d[8] = {r0, nr, ioff, ni, nruns + 1, (int32_t)pr.size(), li, lj - li};
    b.sc_desc.insert(b.sc_desc.end(), d, d + 8);
    li = lj;
  }
  b.n_sc = (int)b.sc_desc.size() / 8;
  b.nblk = (int)b.blk_ij.size();
  const size_t hess = (size_t)b.C2 * kRowB + ((size_t)b.C2 + nf + 1 + 1) / 2;
  const size_t schur = (size_t)b.C * (kRowW + kRowD + kRowH) + ((size_t)max_ints + 1) / 2;
  b.stage_doubles = (int)std::max(hess, schur) + 2;
  return DVM_OK;
}

}  // namespace dvm
