// tools/check_ba_window_tables.cpp -- CPU check of the window optimizers' index tables (run by tests/test_host_logic.py):
// dvm_slam_amd/csrc/ba_window_seq_tables.h (lpos / fpos, Hessian chunks, Schur chunks with runs and pairs) and
// dvm_slam_amd/csrc/ba_window_cluster_tables.h (camera-major order, pt_edges, bp_start / bp_pairs, the wave schedule) against a brute-force
// restatement of block_solver.hpp's Schur loop: per landmark, edge k1 (outer) x edge k2 (inner) over its free-camera observations, lower
// blocks only, no off-diagonal pair of two observations by the same camera.  Pure host code:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/check_ba_window_tables.cpp -o /tmp/check_ba_window_tables
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../dvm_slam_amd/csrc/ba_window_cluster_tables.h"
#include "../dvm_slam_amd/csrc/ba_window_seq_tables.h"

static std::string g_error;
namespace dvm { void set_error(const std::string& msg) { g_error = msg; } }
using namespace dvm;

static const char* g_case = "";
#define CHECK(cond)                                                                                  \
  do {                                                                                               \
    if (!(cond)) { std::printf("FAILED [%s] line %d: %s\n", g_case, __LINE__, #cond); std::exit(1); } \
  } while (0)

struct Window {
  std::vector<double> poses, points;
  std::vector<uint8_t> fixed;
  std::vector<dvm_ba_edge> edges;
  dvm_ba_window w() const {
    dvm_ba_window x;
    std::memset(&x, 0, sizeof(x));
    x.n_poses = (int)fixed.size(); x.n_points = (int)points.size() / 3; x.n_edges = (int)edges.size(); x.iterations = 5;
    x.poses = poses.data(); x.fixed = fixed.data(); x.points = points.data(); x.edges = edges.data();
    return x;
  }
};
static uint32_t g_seed = 12345u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// P cameras (fixed as given), L landmarks, landmark l seen by cameras cams_of(l); the edge list is then shuffled: neither landmark- nor
// camera-major
template <class F> static Window make(const std::vector<uint8_t>& fixed, int L, F&& cams_of) {
  Window W;
  const int P = (int)fixed.size();
  W.fixed = fixed;
  W.poses.assign(7 * (size_t)P, 0.0);
  for (int p = 0; p < P; p++) { W.poses[7 * p] = 0.1 * p; W.poses[7 * p + 6] = (p & 1) ? -2.0 : 1.0; }     // (unnormalised, one negative w)
  W.points.assign(3 * (size_t)L, 1.0);
  for (int l = 0; l < L; l++)
    for (int p : cams_of(l)) { dvm_ba_edge e; std::memset(&e, 0, sizeof(e)); e.pose = p; e.point = l; e.u = (float)(l + p); e.v = (float)(l - p); e.inv_sigma2 = 1.0f; W.edges.push_back(e); }
  for (size_t i = W.edges.size(); i > 1; i--) std::swap(W.edges[i - 1], W.edges[rnd() % i]);
  return W;
}

struct Truth {
  int nfree = 0, nact = 0, F = 0;
  std::vector<int> pidx, lidx;
  std::set<std::tuple<int, int, int, int>> pairs;     // (i1, i2, edge k1, edge k2), the caller's edge indices
};
static Truth brute(const Window& W) {
  Truth T;
  const int P = (int)W.fixed.size(), L = (int)W.points.size() / 3, E = (int)W.edges.size();
  std::vector<char> pu(P, 0), lu(L, 0);
  for (const dvm_ba_edge& e : W.edges) { pu[e.pose] = 1; lu[e.point] = 1; }
  T.pidx.assign(P, -1); T.lidx.assign(L, -1);
  for (int p = 0; p < P; p++) if (!W.fixed[p] && pu[p]) T.pidx[p] = T.nfree++;
  for (int l = 0; l < L; l++) if (lu[l]) T.lidx[l] = T.nact++;
  for (int l = 0; l < L; l++) {
    std::vector<int> obs;
    for (int k = 0; k < E; k++) if (W.edges[k].point == l && T.pidx[W.edges[k].pose] >= 0) obs.push_back(k);
    T.F += (int)obs.size();
    for (int k1 : obs)
      for (int k2 : obs) {
        const int i1 = T.pidx[W.edges[k1].pose], i2 = T.pidx[W.edges[k2].pose];
        if (i2 > i1 || (i2 == i1 && k1 != k2)) continue;
        CHECK(T.pairs.insert({i1, i2, k1, k2}).second);
      }
  }
  return T;
}
static bool is_permutation_of_range(std::vector<int32_t> v, int n) {
  if ((int)v.size() != n) return false;
  std::sort(v.begin(), v.end());
  for (int i = 0; i < n; i++) if (v[i] != i) return false;
  return true;
}
static void check_graph(const Window& W, const Truth& T, const WinGraph& g) {
  const int E = (int)W.edges.size();
  CHECK(g.P == (int)W.fixed.size() && g.L == (int)W.points.size() / 3 && g.E == E && g.nfree == T.nfree && g.nact == T.nact);
  CHECK(std::vector<int>(g.pidx.begin(), g.pidx.end()) == T.pidx && std::vector<int>(g.lidx.begin(), g.lidx.end()) == T.lidx);
  CHECK((int)g.free_pose.size() == T.nfree && (int)g.act_pt.size() == T.nact);
  for (int i = 0; i < T.nfree; i++) CHECK(g.pidx[g.free_pose[i]] == i);
  for (int i = 0; i < T.nact; i++) CHECK(g.lidx[g.act_pt[i]] == i);
  for (int p = 0; p < g.P; p++) {     // normalised as SE3Quat's constructor does: w >= 0, unit norm
    const double* q = &g.poses[7 * (size_t)p + 3];
    CHECK(q[3] >= 0 && std::fabs(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] - 1.0) < 1e-12);
  }
}

static void check_seq(const Window& W, const Truth& T) {
  SeqBuild b;
  const dvm_ba_window w = W.w();
  CHECK(build_window_seq(w, b, true) == DVM_OK);
  const WinGraph& g = b.g;
  check_graph(W, T, g);
  const int E = g.E, nf = g.nfree;
  for (int k = 0; k < E; k++) CHECK(g.e_pose[k] == W.edges[k].pose && g.e_point[k] == W.edges[k].point);     // the caller's order
  CHECK(b.F == T.F && (nf > 24 ? (b.C == 32 && b.C2 == 64) : (b.C == 128 && b.C2 == 256)));
  // lpos: a permutation of [0, E), landmark-major, a landmark's edges in input order
  CHECK(is_permutation_of_range(b.lpos, E) && (int)b.pt_start.size() == g.nact + 1 && b.pt_start[g.nact] == E);
  std::vector<int> at(E);
  for (int k = 0; k < E; k++) at[b.lpos[k]] = k;
  for (int li = 0; li < g.nact; li++)
    for (int q = b.pt_start[li]; q < b.pt_start[li + 1]; q++) { CHECK(g.lidx[g.e_point[at[q]]] == li); CHECK(q == b.pt_start[li] || at[q - 1] < at[q]); }
  // fpos: -1 for the fixed cameras' edges, else a permutation of [0, F), the free subsequence of the landmark-major order
  std::vector<int32_t> fp;
  std::vector<int> f_edge(b.F, -1);
  for (int k = 0; k < E; k++) {
    CHECK((b.fpos[k] < 0) == (g.pidx[g.e_pose[k]] < 0));
    if (b.fpos[k] >= 0) { fp.push_back(b.fpos[k]); CHECK(b.fpos[k] < b.F); f_edge[b.fpos[k]] = k; }
  }
  CHECK(is_permutation_of_range(fp, b.F) && (int)b.f_cam.size() == b.F && (int)b.f_start.size() == g.nact + 1 && b.f_start[g.nact] == b.F);
  for (int r = 0; r < b.F; r++) { CHECK(b.f_cam[r] == g.pidx[g.e_pose[f_edge[r]]]); CHECK(r == 0 || b.lpos[f_edge[r - 1]] < b.lpos[f_edge[r]]); }
  for (int li = 0; li < g.nact; li++) for (int r = b.f_start[li]; r < b.f_start[li + 1]; r++) CHECK(g.lidx[g.e_point[f_edge[r]]] == li);
  // Hessian chunks: C2 consecutive edges, the free cameras' among them listed per camera in edge order
  CHECK(b.n_hc == (nf ? (E + b.C2 - 1) / b.C2 : 0) && b.hc_ints.size() == (size_t)b.n_hc * (nf + 1 + b.C2));
  for (int c = 0; c < b.n_hc; c++) {
    const int32_t* rg = &b.hc_ints[(size_t)c * (nf + 1 + b.C2)];
    const int k0 = c * b.C2, k1 = std::min(E, k0 + b.C2);
    CHECK(rg[0] == 0 && rg[nf] <= b.C2);
    int listed = 0;
    for (int i = 0; i < nf; i++) {
      CHECK(rg[i] <= rg[i + 1]);
      for (int q = rg[i]; q < rg[i + 1]; q++, listed++) {
        const int s = rg[nf + 1 + q];
        CHECK(s >= 0 && k0 + s < k1 && g.pidx[g.e_pose[k0 + s]] == i && (q == rg[i] || rg[nf + 1 + q - 1] < s));
      }
    }
    int want = 0;
    for (int k = k0; k < k1; k++) want += g.pidx[g.e_pose[k]] >= 0 ? 1 : 0;
    CHECK(listed == want);
  }
  // Schur chunks: whole landmarks in order, within C and kWinIntCap; the pairs of all chunks = the direct enumeration, every block's in landmark order
  CHECK(b.sc_desc.size() == 8 * (size_t)b.n_sc && (int)b.blk_ij.size() == b.nblk);
  std::set<std::tuple<int, int, int, int>> seen;
  std::map<std::pair<int, int>, int> last_lm;
  std::set<int32_t> blocks;
  int next_row = 0, next_lm = 0;
  for (int c = 0; c < b.n_sc; c++) {
    const int32_t* d = &b.sc_desc[8 * (size_t)c];
    const int r0 = d[0], nr = d[1], ioff = d[2], ni = d[3], nu = d[4], np = d[5], la = d[6], nlm = d[7];
    CHECK(r0 == next_row && la == next_lm && nlm >= 1 && nlm <= b.C && nr <= b.C && ni <= kWinIntCap && np < 65536);
    CHECK(r0 == b.f_start[la] && r0 + nr == b.f_start[la + nlm] && ni == nf + 1 + 2 * nr + nu + np && ioff + ni <= (int)b.sc_ints.size());
    next_row = r0 + nr; next_lm = la + nlm;
    const int32_t* rg = &b.sc_ints[ioff];
    const int32_t *rows = rg + nf + 1, *rowlm = rows + nr, *runs = rowlm + nr, *pairs = runs + nu;
    CHECK(rg[0] == 0 && rg[nf] == nr);
    std::vector<int32_t> slots(rows, rows + nr);
    CHECK(is_permutation_of_range(slots, nr));
    for (int i = 0; i < nf; i++) for (int q = rg[i]; q < rg[i + 1]; q++) { CHECK(b.f_cam[r0 + rows[q]] == i); CHECK(q == rg[i] || rows[q - 1] < rows[q]); }
    for (int s = 0; s < nr; s++) CHECK(g.lidx[g.e_point[f_edge[r0 + s]]] == la + rowlm[s]);
    CHECK((runs[0] >> 16) == 0 && (runs[nu - 1] >> 16) == np);
    std::set<int> run_blocks;
    for (int u = 0; u + 1 < nu; u++) {
      const int i1 = runs[u] & 255, i2 = (runs[u] >> 8) & 255, q0 = runs[u] >> 16, q1 = runs[u + 1] >> 16;
      CHECK(q0 < q1 && i2 <= i1 && i1 < nf && run_blocks.insert(i1 | (i2 << 8)).second);     // a block appears in ONE run per chunk
      blocks.insert(i1 | (i2 << 8));
      for (int q = q0; q < q1; q++) {
        const int s1 = pairs[q] & 0xffff, s2 = pairs[q] >> 16;
        CHECK(s1 < nr && s2 < nr && b.f_cam[r0 + s1] == i1 && b.f_cam[r0 + s2] == i2 && rowlm[s1] == rowlm[s2]);
        int& lm = last_lm.insert({{i1, i2}, -1}).first->second;
        CHECK(lm <= la + rowlm[s1]);
        lm = la + rowlm[s1];
        CHECK(seen.insert({i1, i2, f_edge[r0 + s1], f_edge[r0 + s2]}).second);
      }
    }
  }
  CHECK(next_row == b.F && (b.n_sc == 0 || next_lm == g.nact) && seen == T.pairs);
  CHECK(blocks == std::set<int32_t>(b.blk_ij.begin(), b.blk_ij.end()) && (int)blocks.size() == b.nblk);
}

static void check_cluster(const Window& W, const Truth& T, ClusterTables& b, int waves) {
  const dvm_ba_window w = W.w();
  b.cluster_waves = waves;
  CHECK(build_window_fast(w, b) == DVM_OK);
  const WinGraph& g = b.g;
  check_graph(W, T, g);
  const int E = g.E, nf = g.nfree;
  CHECK(b.F == T.F && b.Fp >= b.F && b.Fp % 64 == 0 && b.Fp < b.F + 64);
  // the sort: e_orig is a permutation; camera-major -- free cameras by free index, then the fixed cameras' edges --, a camera's edges by
  // landmark, equal (camera, landmark) in the caller's order
  CHECK(is_permutation_of_range(b.e_orig, E) && (int)b.cam_start.size() == nf + 1 && (int)b.f_cam.size() == b.F && (int)b.e_lm.size() == E);
  auto rank = [&](int j) { const int i = g.pidx[g.e_pose[j]]; return i >= 0 ? i : nf + g.e_pose[j]; };
  for (int j = 0; j < E; j++) {
    const dvm_ba_edge& e = W.edges[b.e_orig[j]];
    CHECK(g.e_pose[j] == e.pose && g.e_point[j] == e.point && g.e_obs[2 * (size_t)j] == e.u && g.e_obs[2 * (size_t)j + 1] == e.v && g.e_info[j] == e.inv_sigma2);
    CHECK(b.e_lm[j] == g.lidx[e.point] && (j < b.F) == (g.pidx[e.pose] >= 0));
    if (j < b.F) CHECK(b.f_cam[j] == g.pidx[e.pose] && b.cam_start[b.f_cam[j]] <= j && j < b.cam_start[b.f_cam[j] + 1]);
    if (j > 0) CHECK(std::make_tuple(rank(j - 1), b.e_lm[j - 1], b.e_orig[j - 1]) < std::make_tuple(rank(j), b.e_lm[j], b.e_orig[j]));
  }
  CHECK(b.cam_start[0] == 0 && b.cam_start[nf] == b.F);
  // a landmark's edges: every sorted index once, ascending within the landmark
  CHECK(is_permutation_of_range(b.pt_edges, E) && (int)b.pt_start.size() == g.nact + 1 && b.pt_start[g.nact] == E);
  for (int li = 0; li < g.nact; li++)
    for (int q = b.pt_start[li]; q < b.pt_start[li + 1]; q++) { CHECK(b.e_lm[b.pt_edges[q]] == li); CHECK(q == b.pt_start[li] || b.pt_edges[q - 1] < b.pt_edges[q]); }
  // blocks and pairs
  CHECK((int)b.blk_ij.size() == b.nblk && (int)b.bp_start.size() == b.nblk + 1 && b.bp_start[0] == 0 && b.bp_pairs.size() == 2 * (size_t)b.bp_start[b.nblk]);
  std::set<std::tuple<int, int, int, int>> seen;
  std::set<int32_t> blocks;
  for (int j = 0; j < b.nblk; j++) {
    const int i1 = b.blk_ij[j] & 255, i2 = (b.blk_ij[j] >> 8) & 255;
    CHECK(i2 <= i1 && i1 < nf && blocks.insert(b.blk_ij[j]).second && b.bp_start[j] < b.bp_start[j + 1]);
    int lm = -1;
    for (int q = b.bp_start[j]; q < b.bp_start[j + 1]; q++) {
      const int r1 = b.bp_pairs[2 * (size_t)q], r2 = b.bp_pairs[2 * (size_t)q + 1];
      CHECK(r1 >= 0 && r1 < b.F && r2 >= 0 && r2 < b.F && b.f_cam[r1] == i1 && b.f_cam[r2] == i2 && b.e_lm[r1] == b.e_lm[r2] && lm <= b.e_lm[r1]);
      lm = b.e_lm[r1];
      CHECK(seen.insert({i1, i2, b.e_orig[r1], b.e_orig[r2]}).second);
    }
  }
  CHECK(seen == T.pairs);
  // the schedule: every right-hand side and every block exactly once over the cluster's waves
  const int nt = nf + b.nblk;
  CHECK((int)b.sched_start.size() == waves + 1 && b.sched_start[0] == 0 && b.sched_start[waves] == nt && (int)b.sched_task.size() == std::max(nt, 1));
  std::vector<int32_t> tasks;
  for (int wv = 0; wv < waves; wv++) { CHECK(b.sched_start[wv] <= b.sched_start[wv + 1]); for (int q = b.sched_start[wv]; q < b.sched_start[wv + 1]; q++) tasks.push_back(b.sched_task[q]); }
  CHECK(is_permutation_of_range(tasks, nt));
  CHECK(b.stage_doubles >= kLpPitch * (6 * nf + 1) - 256 + 8 && b.stage_doubles >= (kWinThreads / 64) * 4 * 36);
}

static ClusterTables g_pooled;     // used by every case in turn, as the launcher's per-thread pool is
static void check_window(const char* name, const Window& W) {
  g_case = name;
  const Truth T = brute(W);
  check_seq(W, T);
  for (int waves : {8, 64}) {
    ClusterTables fresh;
    check_cluster(W, T, fresh, waves);
    check_cluster(W, T, g_pooled, waves);
    CHECK(fresh.e_orig == g_pooled.e_orig && fresh.blk_ij == g_pooled.blk_ij && fresh.bp_pairs == g_pooled.bp_pairs && fresh.sched_task == g_pooled.sched_task &&
          fresh.g.free_pose == g_pooled.g.free_pose && fresh.g.act_pt == g_pooled.g.act_pt);
  }
  std::printf("%-44s P=%-3d L=%-3d E=%-4d free=%-2d pairs=%zu ok\n", name, (int)W.fixed.size(), (int)W.points.size() / 3, (int)W.edges.size(), T.nfree, T.pairs.size());
}
static void check_refused(const char* name, const Window& W, int rc_want, const char* text) {
  g_case = name;
  const dvm_ba_window w = W.w();
  SeqBuild s;
  ClusterTables c;
  g_error.clear(); CHECK(win_graph(w, true, nullptr) == rc_want && g_error.find(text) != std::string::npos);
  g_error.clear(); CHECK(build_window_seq(w, s, true) == rc_want && g_error.find(text) != std::string::npos);
  g_error.clear(); CHECK(build_window_fast(w, c) == rc_want && g_error.find(text) != std::string::npos);
  std::printf("%-44s refused (%d): %s\n", name, rc_want, g_error.c_str());
}
// `nfree` free cameras behind two fixed ones; every landmark seen by `deg` cameras
static Window ring(int nfree, int L, int deg) {
  std::vector<uint8_t> fixed(nfree + 2, 0);
  fixed[0] = fixed[1] = 1;
  const int P = nfree + 2;
  return make(fixed, L, [=](int l) { std::vector<int> c; for (int j = 0; j < deg; j++) c.push_back((l * 5 + j * 3) % P); std::sort(c.begin(), c.end()); c.erase(std::unique(c.begin(), c.end()), c.end()); return c; });
}

int main() {
  // one free camera; pose 3 is free but unobserved, landmark 7 unobserved: neither is numbered
  check_window("1 free camera", make({1, 1, 0, 0}, 60, [](int l) { return l == 7 ? std::vector<int>{} : l % 3 ? std::vector<int>{0, 1, 2} : std::vector<int>{2, 1}; }));
  check_window("2 keyframes, the second free", make({1, 0}, 150, [](int l) { return l % 11 ? std::vector<int>{0, 1} : std::vector<int>{1}; }));
  check_window("a landmark seen twice by one camera", make({1, 0, 0, 0}, 40, [](int l) { return l % 4 == 0 ? std::vector<int>{1, 2, 1, 3, 0} : l % 4 == 1 ? std::vector<int>{2, 2} : std::vector<int>{0, 1, 2, 3}; }));
  check_window("a landmark seen only by fixed cameras", make({1, 1, 0, 0}, 50, [](int l) { return l % 5 == 2 ? std::vector<int>{0, 1} : std::vector<int>{0, 2, 3}; }));
  { const Window W = ring(25, 48, 8); check_window("25 free cameras (C = 32)", W); }
  check_window("30 free cameras", ring(30, 40, 9));
  check_refused("31 free cameras", ring(31, 40, 9), DVM_ERR_CAPACITY, "more than 30 free cameras");
  check_window("E = 0", make({1, 0}, 3, [](int) { return std::vector<int>{}; }));
  { Window W = ring(3, 20, 3); W.edges[W.edges.size() / 2].point = 20; check_refused("an edge's point out of range", W, DVM_ERR_INVALID, "edge index out of range"); }
  { Window W = ring(3, 20, 3); W.edges.back().pose = -1; check_refused("an edge's pose out of range", W, DVM_ERR_INVALID, "edge index out of range"); }
  std::printf("window tables as the direct enumeration\n");
  return 0;
}
