// dvm_slam_amd/csrc/ba_window_common.h -- what the two window optimizers really share.
//   ba_window_seq.hip      k_ba_window: g2o's summation order, the oracle's bits, pinhole (dvm_ba_optimize_windows)
//   ba_window_cluster.hip  k_ba_window_cluster<CAM>: tree sums, G workgroups per window (dvm_ba_optimize_windows_fast[_cam], dvm_ba_pool_*)
//   ba_window.cpp          the C entry points, the pool, and the host bookkeeping of a call that both launchers use (WinCall)
//   ba_window_resident.hip the gather / prepare kernels dvm_ba_resident_optimize puts around the cluster form (WinResident, ResidentStage)
// Host part first (no HIP: tools/check_ba_window_tables.cpp compiles it with g++): the graph front end of a window.  Device part below.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/dvmslam_hip.h"

namespace dvm {

void set_error(const std::string& msg);   // (orb_pipeline.h)

constexpr int kWinThreads = 512;
constexpr int kWinMaxFree = 30;          // 6 * 30 = 180 rows: packed lower triangle 130 320 B of LDS
constexpr int kRowB = 16, kRowA = 12, kRowW = 18, kRowD = 24, kRowH = 12;   // doubles per row of the per-edge / per-landmark arrays (rowA and Hll | bl: both forms)

// g2o's vertex numbering of one window (sparse_optimizer.cpp:161-185): the cameras that are free AND observed in pose order, the observed
// landmarks in point order; the edges as index arrays, in the caller's order.
struct WinGraph {
  int P = 0, L = 0, E = 0, nfree = 0, nact = 0;
  std::vector<double> poses;                 // [P][7], quaternions normalised if asked for (SE3Quat's constructor)
  std::vector<int32_t> pidx, lidx;           // [P] free index or -1; [L] active index or -1
  std::vector<int32_t> free_pose, act_pt;    // [nfree], [nact]
  std::vector<int32_t> e_pose, e_point;      // [E]
  std::vector<double> e_obs, e_info;         // [E][2], [E]
};
// validates the window's arrays, range-checks the edges, marks the used vertices, numbers them, applies the limit of 30 free cameras.
// g == nullptr: the checks alone, nothing built (a call of two launches checks ALL its windows before the first launch).
// obs != nullptr: a window of dvm_ba_resident_optimize -- the edges' indices come from obs, w.edges and w.points are not read and
// e_obs / e_info stay empty (a gather kernel fills them on the device from the resident stores).
// the obs argument of win_graph for a resident window (never NULL: a window without edges has no array to give)
inline const dvm_ba_obs* resident_obs(const dvm_ba_window_resident& w) { static const dvm_ba_obs none{0, 0, 0}; return w.obs ? w.obs : &none; }
inline int win_graph(const dvm_ba_window& w, bool normalize, WinGraph* g, const dvm_ba_obs* obs = nullptr) {
  const int P = w.n_poses, L = w.n_points, E = w.n_edges;
  if (P < 0 || L < 0 || E < 0 || (P && (!w.poses || !w.fixed)) || (!obs && ((L && !w.points) || (E && !w.edges)))) { set_error("dvm_ba_optimize_windows: null array"); return DVM_ERR_INVALID; }
  std::vector<uint8_t> pose_used(P, 0), pt_used(L, 0);
  if (g) { g->e_pose.resize(E); g->e_point.resize(E); g->e_obs.resize(obs ? 0 : 2 * (size_t)E); g->e_info.resize(obs ? 0 : E); }
  for (int k = 0; obs && k < E; k++) {
    const dvm_ba_obs& e = obs[k];
    if (e.pose < 0 || e.pose >= P || e.point < 0 || e.point >= L) { set_error("dvm_ba_optimize_windows: edge index out of range"); return DVM_ERR_INVALID; }
    pose_used[e.pose] = 1; pt_used[e.point] = 1;
    if (g) { g->e_pose[k] = e.pose; g->e_point[k] = e.point; }
  }
  for (int k = 0; !obs && k < E; k++) {
    const dvm_ba_edge& e = w.edges[k];
    if (e.pose < 0 || e.pose >= P || e.point < 0 || e.point >= L) { set_error("dvm_ba_optimize_windows: edge index out of range"); return DVM_ERR_INVALID; }
    pose_used[e.pose] = 1; pt_used[e.point] = 1;
    if (g) { g->e_pose[k] = e.pose; g->e_point[k] = e.point; g->e_obs[2 * (size_t)k] = e.u; g->e_obs[2 * (size_t)k + 1] = e.v; g->e_info[k] = e.inv_sigma2; }
  }
  int nfree = 0;
  for (int p = 0; p < P; p++) nfree += (!w.fixed[p] && pose_used[p]) ? 1 : 0;
  if (nfree > kWinMaxFree) { set_error("dvm_ba_optimize_windows: more than 30 free cameras in one window (use dvm_ba_optimize)"); return DVM_ERR_CAPACITY; }
  if (!g) return DVM_OK;
  g->P = P; g->L = L; g->E = E; g->nfree = g->nact = 0;
  g->poses.assign(w.poses, w.poses + 7 * (size_t)P);
  for (int p = 0; normalize && p < P; p++) {   // quat_normalize as the oracle / g2o::SE3Quat(q, t) does it: sign, then divide by the norm
    double* q = &g->poses[7 * (size_t)p + 3];
    if (q[3] < 0) for (int i = 0; i < 4; i++) q[i] = -q[i];
    const double nrm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; i++) q[i] /= nrm;
  }
  g->pidx.assign(P, -1); g->lidx.assign(L, -1); g->free_pose.clear(); g->act_pt.clear();
  for (int p = 0; p < P; p++) if (!w.fixed[p] && pose_used[p]) { g->pidx[p] = g->nfree++; g->free_pose.push_back(p); }
  for (int l = 0; l < L; l++) if (pt_used[l]) { g->lidx[l] = g->nact++; g->act_pt.push_back(l); }
  return DVM_OK;
}

}  // namespace dvm

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <chrono>
#include <type_traits>

#include "host_stage.h"
#include "proj_edge.h"

namespace dvm {

// packed lower triangle: row i starts at i (i + 1) / 2
__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }

// barrier for data exchanged through LDS only: __syncthreads() also waits for every global access in flight (s_waitcnt vmcnt(0)), i.e.
// for the NEXT chunk's rows that have just been requested -- which is the round trip the register pipeline exists to hide
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// the window's camera (proj_edge.h) out of its view: fx, fy, cx, cy, or the view's kb8[8] = mvParameters of a KannalaBrandt8 camera.  The
// sequential-order kernel is instantiated for the pinhole camera only -- its promise is g2o's bits, which a float atan2f does not have --,
// the cluster form for both.
template <class CAM, class WIN>
__device__ __forceinline__ CAM win_cam(const WIN& W) {
  if constexpr (std::is_same<CAM, PoseCamPinhole>::value) return PoseCamPinhole{W.fx, W.fy, W.cx, W.cy};
  else return PoseCamKB8{{W.kb8[0], W.kb8[1], W.kb8[2], W.kb8[3], W.kb8[4], W.kb8[5], W.kb8[6], W.kb8[7]}};
}

// a kernel's first words: the window's stats start as zeros (by the ONE thread that writes them)
__device__ __forceinline__ void win_stats_zero(dvm_ba_stats* st) {
  st->iterations = st->total_trials = st->stop_reason = st->kernel_us = 0;
  st->chi2_initial = st->chi2_final = st->lambda_final = 0;
  for (int i = 0; i < 64; i++) { st->trials_per_iter[i] = 0; st->chi2_per_iter[i] = 0; st->lambda_per_iter[i] = 0; }
  st->ms_structure = st->ms_optimize = 0; st->spec_trials = st->spec_kept = 0;
}

// ---- ba_window.cpp: the part of a call's host side that is the same for both forms -- the stop word the kernel polls, the per-window
// outputs (straight into the caller's arrays where it gave any), the wait that forwards the caller's stop flag, stats and the two
// measurement switches (DVM_BA_WINDOW_PROF: shader clocks per phase of window 0; DVM_BA_WINDOW_TIMING: the host phases of the call).
struct WinCall {
  using clock = std::chrono::steady_clock;
  const dvm_ba_window* windows;
  int K;
  const volatile uint8_t* stop_flag;
  int* stop_host = nullptr;             // the word the kernel polls, as the host writes it
  clock::time_point t[8];              // 0 entry, 1 built, 2 registered, 3 laid out, 4 views, 5 uploaded, 6 launched + waited, 7 downloaded
  struct Slots { int out_poses, out_pts, echi, edepth, stats, prof; };
  std::vector<Slots> sl;
  std::vector<dvm_ba_stats> st_out;
  std::vector<std::vector<unsigned long long>> prof_out;
  std::vector<unsigned long long> prof_zero;
  WinCall(const dvm_ba_window* w, int k, const volatile uint8_t* stop) : windows(w), K(k), stop_flag(stop) { mark(0); }     // (allocates nothing: the builds come first)
  void mark(int i) { t[i] = clock::now(); }
  int arm(int** stop_dev);              // the calling thread's stop word, set from the caller's flag; *stop_dev: its device address
  void add_outputs(Stage& st);
  template <class VIEW> void fill(const Stage& st, int k, VIEW& v) const {
    const Slots& s = sl[k];
    v.out_poses = st.ptr<double>(s.out_poses); v.out_pts = st.ptr<double>(s.out_pts);
    v.e_chi2 = st.ptr<double>(s.echi); v.e_depth = st.ptr<uint8_t>(s.edepth);
    v.stats = st.ptr<dvm_ba_stats>(s.stats);
    v.prof = s.prof >= 0 ? st.ptr<unsigned long long>(s.prof) : nullptr;
  }
  int wait(Stage& st, int G);           // behind the launch: forwards the caller's stop flag until the stream is through, then downloads
  // hands out the stats (and window 0's phase clocks, if asked for); kernel_us < 0: as the kernel left it (0)
  void finish(dvm_ba_stats* stats, const char* const* phase_names, int kernel_us);
};

// ---- dvm_ba_resident_optimize (ba_window.cpp: the entry and its checks; ba_window_resident.hip: the kernels): a window whose measurements
// and points lie in a keyframe store and a map store.  ba_windows_cluster takes one WinResident per window as the SOURCE of the solver
// view's e_obs / e_info / pts -- filled by a gather kernel in front of the solver instead of from the caller's arrays -- and runs the
// prepare kernels behind it; the launcher, its tables and the solver are the same.
struct dvm_keypoint_pod;
struct ResidentKf { const dvm_keypoint_pod* kps; const float *inv_sigma2, *sf; int32_t n_levels, pad; };   // a camera's slot (device addresses)
struct WinResident {
  const dvm_ba_window_resident* w;       // checked by the entry: every index the kernels form lies inside its array
  const ResidentKf* kf;                  // [n_poses], host
  const dvm_local_point* records;        // the window's map store (device)
  const int32_t *pe_start, *pe_edges;    // a point's edges in the caller's order (ba_resident_lists.h), host
  float* geom; uint8_t* state; int32_t* slot; float* ow;   // memory of the handle (device): what a commit reads
};
struct ResidentCall {
  const WinResident* win;                // [K]
  const dvm_keyframe_store* const* kf_stores; int n_kf_stores;   // the distinct stores of the call: the brackets around the reading kernels
  const dvm_map_store* const* map_stores; int n_map_stores;
  const hipEvent_t* wait_ev; int n_wait; // queued commits that still read the handle's memory: the prepare kernels wait for them
  int64_t *h2d, *d2h;                    // bytes sent up / fetched, accumulated over the call's launches
};
// the device view of a window for the three kernels; state: 0 clean and used, 1 dirty, 2 unused
struct ResidentWinDev {
  int32_t P, L, E, pad;
  const dvm_ba_obs* obs; const ResidentKf* kf; const int32_t* mp_slot; const dvm_local_point* records; const int32_t* e_orig;
  double *e_obs, *e_info, *pts;
  const double *in_poses, *out_poses, *out_pts, *e_chi2; const uint8_t *fixed, *e_depth; const float* ow_in;
  const int32_t *pe_start, *pe_edges, *ref_edge; double chi2_erase;
  float *geom, *ow, *geom_out, *ow_out; uint8_t *state, *dirty_out; int32_t* slot;
};
// the Stage items, views and launches a ResidentCall adds to ba_windows_cluster
struct ResidentStage {
  const ResidentCall rc; const int K;
  struct Slots { int obs, kf, mp_slot, pe_start, pe_edges, ref_edge, in_poses, fixed, ow_in, e_obs, e_info, pts, geom_out, dirty_out, ow_out; };
  std::vector<Slots> sl;
  std::vector<ResidentWinDev> views;
  int views_slot = -1, max_el = 0, max_p = 0, max_l = 0;
  ResidentStage(const ResidentCall& c, int k) : rc(c), K(k), sl(k), views(k) {}
  // before layout().  Inputs first; the host outputs right behind WinCall's (Stage::download fetches ONE span from the first output to
  // the last: working memory between two outputs would travel down with them); then the solver's three arrays as scratch
  void add_inputs(Stage& st);
  void add_outputs(Stage& st);
  void add_scratch(Stage& st);
  double* e_obs(const Stage& st, int k) const { return st.ptr<double>(sl[k].e_obs); }
  double* e_info(const Stage& st, int k) const { return st.ptr<double>(sl[k].e_info); }
  double* pts(const Stage& st, int k) const { return st.ptr<double>(sl[k].pts); }
  // behind layout(): window k's view from the solver view's pointers
  void fill(const Stage& st, int k, const int32_t* e_orig, const double* out_poses, const double* out_pts, const double* e_chi2, const uint8_t* e_depth);
  int gather(const Stage& st);           // read brackets of the stores open, the gather kernel, the map stores' brackets closed
  int prepare(const Stage& st);          // the waits for queued commits, centres and points, the keyframe stores' brackets closed
};

}  // namespace dvm
#endif  // __HIPCC__
