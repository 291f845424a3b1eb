// dvm_slam_amd/csrc/ba_window_resident.hip -- the two ends dvm_ba_resident_optimize attaches to the cluster form of the window optimizer
// (ba_window_cluster.hip, untouched): a GATHER kernel in front of the solver that fills the solver view's e_obs / e_info / pts from the
// keyframe slots and the map slots, and the PREPARE kernels behind it that leave the camera centres, the dirty flags and the geometry of
// SetWorldPos + MapPoint::UpdateNormalAndDepth in memory of the handle, where dvm_ba_resident_commit's scatter (map_store_kernels.hip)
// reads them.  No kernel checks an index: the entry has (ba_window.cpp), before anything was queued.  A lane per edge / point / camera,
// no LDS, no barrier.  Float arithmetic: pose_f32.h, one rounding per operation (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "ba_window_common.h"
#include "keyframe_store.h"
#include "map_store.h"
#include "point_geometry.h"
#include "pose_f32.h"

namespace dvm {

static_assert(sizeof(dvm_ba_obs) == 12 && sizeof(ResidentKf) == 32, "what travels up per observation and per camera");

// blockIdx.y = window; lane j < E: the edge at SORTED index j (the tables' order) from its caller index e_orig[j]; lane l < L: the point.
// The casts are Optimizer.cc:1188 (Vector3d of GetWorldPos) and :1207-1217 (obs << kpUn.pt.x, kpUn.pt.y; mvInvLevelSigma2[kpUn.octave]).
__global__ void __launch_bounds__(256) k_ba_res_gather(const ResidentWinDev* __restrict__ wins) {
  const ResidentWinDev& W = wins[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < W.E) {
    const dvm_ba_obs ob = W.obs[W.e_orig[i]];
    const ResidentKf kf = W.kf[ob.pose];
    const dvm_keypoint_pod kp = kf.kps[ob.kp];
    W.e_obs[2 * (size_t)i] = (double)kp.x;
    W.e_obs[2 * (size_t)i + 1] = (double)kp.y;
    W.e_info[i] = (double)kf.inv_sigma2[kp.octave];
  }
  if (i < W.L) {
    const float* pos = W.records[W.mp_slot[i]].pos;
    W.pts[3 * (size_t)i] = (double)pos[0];
    W.pts[3 * (size_t)i + 1] = (double)pos[1];
    W.pts[3 * (size_t)i + 2] = (double)pos[2];
  }
}

// blockIdx.y = window, a lane per camera: mOw as SetPose leaves it.  Free: SE3f(Quaternionf(q), t) of the optimised pose -- the constructor
// normalises the quaternion (Optimizer.cc:1374) -- then inverse().translation().  Fixed: the caller's row, or the same of the input pose as it is.
__global__ void __launch_bounds__(64) k_ba_res_centres(const ResidentWinDev* __restrict__ wins) {
  const ResidentWinDev& W = wins[blockIdx.y];
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= W.P) return;
  float o[3];
  const bool fixed = W.fixed[p] != 0;
  if (fixed && W.ow_in) {
    o[0] = W.ow_in[3 * p]; o[1] = W.ow_in[3 * p + 1]; o[2] = W.ow_in[3 * p + 2];
  } else {
    const double* T = (fixed ? W.in_poses : W.out_poses) + 7 * (size_t)p;
    const float t[3] = {(float)T[0], (float)T[1], (float)T[2]};
    float q[4] = {(float)T[3], (float)T[4], (float)T[5], (float)T[6]};
    if (!fixed) { const float r[4] = {q[0], q[1], q[2], q[3]}; dvm_pose::quat_div(r, sqrtf(dvm_pose::sqnorm4(r)), q); }
    float qi[4];
    dvm_pose::se3_inverse(q, t, qi, o);
  }
  for (int c = 0; c < 3; c++) {
    W.ow[3 * p + c] = o[c];
    if (W.ow_out) W.ow_out[3 * p + c] = o[c];
  }
}

// blockIdx.y = window, a lane per point (its edges: a few tens at most).  Dirty: an edge with chi2 > chi2_erase or no positive depth
// (Optimizer.cc:1324).  Clean and used: SetWorldPos + UpdateNormalAndDepth over the edges in the caller's order (point_geometry.h).
__global__ void __launch_bounds__(256) k_ba_res_points(const ResidentWinDev* __restrict__ wins) {
  const ResidentWinDev& W = wins[blockIdx.y];
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= W.L) return;
  const int q0 = W.pe_start[l], q1 = W.pe_start[l + 1];
  bool dirty = false;
  for (int q = q0; q < q1; q++) {
    const int e = W.pe_edges[q];
    dirty = dirty || W.e_chi2[e] > W.chi2_erase || !W.e_depth[e];
  }
  const uint8_t state = q1 == q0 ? 2 : dirty ? 1 : 0;
  float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (state == 0) {
    const float pos[3] = {(float)W.out_pts[3 * (size_t)l], (float)W.out_pts[3 * (size_t)l + 1], (float)W.out_pts[3 * (size_t)l + 2]};
    float normal[3] = {0.f, 0.f, 0.f};
    for (int q = q0; q < q1; q++) {
      float t[3];
      geo_term(pos, W.ow + 3 * W.obs[W.pe_edges[q]].pose, t);
      geo_add(normal, t[0], t[1], t[2]);
    }
    geo_mean(pos, normal, q1 - q0, g);
    if (W.ref_edge) {
      const dvm_ba_obs ref = W.obs[W.ref_edge[l]];
      const ResidentKf kf = W.kf[ref.pose];
      geo_distances(pos, W.ow + 3 * ref.pose, kf.sf, kf.kps[ref.kp].octave, kf.n_levels, g);
    }
  }
  for (int c = 0; c < 8; c++) {
    W.geom[8 * (size_t)l + c] = g[c];
    if (W.geom_out) W.geom_out[8 * (size_t)l + c] = g[c];
  }
  W.state[l] = state;
  W.slot[l] = W.mp_slot[l];
  if (W.dirty_out) W.dirty_out[l] = state == 1 ? 1 : 0;
}

void ResidentStage::add_inputs(Stage& st) {
  for (int k = 0; k < K; k++) {
    const dvm_ba_window_resident& w = *rc.win[k].w;
    const size_t P = (size_t)w.n_poses, L = (size_t)w.n_points, E = (size_t)w.n_edges;
    Slots& s = sl[k];
    s.obs = st.in(E ? w.obs : nullptr, sizeof(dvm_ba_obs) * E);
    s.kf = st.in(P ? rc.win[k].kf : nullptr, sizeof(ResidentKf) * P);
    s.mp_slot = st.in(L ? w.mp_slot : nullptr, 4 * L);
    s.pe_start = st.in(rc.win[k].pe_start, 4 * (L + 1));
    s.pe_edges = st.in(E ? rc.win[k].pe_edges : nullptr, 4 * E);
    s.ref_edge = st.in(L ? w.ref_edge : nullptr, 4 * L);
    s.in_poses = st.in(P ? w.poses : nullptr, 56 * P);
    s.fixed = st.in(P ? w.fixed : nullptr, P);
    s.ow_in = st.in(P ? w.ow : nullptr, 12 * P);
    max_el = std::max(max_el, std::max(w.n_edges, w.n_points)); max_p = std::max(max_p, w.n_poses); max_l = std::max(max_l, w.n_points);
  }
  views_slot = st.in(views.data(), sizeof(ResidentWinDev) * (size_t)K);      // filled in by fill(), behind layout()
}
void ResidentStage::add_outputs(Stage& st) {
  for (int k = 0; k < K; k++) {
    const dvm_ba_window_resident& w = *rc.win[k].w;
    const size_t P = (size_t)w.n_poses, L = (size_t)w.n_points;
    Slots& s = sl[k];
    s.geom_out = st.out(L ? w.geometry_out : nullptr, 32 * L);
    s.dirty_out = st.out(L ? w.point_dirty_out : nullptr, L);
    s.ow_out = st.out(P ? w.ow_out : nullptr, 12 * P);
  }
}
void ResidentStage::add_scratch(Stage& st) {
  for (int k = 0; k < K; k++) {
    const dvm_ba_window_resident& w = *rc.win[k].w;
    const size_t L = (size_t)w.n_points, E = (size_t)w.n_edges;
    Slots& s = sl[k];
    s.e_obs = st.scratch(16 * E); s.e_info = st.scratch(8 * E); s.pts = st.scratch(24 * L);
  }
}

void ResidentStage::fill(const Stage& st, int k, const int32_t* e_orig, const double* out_poses, const double* out_pts, const double* e_chi2, const uint8_t* e_depth) {
  const WinResident& r = rc.win[k];
  const dvm_ba_window_resident& w = *r.w;
  const Slots& s = sl[k];
  ResidentWinDev& v = views[k];
  std::memset(&v, 0, sizeof(v));
  v.P = w.n_poses; v.L = w.n_points; v.E = w.n_edges;
  v.obs = st.ptr<dvm_ba_obs>(s.obs); v.kf = st.ptr<ResidentKf>(s.kf); v.mp_slot = st.ptr<int32_t>(s.mp_slot); v.records = r.records; v.e_orig = e_orig;
  v.e_obs = st.ptr<double>(s.e_obs); v.e_info = st.ptr<double>(s.e_info); v.pts = st.ptr<double>(s.pts);
  v.in_poses = st.ptr<double>(s.in_poses); v.out_poses = out_poses; v.out_pts = out_pts; v.e_chi2 = e_chi2;
  v.fixed = st.ptr<uint8_t>(s.fixed); v.e_depth = e_depth; v.ow_in = st.ptr<float>(s.ow_in);
  v.pe_start = st.ptr<int32_t>(s.pe_start); v.pe_edges = st.ptr<int32_t>(s.pe_edges); v.ref_edge = st.ptr<int32_t>(s.ref_edge);
  v.chi2_erase = w.chi2_erase;
  v.geom = r.geom; v.ow = r.ow; v.state = r.state; v.slot = r.slot;
  v.geom_out = st.ptr<float>(s.geom_out); v.ow_out = st.ptr<float>(s.ow_out); v.dirty_out = st.ptr<uint8_t>(s.dirty_out);
}

int ResidentStage::gather(const Stage& st) {
  hipStream_t s = st.stream();
  for (int i = 0; i < rc.n_kf_stores; i++) { const int r = kfs_read_begin(rc.kf_stores[i], s); if (r != DVM_OK) return r; }
  for (int i = 0; i < rc.n_map_stores; i++) { const int r = store_read_begin(rc.map_stores[i], s); if (r != DVM_OK) return r; }
  if (max_el > 0) hipLaunchKernelGGL(k_ba_res_gather, dim3((unsigned)((max_el + 255) / 256), (unsigned)K), dim3(256), 0, s, st.ptr<ResidentWinDev>(views_slot));
  { const int r = hip_check(hipGetLastError(), "k_ba_res_gather"); if (r != DVM_OK) return r; }
  for (int i = 0; i < rc.n_map_stores; i++) { const int r = store_read_end(rc.map_stores[i], s); if (r != DVM_OK) return r; }
  return DVM_OK;
}

int ResidentStage::prepare(const Stage& st) {
  hipStream_t s = st.stream();
  for (int i = 0; i < rc.n_wait; i++) DVM_HIP(hipStreamWaitEvent(s, rc.wait_ev[i], 0));
  if (max_p > 0) hipLaunchKernelGGL(k_ba_res_centres, dim3((unsigned)((max_p + 63) / 64), (unsigned)K), dim3(64), 0, s, st.ptr<ResidentWinDev>(views_slot));
  if (max_l > 0) hipLaunchKernelGGL(k_ba_res_points, dim3((unsigned)((max_l + 255) / 256), (unsigned)K), dim3(256), 0, s, st.ptr<ResidentWinDev>(views_slot));
  { const int r = hip_check(hipGetLastError(), "k_ba_res_points"); if (r != DVM_OK) return r; }
  for (int i = 0; i < rc.n_kf_stores; i++) { const int r = kfs_read_end(rc.kf_stores[i], s); if (r != DVM_OK) return r; }
  return DVM_OK;
}

}  // namespace dvm
