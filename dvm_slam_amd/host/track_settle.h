// dvm_slam_amd/host/track_settle.h -- the per-frame epilogue of dvmh_track_with_motion_model[_batch][_resident] (tracking.cpp): what the
// device chain handed back for one frame (dvm_track_result, the keypoints' query numbers, PoseOptimization's outlier flags) turned into
// CurrentFrame.mvpMapPoints after the outlier drop, the dropped points and dvmh_track_result.  Pure: only the two public headers, so it
// compiles without the device library (tools/check_track_settle.cpp).
#pragma once
#include <cstdint>
#include <cstring>

#include "dvmslam_host.h"

namespace dvm_host {

// Where query q's map-point id comes from is the caller's: LastFrame's mvpMapPoints through the keypoint the query was built from
// (mp_l[qi[q]]), or, with the map points resident on the device, the entry lists' slot[q] (dvm_track_finish_batch_resident numbers its
// queries by entry).  The two sources as callables for settle_tracked_frame:
struct HostIds { const int32_t* mp_l; const int* qi; int32_t operator()(int q) const { return mp_l[qi[q]]; } };
struct SlotIds { const int32_t* slot; int32_t operator()(int q) const { return slot[q]; } };

// what every outcome starts from: the extraction's counts, the flags of the search, nothing matched
inline void settle_begin(const dvm_track_result& r, int wide_window, int32_t* mp_c, int32_t* dropped, dvmh_track_result* out) {
  out->n = r.n; out->mono_index = r.mono_index; out->n_requeried = r.n_requeried; out->wide_window = wide_window;
  for (int j = 0; j < r.n; j++) { mp_c[j] = -1; dropped[j] = -1; }
}

// Sophus::SE3f(SE3quat_recov.rotation().cast<float>(), SE3quat_recov.translation().cast<float>()) (Optimizer.cc:1023-1025)
inline void pose_to_Tcw(const double* pose, dvm_se3f* Tcw) {
  for (int k = 0; k < 3; k++) Tcw->t[k] = (float)pose[k];
  for (int k = 0; k < 4; k++) Tcw->q[k] = (float)pose[3 + k];
}

// assign[j]: the query keypoint j was matched to, or -1; outlier[j]: PoseOptimization rejected that match (read for a complete frame)
template <class Ids>
inline void settle_tracked_frame(const dvm_track_result& r, const int32_t* assign, const uint8_t* outlier, const Ids id, const dvm_se3f& Tcw_pred,
                                 int wide_window, int32_t* mp_c, int32_t* dropped, dvmh_track_result* out) {
  settle_begin(r, wide_window, mp_c, dropped, out);
  const int N = r.n;
  out->nmatches_search = r.nmatches;
  if (r.status != DVM_TRACK_COMPLETE) {     // not tracked: the matches of the (doubled) search stay as SearchByProjection left them
    for (int j = 0; j < N; j++) if (assign[j] >= 0) mp_c[j] = id(assign[j]);
    out->nmatches = r.nmatches; out->tracked = 0; out->Tcw = Tcw_pred;
    // g2o::SE3Quat(Tcw.unit_quaternion().cast<double>(), Tcw.translation().cast<double>()) (Optimizer.cc:760): the pose untouched
    for (int k = 0; k < 3; k++) out->pose[k] = (double)Tcw_pred.t[k];
    for (int k = 0; k < 4; k++) out->pose[3 + k] = (double)Tcw_pred.q[k];
    return;
  }
  for (int j = 0; j < N; j++) {
    if (assign[j] < 0) continue;
    const int32_t mp = id(assign[j]);
    if (outlier[j]) dropped[j] = mp; else mp_c[j] = mp;
  }
  out->nmatches = r.nmatches_after; out->nmatches_map = r.nmatches_map; out->n_inliers = r.n_inliers; out->tracked = 1;
  std::memcpy(out->pose, r.pose, 56);
  pose_to_Tcw(out->pose, &out->Tcw);
}

}  // namespace dvm_host
