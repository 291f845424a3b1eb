// dvm_slam_amd/host/tracking.cpp -- dvmh_track_with_motion_model (include/dvmslam_host.h): the host side of the one-chain tracking
// step.  Reference: Frame::Frame -> ExtractORB (src/Frame.cc:371-411), Tracking::TrackWithMotionModel (src/Tracking.cc:2584-2667).
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dvmslam_host.h"
#include "orb_matcher.h"
#include "../csrc/camera_model.h"

using dvm_host::FrameQueries;
using dvm_host::FrameView;

namespace {
constexpr int TH_HIGH = 100;   // ORBmatcher::TH_HIGH, ORBmatcher.cc:36

// What the _cam entries do with their model before the shared body runs: checked as every *_cam entry checks it, the tracker set to it
// (dvm_tracker_set_camera_model).  *K: fx fy cx cy of the model (the caller's K is not read); *cam: the model for FrameView::mpCamera and
// dvm_pose_optimize_cam under KannalaBrandt8, NULL under model 0 -- the body is then the plain entry's, bit for bit.
int use_camera_model(dvm_tracker* t, const dvm_camera_model* model, const float** K, const dvm_camera_model** cam) {
  if (!t || !model || !dvm_cam::model_ok(model->model, model->p)) return DVM_ERR_INVALID;
  *cam = model->model == dvm_cam::kKannalaBrandt8 ? model : nullptr;
  *K = model->p;
  return dvm_tracker_set_camera_model(t, *cam);
}

// dvmh_track_with_motion_model and _cam: model NULL: the pinhole camera K; else a KannalaBrandt8 model the tracker is set to, K = model->p
int track_with_motion_model(dvm_tracker* t, dvm_orb* h, int device, const uint8_t* img, int rows, int cols, int stride, int lap0, int lap1,
                            const dvm_se3f* Tcw_pred, const float* K, const dvm_camera_model* model, const float* bounds, const dvm_distortion* dist,
                            const float* scale_factors, const float* inv_level_sigma2, int nlevels, int Nl, const dvm_keypoint* kps_l,
                            const int32_t* mp_l, const uint8_t* outlier_l, const dvmh_map_point* mps, float th, int check_ori, dvm_keypoint* kps,
                            uint8_t* desc, int cap, dvm_keypoint* kps_un, int32_t* mp_c, int32_t* dropped, dvmh_track_result* out) {
  if (!t || !h || !img || !Tcw_pred || !K || !bounds || !scale_factors || !inv_level_sigma2 || !kps || !desc || !mp_c || !dropped || !out ||
      (Nl && (!kps_l || !mp_l || !mps)))
    return DVM_ERR_INVALID;
  std::memset(out, 0, sizeof(*out));
  // 1. the extraction is on its way ...
  int rc = dvm_track_begin(t, h, img, rows, cols, stride, lap0, lap1);
  if (rc != DVM_OK) return rc;
  // 2. ... while the queries are built (they need LastFrame and the predicted pose only)
  FrameView C, L;
  C.N = 0; C.Tcw = *Tcw_pred;
  C.fx = K[0]; C.fy = K[1]; C.cx = K[2]; C.cy = K[3];
  C.mpCamera = model;            // CurrentFrame.mpCamera->project of LastFrame's points (ORBmatcher.cc:1586), both attempts
  C.mnMinX = bounds[0]; C.mnMaxX = bounds[1]; C.mnMinY = bounds[2]; C.mnMaxY = bounds[3];
  C.mvScaleFactors = scale_factors; C.nLevels = nlevels;
  L = C;
  L.N = Nl; L.mvKeysUn = kps_l; L.mvpMapPoints = const_cast<int32_t*>(mp_l); L.mvbOutlier = outlier_l;
  std::vector<dvm_keypoint> un_local;
  if (!kps_un) { un_local.resize((size_t)cap); kps_un = un_local.data(); }
  std::vector<int32_t> assign((size_t)cap);
  std::vector<uint8_t> outl((size_t)cap);
  std::vector<uint32_t> ranked;
  FrameQueries Q;
  std::vector<uint8_t> q_claims;
  std::vector<float> q_angle, q_pos;
  dvm_track_queries tq;
  dvm_track_result tr;
  float th_now = th;
  for (int attempt = 0; attempt < 2; attempt++) {
    dvm_host::BuildFrameQueries(C, L, mps, th_now, Q);
    const int nq = (int)Q.qi.size();
    q_claims.resize((size_t)nq); q_angle.resize((size_t)nq); q_pos.resize((size_t)nq * 3);
    for (int q = 0; q < nq; q++) {
      const int i = Q.qi[q], mp = mp_l[i];
      q_claims[q] = mps[mp].n_obs > 0;
      q_angle[q] = kps_l[i].angle;
      q_pos[3 * q] = mps[mp].pos[0]; q_pos[3 * q + 1] = mps[mp].pos[1]; q_pos[3 * q + 2] = mps[mp].pos[2];
    }
    ranked.resize((size_t)nq * 4 + 4);
    std::memset(&tq, 0, sizeof(tq));
    tq.nq = nq; tq.qdesc = Q.qdesc.data(); tq.qx = Q.qx.data(); tq.qy = Q.qy.data(); tq.qr = Q.qr.data(); tq.qmin = Q.qmin.data(); tq.qmax = Q.qmax.data();
    tq.q_claims = q_claims.data(); tq.q_angle = q_angle.data(); tq.q_pos = q_pos.data();
    std::memcpy(tq.bounds, bounds, 16);
    tq.dist = dist; tq.inv_level_sigma2 = inv_level_sigma2; tq.nlevels = nlevels;
    tq.cam.fx = K[0]; tq.cam.fy = K[1]; tq.cam.cx = K[2]; tq.cam.cy = K[3]; tq.cam.huber_delta = 0.0;
    // g2o::SE3Quat(Tcw.unit_quaternion().cast<double>(), Tcw.translation().cast<double>()) (Optimizer.cc:760)
    for (int k = 0; k < 3; k++) tq.pose_in[k] = (double)Tcw_pred->t[k];
    for (int k = 0; k < 4; k++) tq.pose_in[3 + k] = (double)Tcw_pred->q[k];
    tq.th_high = TH_HIGH; tq.check_ori = check_ori; tq.min_matches = 20;
    rc = dvm_track_finish(t, h, &tq, kps, desc, cap, kps_un, assign.data(), outl.data(), ranked.data(), &tr);
    if (rc != DVM_OK) return rc;
    out->n = tr.n; out->mono_index = tr.mono_index; out->n_requeried = tr.n_requeried;
    if (tr.status != DVM_TRACK_FEW_MATCHES || attempt == 1) break;
    th_now = 2 * th;                       // Tracking.cc:2616-2624: "Not enough matches, wider window search"
    out->wide_window = 1;
  }
  const int N = tr.n;
  for (int j = 0; j < N; j++) { mp_c[j] = -1; dropped[j] = -1; }
  if (tr.status == DVM_TRACK_REPLAY_ON_HOST) {
    // rare: a query ran out of ranked candidates.  The separate calls take over from the frame's host arrays (same results by
    // construction: they are what the chain is tested against)
    out->replayed_on_host = 1;
    C.N = N; C.mvKeysUn = kps_un; C.mDescriptors = desc; C.mvpMapPoints = mp_c;
    dvm_host::ORBmatcher m(0.9f, check_ori != 0, device);
    int nm = m.SearchByProjection(C, L, mps, th_now, true);
    if (nm < 0) return nm;
    if (nm < 20 && !out->wide_window) {
      for (int j = 0; j < N; j++) mp_c[j] = -1;
      out->wide_window = 1;
      nm = m.SearchByProjection(C, L, mps, 2 * th, true);
      if (nm < 0) return nm;
    }
    out->nmatches_search = nm;
    if (nm < 20) { out->nmatches = nm; out->tracked = 0; out->Tcw = *Tcw_pred; return DVM_OK; }
    std::vector<double> Xw, obs, w;
    std::vector<int> kp_of;
    for (int j = 0; j < N; j++) {
      if (mp_c[j] < 0) continue;
      for (int k = 0; k < 3; k++) Xw.push_back((double)mps[mp_c[j]].pos[k]);
      obs.push_back((double)kps_un[j].x); obs.push_back((double)kps_un[j].y);
      w.push_back((double)inv_level_sigma2[kps_un[j].octave]);
      kp_of.push_back(j);
    }
    const int32_t ne = (int32_t)kp_of.size();
    std::vector<uint8_t> rej((size_t)ne);
    int32_t inl = 0;
    rc = model ? dvm_pose_optimize_cam(device, tq.pose_in, Xw.data(), obs.data(), w.data(), &ne, ne, 1, model, out->pose, rej.data(), &inl)
               : dvm_pose_optimize(device, tq.pose_in, Xw.data(), obs.data(), w.data(), &ne, ne, 1, &tq.cam, out->pose, rej.data(), &inl);
    if (rc != DVM_OK) return rc;
    out->n_inliers = inl;
    int left = nm, nmap = 0;
    for (int e = 0; e < ne; e++) {
      const int j = kp_of[e];
      if (rej[e]) { dropped[j] = mp_c[j]; mp_c[j] = -1; left--; }
      else if (mps[mp_c[j]].n_obs > 0) nmap++;
    }
    out->nmatches = left; out->nmatches_map = nmap; out->tracked = 1;
  } else {
    out->nmatches_search = tr.nmatches;
    if (tr.status == DVM_TRACK_FEW_MATCHES) {    // not tracked: the matches of the (doubled) search stay as SearchByProjection left them
      for (int j = 0; j < N; j++) if (assign[j] >= 0) mp_c[j] = mp_l[Q.qi[assign[j]]];
      out->nmatches = tr.nmatches; out->tracked = 0; out->Tcw = *Tcw_pred;
      for (int k = 0; k < 7; k++) out->pose[k] = tq.pose_in[k];
      return DVM_OK;
    }
    for (int j = 0; j < N; j++) {
      if (assign[j] < 0) continue;
      const int mp = mp_l[Q.qi[assign[j]]];
      if (outl[j]) dropped[j] = mp; else mp_c[j] = mp;
    }
    out->nmatches = tr.nmatches_after; out->nmatches_map = tr.nmatches_map; out->n_inliers = tr.n_inliers; out->tracked = 1;
    std::memcpy(out->pose, tr.pose, 56);
  }
  // Sophus::SE3f(SE3quat_recov.rotation().cast<float>(), SE3quat_recov.translation().cast<float>()) (Optimizer.cc:1023-1025)
  for (int k = 0; k < 3; k++) out->Tcw.t[k] = (float)out->pose[k];
  for (int k = 0; k < 4; k++) out->Tcw.q[k] = (float)out->pose[3 + k];
  return DVM_OK;
}
}  // namespace

extern "C" int dvmh_track_with_motion_model(dvm_tracker* t, dvm_orb* h, int device, const uint8_t* img, int rows, int cols, int stride, int lap0,
                                            int lap1, const dvm_se3f* Tcw_pred, const float* K, const float* bounds, const dvm_distortion* dist,
                                            const float* scale_factors, const float* inv_level_sigma2, int nlevels, int Nl,
                                            const dvm_keypoint* kps_l, const int32_t* mp_l, const uint8_t* outlier_l, const dvmh_map_point* mps,
                                            float th, int check_ori, dvm_keypoint* kps, uint8_t* desc, int cap, dvm_keypoint* kps_un,
                                            int32_t* mp_c, int32_t* dropped, dvmh_track_result* out) {
  return track_with_motion_model(t, h, device, img, rows, cols, stride, lap0, lap1, Tcw_pred, K, nullptr, bounds, dist, scale_factors, inv_level_sigma2,
                                 nlevels, Nl, kps_l, mp_l, outlier_l, mps, th, check_ori, kps, desc, cap, kps_un, mp_c, dropped, out);
}
extern "C" int dvmh_track_with_motion_model_cam(dvm_tracker* t, dvm_orb* h, int device, const uint8_t* img, int rows, int cols, int stride, int lap0,
                                                int lap1, const dvm_se3f* Tcw_pred, const float* K, const dvm_camera_model* model, const float* bounds,
                                                const dvm_distortion* dist, const float* scale_factors, const float* inv_level_sigma2, int nlevels,
                                                int Nl, const dvm_keypoint* kps_l, const int32_t* mp_l, const uint8_t* outlier_l,
                                                const dvmh_map_point* mps, float th, int check_ori, dvm_keypoint* kps, uint8_t* desc, int cap,
                                                dvm_keypoint* kps_un, int32_t* mp_c, int32_t* dropped, dvmh_track_result* out) {
  (void)K;
  const float* Km = nullptr; const dvm_camera_model* cam = nullptr;
  const int rc = use_camera_model(t, model, &Km, &cam);
  if (rc != DVM_OK) return rc;
  return track_with_motion_model(t, h, device, img, rows, cols, stride, lap0, lap1, Tcw_pred, Km, cam, bounds, dist, scale_factors, inv_level_sigma2,
                                 nlevels, Nl, kps_l, mp_l, outlier_l, mps, th, check_ori, kps, desc, cap, kps_un, mp_c, dropped, out);
}


// ---- K agents' frames at one camera tick: dvmh_track_with_motion_model for `count` frames through ONE chain of batched launches
// (dvm_track_begin_batch / dvm_track_finish_batch).  Per frame exactly the steps of the single call; the queries of the frames are
// built by a few host threads while the batch extraction runs.
namespace {
struct AgentQueries {
  FrameQueries Q;
  std::vector<uint8_t> q_claims;
  std::vector<float> q_angle, q_pos;
  FrameView C, L;
  void build(const dvmh_track_in& in, const float* K, const dvm_camera_model* model, const float* bounds, const float* scale_factors, int nlevels, float th) {
    C = FrameView();
    C.N = 0; C.Tcw = *in.Tcw_pred;
    C.fx = K[0]; C.fy = K[1]; C.cx = K[2]; C.cy = K[3];
    C.mpCamera = model;
    C.mnMinX = bounds[0]; C.mnMaxX = bounds[1]; C.mnMinY = bounds[2]; C.mnMaxY = bounds[3];
    C.mvScaleFactors = scale_factors; C.nLevels = nlevels;
    L = C;
    L.N = in.Nl; L.mvKeysUn = in.kps_l; L.mvpMapPoints = const_cast<int32_t*>(in.mp_l); L.mvbOutlier = in.outlier_l;
    dvm_host::BuildFrameQueries(C, L, in.mps, th, Q);
    const int nq = (int)Q.qi.size();
    q_claims.resize((size_t)nq); q_angle.resize((size_t)nq); q_pos.resize((size_t)nq * 3);
    for (int q = 0; q < nq; q++) {
      const int i = Q.qi[q], mp = in.mp_l[i];
      q_claims[q] = in.mps[mp].n_obs > 0;
      q_angle[q] = in.kps_l[i].angle;
      q_pos[3 * q] = in.mps[mp].pos[0]; q_pos[3 * q + 1] = in.mps[mp].pos[1]; q_pos[3 * q + 2] = in.mps[mp].pos[2];
    }
  }
  void fill(dvm_track_queries& tq, const dvmh_track_in& in, const float* K, const float* bounds, const float* inv_level_sigma2, int nlevels, int check_ori) const {
    std::memset(&tq, 0, sizeof(tq));
    tq.nq = (int)Q.qi.size(); tq.qdesc = Q.qdesc.data(); tq.qx = Q.qx.data(); tq.qy = Q.qy.data(); tq.qr = Q.qr.data(); tq.qmin = Q.qmin.data(); tq.qmax = Q.qmax.data();
    tq.q_claims = q_claims.data(); tq.q_angle = q_angle.data(); tq.q_pos = q_pos.data();
    std::memcpy(tq.bounds, bounds, 16);
    tq.dist = nullptr; tq.inv_level_sigma2 = inv_level_sigma2; tq.nlevels = nlevels;
    tq.cam.fx = K[0]; tq.cam.fy = K[1]; tq.cam.cx = K[2]; tq.cam.cy = K[3]; tq.cam.huber_delta = 0.0;
    for (int k = 0; k < 3; k++) tq.pose_in[k] = (double)in.Tcw_pred->t[k];
    for (int k = 0; k < 4; k++) tq.pose_in[3 + k] = (double)in.Tcw_pred->q[k];
    tq.th_high = TH_HIGH; tq.check_ori = check_ori; tq.min_matches = 20;
  }
};
}  // namespace

#include <thread>

namespace {
// A few persistent host threads for the per-tick work of the batched chain (the agents' query lists are independent): run(n, width, fn) calls
// fn(i) for i in [0, n) on the caller and up to width - 1 workers and returns when all are done.  One job at a time; never destroyed (its
// sleeping workers end with the process -- a destructor that joined them would run in forked children, where they do not exist).
class TickPool {
 public:
  static TickPool& get() { static TickPool* p = new TickPool; return *p; }
  template <class F> void run(int n, int width, F&& fn) {
    if (n <= 0) return;
    if (width <= 1 || n == 1) { for (int i = 0; i < n; i++) fn(i); return; }
    std::lock_guard<std::mutex> job(job_mtx_);
    std::function<void(int)> f = fn;
    {
      std::lock_guard<std::mutex> l(mtx_);
      const int want = std::min(std::min(width - 1, n - 1), 31);
      while ((int)workers_.size() < want) spawn();
      fn_ = &f; n_ = n; next_.store(0); active_ = want; pending_ = want; gen_++;
    }
    cv_.notify_all();
    for (;;) { const int i = next_.fetch_add(1); if (i >= n) break; f(i); }
    std::unique_lock<std::mutex> l(mtx_);
    done_.wait(l, [&] { return pending_ == 0; });
    fn_ = nullptr;
  }
 private:
  std::mutex job_mtx_, mtx_;
  std::condition_variable cv_, done_;
  std::vector<std::thread> workers_;
  const std::function<void(int)>* fn_ = nullptr;
  int n_ = 0, active_ = 0, pending_ = 0;
  std::atomic<int> next_{0};
  unsigned long gen_ = 0;
  void spawn() {
    const int id = (int)workers_.size();
    workers_.emplace_back([this, id] {
      unsigned long seen = 0;
      for (;;) {
        std::unique_lock<std::mutex> l(mtx_);
        cv_.wait(l, [&] { return gen_ != seen && id < active_; });
        seen = gen_;
        const std::function<void(int)>* f = fn_;
        const int n = n_;
        l.unlock();
        for (;;) { const int i = next_.fetch_add(1); if (i >= n) break; (*f)(i); }
        l.lock();
        if (--pending_ == 0) done_.notify_one();
      }
    });
    workers_.back().detach();
  }
};
}  // namespace

namespace {
// dvmh_track_with_motion_model_batch and _cam: model as in track_with_motion_model
int track_with_motion_model_batch(dvm_tracker* t, dvm_orb* h, int device, int count, const uint8_t* imgs, int rows, int cols, int stride, int64_t frame_stride,
                                  int lap0, int lap1, const float* K, const dvm_camera_model* model, const float* bounds, const float* scale_factors,
                                  const float* inv_level_sigma2, int nlevels, float th, int check_ori, const dvmh_track_in* in, const dvmh_track_out* outs,
                                  dvmh_track_result* res) {
  if (!t || !h || !K || !bounds || !scale_factors || !inv_level_sigma2 || !in || !outs || !res || count < 1) return DVM_ERR_INVALID;
  for (int b = 0; b < count; b++) {
    if (!in[b].Tcw_pred || (in[b].Nl && (!in[b].kps_l || !in[b].mp_l || !in[b].mps)) || !outs[b].kps || !outs[b].desc || !outs[b].mp_c || !outs[b].dropped) return DVM_ERR_INVALID;
    std::memset(&res[b], 0, sizeof(res[b]));
  }
  (void)device;
  static const bool timing = std::getenv("DVM_TRACK_BATCH_TIMING") != nullptr;       // host-side phase times of a tick on stderr
  using clk = std::chrono::steady_clock;
  clk::time_point tp0 = clk::now(), tp1, tp2, tp3, tp4;
  int rc = imgs ? dvm_track_begin_batch(t, h, imgs, count, rows, cols, stride, frame_stride, lap0, lap1) : dvm_track_begin_staged(t, h, count, rows, cols, lap0, lap1);
  if (rc != DVM_OK) return rc;
  tp1 = clk::now();
  std::vector<AgentQueries> AQ((size_t)count);
  // (persistent workers: spawning eight threads per tick and giving each four agents' queries took 0.45 ms of a 1.6 ms tick of 32 frames --
  //  longer than the extraction it was meant to run under)
  auto build_all = [&](float scale, const std::vector<uint8_t>* only) {
    TickPool::get().run(count, 24, [&](int b) { if (!only || (*only)[b]) AQ[b].build(in[b], K, model, bounds, scale_factors, nlevels, scale * th); });
  };
  build_all(1.0f, nullptr);
  tp2 = clk::now();
  std::vector<dvm_track_queries> tq((size_t)count);
  std::vector<dvm_track_frame_out> fo((size_t)count);
  std::vector<dvm_track_result> tr((size_t)count);
  std::vector<std::vector<int32_t>> assign((size_t)count);
  std::vector<std::vector<uint8_t>> outl((size_t)count);
  std::vector<std::vector<dvm_keypoint>> un_local((size_t)count);
  for (int b = 0; b < count; b++) {
    const int cap = outs[b].cap;
    assign[b].resize((size_t)cap); outl[b].resize((size_t)cap);
    dvm_keypoint* un = outs[b].kps_un;
    if (!un) { un_local[b].resize((size_t)cap); un = un_local[b].data(); }
    fo[b] = dvm_track_frame_out{outs[b].kps, outs[b].desc, cap, un, assign[b].data(), outl[b].data(), nullptr};
  }
  std::vector<uint8_t> wide((size_t)count, 0);
  for (int attempt = 0; attempt < 2; attempt++) {
    for (int b = 0; b < count; b++) AQ[b].fill(tq[b], in[b], K, bounds, inv_level_sigma2, nlevels, check_ori);
    if (attempt == 0) tp3 = clk::now();
    rc = dvm_track_finish_batch(t, h, count, tq.data(), fo.data(), tr.data());
    if (rc != DVM_OK) return rc;
    if (attempt == 0) tp4 = clk::now();
    bool any = false;
    if (attempt == 0)
      for (int b = 0; b < count; b++) if (tr[b].status == DVM_TRACK_FEW_MATCHES) { wide[b] = 1; any = true; }
    if (!any) break;
    build_all(2.0f, &wide);          // Tracking.cc:2616-2624: "Not enough matches, wider window search" -- for the frames that need it
  }
  for (int b = 0; b < count; b++) {
    dvmh_track_result* out = &res[b];
    const dvm_track_result& r = tr[b];
    const int N = r.n;
    int32_t* mp_c = outs[b].mp_c; int32_t* dropped = outs[b].dropped;
    out->n = r.n; out->mono_index = r.mono_index; out->n_requeried = r.n_requeried; out->wide_window = wide[b];
    for (int j = 0; j < N; j++) { mp_c[j] = -1; dropped[j] = -1; }
    out->nmatches_search = r.nmatches;
    if (r.status != DVM_TRACK_COMPLETE) {     // not tracked: the matches of the (doubled) search stay as SearchByProjection left them
      for (int j = 0; j < N; j++) if (assign[b][j] >= 0) mp_c[j] = in[b].mp_l[AQ[b].Q.qi[assign[b][j]]];
      out->nmatches = r.nmatches; out->tracked = 0; out->Tcw = *in[b].Tcw_pred;
      for (int k = 0; k < 3; k++) out->pose[k] = (double)in[b].Tcw_pred->t[k];
      for (int k = 0; k < 4; k++) out->pose[3 + k] = (double)in[b].Tcw_pred->q[k];
      continue;
    }
    for (int j = 0; j < N; j++) {
      if (assign[b][j] < 0) continue;
      const int mp = in[b].mp_l[AQ[b].Q.qi[assign[b][j]]];
      if (outl[b][j]) dropped[j] = mp; else mp_c[j] = mp;
    }
    out->nmatches = r.nmatches_after; out->nmatches_map = r.nmatches_map; out->n_inliers = r.n_inliers; out->tracked = 1;
    std::memcpy(out->pose, r.pose, 56);
    for (int k = 0; k < 3; k++) out->Tcw.t[k] = (float)out->pose[k];
    for (int k = 0; k < 4; k++) out->Tcw.q[k] = (float)out->pose[3 + k];
  }
  if (timing) {
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    std::fprintf(stderr, "track batch of %d: begin (images in + enqueue) %.3f  queries %.3f  tables + fill %.3f  finish (wait + results out) %.3f  rest %.3f ms\n", count,
                 ms(tp0, tp1), ms(tp1, tp2), ms(tp2, tp3), ms(tp3, tp4), ms(tp4, clk::now()));
  }
  return DVM_OK;
}
}  // namespace

extern "C" int dvmh_track_with_motion_model_batch(dvm_tracker* t, dvm_orb* h, int device, int count, const uint8_t* imgs, int rows, int cols, int stride,
                                                  int64_t frame_stride, int lap0, int lap1, const float* K, const float* bounds, const float* scale_factors,
                                                  const float* inv_level_sigma2, int nlevels, float th, int check_ori, const dvmh_track_in* in,
                                                  const dvmh_track_out* outs, dvmh_track_result* res) {
  return track_with_motion_model_batch(t, h, device, count, imgs, rows, cols, stride, frame_stride, lap0, lap1, K, nullptr, bounds, scale_factors,
                                       inv_level_sigma2, nlevels, th, check_ori, in, outs, res);
}
extern "C" int dvmh_track_with_motion_model_batch_cam(dvm_tracker* t, dvm_orb* h, int device, int count, const uint8_t* imgs, int rows, int cols,
                                                      int stride, int64_t frame_stride, int lap0, int lap1, const float* K,
                                                      const dvm_camera_model* model, const float* bounds, const float* scale_factors,
                                                      const float* inv_level_sigma2, int nlevels, float th, int check_ori, const dvmh_track_in* in,
                                                      const dvmh_track_out* outs, dvmh_track_result* res) {
  (void)K;
  const float* Km = nullptr; const dvm_camera_model* cam = nullptr;
  const int rc = use_camera_model(t, model, &Km, &cam);
  if (rc != DVM_OK) return rc;
  return track_with_motion_model_batch(t, h, device, count, imgs, rows, cols, stride, frame_stride, lap0, lap1, Km, cam, bounds, scale_factors,
                                       inv_level_sigma2, nlevels, th, check_ori, in, outs, res);
}


// ---- the agents' map points resident on the device (dvm_map_store): the batched call above with LastFrame's map points given as store
// slots.  The host projects nothing: it packs the entry lists (slot, octave, angle of every LastFrame keypoint that holds a point and is no
// outlier) and k_track_queries builds the queries from the store.
extern "C" int dvmh_track_with_motion_model_batch_resident(dvm_tracker* t, dvm_orb* h, int device, int count, const uint8_t* imgs, int rows, int cols,
                                                           int stride, int64_t frame_stride, int lap0, int lap1, const float* K, const float* bounds,
                                                           const float* scale_factors, const float* inv_level_sigma2, int nlevels, float th, int check_ori,
                                                           const dvmh_track_in_resident* in, const dvmh_track_out* outs, dvmh_track_result* res) {
  if (!t || !h || !bounds || !scale_factors || !inv_level_sigma2 || !in || !outs || !res || count < 1) return DVM_ERR_INVALID;
  for (int b = 0; b < count; b++) {
    if (!in[b].Tcw_pred || (in[b].Nl && (!in[b].kps_l || !in[b].mp_l || !in[b].store)) || !outs[b].kps || !outs[b].desc || !outs[b].mp_c || !outs[b].dropped) return DVM_ERR_INVALID;
    std::memset(&res[b], 0, sizeof(res[b]));
  }
  (void)device;
  static const bool timing = std::getenv("DVM_TRACK_BATCH_TIMING") != nullptr;       // host-side phase times of a tick on stderr
  using clk = std::chrono::steady_clock;
  clk::time_point tp0 = clk::now(), tp1, tp2, tp3, tp4;
  int rc = imgs ? dvm_track_begin_batch(t, h, imgs, count, rows, cols, stride, frame_stride, lap0, lap1) : dvm_track_begin_staged(t, h, count, rows, cols, lap0, lap1);
  if (rc != DVM_OK) return rc;
  tp1 = clk::now();
  // the entry lists: 9 bytes per entry, in keypoint order
  struct Entries { std::vector<int32_t> slot; std::vector<uint8_t> octave; std::vector<float> angle; int bad = 0; };
  std::vector<Entries> E((size_t)count);
  TickPool::get().run(count, 24, [&](int b) {
    const dvmh_track_in_resident& a = in[b];
    Entries& e = E[b];
    e.slot.reserve((size_t)a.Nl); e.octave.reserve((size_t)a.Nl); e.angle.reserve((size_t)a.Nl);
    for (int i = 0; i < a.Nl; i++) {
      if (a.mp_l[i] < 0) continue;
      if (a.outlier_l && a.outlier_l[i]) continue;
      const int oct = a.kps_l[i].octave;
      if (oct < 0 || oct >= nlevels) { e.bad = 1; return; }
      e.slot.push_back(a.mp_l[i]); e.octave.push_back((uint8_t)oct); e.angle.push_back(a.kps_l[i].angle);
    }
  });
  for (int b = 0; b < count; b++) if (E[b].bad) return DVM_ERR_INVALID;      // (a LastFrame octave outside the level tables)
  tp2 = clk::now();
  dvm_track_shared sh;
  std::memset(&sh, 0, sizeof(sh));
  std::memcpy(sh.bounds, bounds, 16);
  sh.dist = nullptr; sh.scale_factors = scale_factors; sh.inv_level_sigma2 = inv_level_sigma2; sh.nlevels = nlevels;
  if (K) { sh.cam.fx = K[0]; sh.cam.fy = K[1]; sh.cam.cx = K[2]; sh.cam.cy = K[3]; }     // (not read under a KannalaBrandt8 tracker)
  sh.cam.huber_delta = 0.0;
  sh.th_high = TH_HIGH; sh.check_ori = check_ori; sh.min_matches = 20;
  std::vector<dvm_track_last> last((size_t)count);
  std::vector<dvm_track_frame_out> fo((size_t)count);
  std::vector<dvm_track_result> tr((size_t)count);
  std::vector<std::vector<int32_t>> assign((size_t)count);
  std::vector<std::vector<uint8_t>> outl((size_t)count);
  std::vector<std::vector<dvm_keypoint>> un_local((size_t)count);
  for (int b = 0; b < count; b++) {
    const int cap = outs[b].cap;
    assign[b].resize((size_t)cap); outl[b].resize((size_t)cap);
    dvm_keypoint* un = outs[b].kps_un;
    if (!un) { un_local[b].resize((size_t)cap); un = un_local[b].data(); }
    fo[b] = dvm_track_frame_out{outs[b].kps, outs[b].desc, cap, un, assign[b].data(), outl[b].data(), nullptr};
    dvm_track_last& L = last[b];
    L.store = in[b].store; L.n = (int32_t)E[b].slot.size(); L.slot = E[b].slot.data(); L.octave = E[b].octave.data(); L.angle = E[b].angle.data();
    L.Tcw_pred = *in[b].Tcw_pred; L.th = th;
  }
  std::vector<uint8_t> wide((size_t)count, 0);
  for (int attempt = 0; attempt < 2; attempt++) {
    if (attempt == 0) tp3 = clk::now();
    rc = dvm_track_finish_batch_resident(t, h, count, last.data(), &sh, fo.data(), tr.data());
    if (rc != DVM_OK) return rc;
    if (attempt == 0) tp4 = clk::now();
    bool any = false;
    if (attempt == 0)
      for (int b = 0; b < count; b++) if (tr[b].status == DVM_TRACK_FEW_MATCHES) { wide[b] = 1; any = true; last[b].th = 2.0f * th; }
    if (!any) break;                 // Tracking.cc:2616-2624: "Not enough matches, wider window search" -- th changes, nothing is rebuilt here
  }
  for (int b = 0; b < count; b++) {
    dvmh_track_result* out = &res[b];
    const dvm_track_result& r = tr[b];
    const int N = r.n;
    const int32_t* slot = E[b].slot.data();
    int32_t* mp_c = outs[b].mp_c; int32_t* dropped = outs[b].dropped;
    out->n = r.n; out->mono_index = r.mono_index; out->n_requeried = r.n_requeried; out->wide_window = wide[b];
    for (int j = 0; j < N; j++) { mp_c[j] = -1; dropped[j] = -1; }
    out->nmatches_search = r.nmatches;
    if (r.status != DVM_TRACK_COMPLETE) {     // not tracked: the matches of the (doubled) search stay as SearchByProjection left them
      for (int j = 0; j < N; j++) if (assign[b][j] >= 0) mp_c[j] = slot[assign[b][j]];
      out->nmatches = r.nmatches; out->tracked = 0; out->Tcw = *in[b].Tcw_pred;
      for (int k = 0; k < 3; k++) out->pose[k] = (double)in[b].Tcw_pred->t[k];
      for (int k = 0; k < 4; k++) out->pose[3 + k] = (double)in[b].Tcw_pred->q[k];
      continue;
    }
    for (int j = 0; j < N; j++) {
      if (assign[b][j] < 0) continue;
      const int mp = slot[assign[b][j]];
      if (outl[b][j]) dropped[j] = mp; else mp_c[j] = mp;
    }
    out->nmatches = r.nmatches_after; out->nmatches_map = r.nmatches_map; out->n_inliers = r.n_inliers; out->tracked = 1;
    std::memcpy(out->pose, r.pose, 56);
    for (int k = 0; k < 3; k++) out->Tcw.t[k] = (float)out->pose[k];
    for (int k = 0; k < 4; k++) out->Tcw.q[k] = (float)out->pose[3 + k];
  }
  if (timing) {
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    std::fprintf(stderr, "track batch of %d (resident): begin (images in + enqueue) %.3f  entry lists %.3f  fill %.3f  finish (wait + results out) %.3f  rest %.3f ms\n", count,
                 ms(tp0, tp1), ms(tp1, tp2), ms(tp2, tp3), ms(tp3, tp4), ms(tp4, clk::now()));
  }
  return DVM_OK;
}

// The loop header of SearchByProjection(CurrentFrame, LastFrame) on the host for a list of entries whose map points are given as records:
// dvm_host::BuildFrameQueries plus the three per-query arrays of the tracked-frame calls above, the counterpart of k_track_queries
// (dvm_track_debug_build_queries).  Returns nq.
extern "C" int dvmh_build_frame_queries(const dvm_se3f* Tcw_pred, const float* K, const dvm_camera_model* model, const float* bounds,
                                        const float* scale_factors, int nlevels, int n, const int32_t* slot, const dvm_local_point* records,
                                        const uint8_t* octave, const float* angle, float th, int32_t* q_entry, float* qx, float* qy, float* qr,
                                        int32_t* qmin, int32_t* qmax, uint8_t* q_claims, float* q_angle, float* q_pos, uint8_t* qdesc) {
  if (!Tcw_pred || !bounds || !scale_factors || n < 0 || (!K && !model) || (n && (!records || !octave || !angle || !q_entry || !qx || !qy || !qr ||
      !qmin || !qmax || !q_claims || !q_angle || !q_pos || !qdesc)))
    return DVM_ERR_INVALID;
  if (model && !dvm_cam::model_ok(model->model, model->p)) return DVM_ERR_INVALID;
  if (model) K = model->p;
  std::vector<dvm_keypoint> kps((size_t)n);
  std::vector<int32_t> mp_l((size_t)n);
  std::vector<dvmh_map_point> mps((size_t)n);
  for (int i = 0; i < n; i++) {
    if ((int)octave[i] >= nlevels) return DVM_ERR_INVALID;
    const dvm_local_point& r = records[slot ? slot[i] : i];
    std::memset(&kps[i], 0, sizeof(kps[i]));
    kps[i].octave = octave[i]; kps[i].angle = angle[i];
    mp_l[i] = i;
    std::memcpy(mps[i].pos, r.pos, 12); std::memcpy(mps[i].desc, r.desc, 32); mps[i].n_obs = r.n_obs;
  }
  FrameView C, L;
  C.N = 0; C.Tcw = *Tcw_pred;
  C.fx = K[0]; C.fy = K[1]; C.cx = K[2]; C.cy = K[3];
  C.mpCamera = model && model->model == dvm_cam::kKannalaBrandt8 ? model : nullptr;
  C.mnMinX = bounds[0]; C.mnMaxX = bounds[1]; C.mnMinY = bounds[2]; C.mnMaxY = bounds[3];
  C.mvScaleFactors = scale_factors; C.nLevels = nlevels;
  L = C;
  L.N = n; L.mvKeysUn = kps.data(); L.mvpMapPoints = mp_l.data(); L.mvbOutlier = nullptr;
  FrameQueries Q;
  dvm_host::BuildFrameQueries(C, L, mps.data(), th, Q);
  const int nq = (int)Q.qi.size();
  for (int q = 0; q < nq; q++) {
    const int i = Q.qi[q], mp = mp_l[i];
    q_entry[q] = i; qx[q] = Q.qx[q]; qy[q] = Q.qy[q]; qr[q] = Q.qr[q]; qmin[q] = Q.qmin[q]; qmax[q] = Q.qmax[q];
    q_claims[q] = mps[mp].n_obs > 0;
    q_angle[q] = kps[i].angle;
    q_pos[3 * q] = mps[mp].pos[0]; q_pos[3 * q + 1] = mps[mp].pos[1]; q_pos[3 * q + 2] = mps[mp].pos[2];
    std::memcpy(qdesc + 32 * (size_t)q, Q.qdesc.data() + 32 * (size_t)q, 32);
  }
  return nq;
}
