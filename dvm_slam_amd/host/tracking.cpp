// dvm_slam_amd/host/tracking.cpp -- dvmh_track_with_motion_model and its batched and resident forms (include/dvmslam_host.h): the host side
// of the one-chain tracking step.  Reference: Frame::Frame -> ExtractORB (src/Frame.cc:371-411), Tracking::TrackWithMotionModel
// (src/Tracking.cc:2584-2667).
//
// One body, track_frames, runs `count` frames: begin (images or staged) -> the frames' queries built (AgentQueries::build, the one builder)
// or their entry lists packed on the tick pool while the extraction runs -> dvm_track_finish_batch[_resident] -> the wide-window second
// attempt for the frames that need it -> per frame the epilogue (track_settle.h), or the separate calls on the host for a frame the chain
// handed back unfinished (replay_on_host) -> the timing print.  The five extern entry points check their own arguments, describe every
// frame's LastFrame as a LastIn and call it; the single calls are the body with count == 1.
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "dvmslam_host.h"
#include "orb_matcher.h"
#include "track_settle.h"
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

// one frame's LastFrame and map points as the entry points hand them to the body: dvmh_track_in (mps) or dvmh_track_in_resident (store)
struct LastIn {
  const dvm_se3f* Tcw_pred; int Nl; const dvm_keypoint* kps_l; const int32_t* mp_l; const uint8_t* outlier_l;
  const dvmh_map_point* mps; const dvm_map_store* store;
};
// what the frames of a call share
struct TrackShared {
  const float* K; const dvm_camera_model* model;   // model: as use_camera_model leaves *cam
  const float *bounds, *scale_factors, *inv_level_sigma2; int nlevels;
  const dvm_distortion* dist;                      // the single calls': dvm_track_finish_batch takes distortion for one frame
  float th; int check_ori;
};

// ---- the one builder: CurrentFrame (the predicted pose, the camera, no keypoints yet) and LastFrame as SearchByProjection reads them, the
// window queries of LastFrame's map points and the three per-query arrays the chain wants beside them
struct AgentQueries {
  FrameQueries Q;
  std::vector<uint8_t> q_claims;
  std::vector<float> q_angle, q_pos;
  FrameView C, L;
  void build(const dvm_se3f& Tcw_pred, const float* K, const dvm_camera_model* model, const float* bounds, const float* scale_factors, int nlevels, int Nl,
             const dvm_keypoint* kps_l, const int32_t* mp_l, const uint8_t* outlier_l, const dvmh_map_point* mps, float th) {
    C = FrameView();
    C.N = 0; C.Tcw = Tcw_pred;
    C.fx = K[0]; C.fy = K[1]; C.cx = K[2]; C.cy = K[3];
    C.mpCamera = model;            // CurrentFrame.mpCamera->project of LastFrame's points (ORBmatcher.cc:1586), both attempts
    C.mnMinX = bounds[0]; C.mnMaxX = bounds[1]; C.mnMinY = bounds[2]; C.mnMaxY = bounds[3];
    C.mvScaleFactors = scale_factors; C.nLevels = nlevels;
    L = C;
    L.N = Nl; L.mvKeysUn = kps_l; L.mvpMapPoints = const_cast<int32_t*>(mp_l); L.mvbOutlier = outlier_l;
    dvm_host::BuildFrameQueries(C, L, mps, th, Q);
    const int nq = (int)Q.qi.size();
    q_claims.resize((size_t)nq); q_angle.resize((size_t)nq); q_pos.resize((size_t)nq * 3);
    for (int q = 0; q < nq; q++) {
      const int i = Q.qi[q], mp = mp_l[i];
      q_claims[q] = mps[mp].n_obs > 0;
      q_angle[q] = kps_l[i].angle;
      q_pos[3 * q] = mps[mp].pos[0]; q_pos[3 * q + 1] = mps[mp].pos[1]; q_pos[3 * q + 2] = mps[mp].pos[2];
    }
  }
  void fill(dvm_track_queries& tq, const dvm_se3f& Tcw_pred, const TrackShared& S) const {
    std::memset(&tq, 0, sizeof(tq));
    tq.nq = (int)Q.qi.size(); tq.qdesc = Q.qdesc.data(); tq.qx = Q.qx.data(); tq.qy = Q.qy.data(); tq.qr = Q.qr.data(); tq.qmin = Q.qmin.data(); tq.qmax = Q.qmax.data();
    tq.q_claims = q_claims.data(); tq.q_angle = q_angle.data(); tq.q_pos = q_pos.data();
    std::memcpy(tq.bounds, S.bounds, 16);
    tq.dist = S.dist; tq.inv_level_sigma2 = S.inv_level_sigma2; tq.nlevels = S.nlevels;
    tq.cam.fx = S.K[0]; tq.cam.fy = S.K[1]; tq.cam.cx = S.K[2]; tq.cam.cy = S.K[3]; tq.cam.huber_delta = 0.0;
    // g2o::SE3Quat(Tcw.unit_quaternion().cast<double>(), Tcw.translation().cast<double>()) (Optimizer.cc:760)
    for (int k = 0; k < 3; k++) tq.pose_in[k] = (double)Tcw_pred.t[k];
    for (int k = 0; k < 4; k++) tq.pose_in[3 + k] = (double)Tcw_pred.q[k];
    tq.th_high = TH_HIGH; tq.check_ori = S.check_ori; tq.min_matches = 20;
  }
};

// LastFrame's entry lists for the resident finish: slot, octave, angle of every keypoint that holds a point and is no outlier, in keypoint
// order (9 bytes per entry); bad: an octave outside the level tables
struct Entries {
  std::vector<int32_t> slot; std::vector<uint8_t> octave; std::vector<float> angle; int bad = 0;
  void pack(const LastIn& a, int nlevels) {
    slot.reserve((size_t)a.Nl); octave.reserve((size_t)a.Nl); angle.reserve((size_t)a.Nl);
    for (int i = 0; i < a.Nl; i++) {
      if (a.mp_l[i] < 0) continue;
      if (a.outlier_l && a.outlier_l[i]) continue;
      const int oct = a.kps_l[i].octave;
      if (oct < 0 || oct >= nlevels) { bad = 1; return; }
      slot.push_back(a.mp_l[i]); octave.push_back((uint8_t)oct); angle.push_back(a.kps_l[i].angle);
    }
  }
};

// A frame the chain handed back as DVM_TRACK_REPLAY_ON_HOST (a query ran out of ranked candidates and the device did not search its window
// again: only under the DVM_TRACK_NO_REQUERY timing switch): the separate calls take over from the frame's host arrays -- same results by
// construction, they are what the chain is tested against.  A: the frame's views as its last build left them; th_now: that build's th.
int replay_on_host(int device, AgentQueries& A, const LastIn& in, const TrackShared& S, float th_now, const dvm_track_result& r, int wide_window,
                   const dvm_keypoint* kps_un, const uint8_t* desc, int32_t* mp_c, int32_t* dropped, dvmh_track_result* out) {
  dvm_host::settle_begin(r, wide_window, mp_c, dropped, out);
  out->replayed_on_host = 1;
  const int N = r.n;
  FrameView& C = A.C;
  C.N = N; C.mvKeysUn = kps_un; C.mDescriptors = desc; C.mvpMapPoints = mp_c;
  dvm_host::ORBmatcher m(0.9f, S.check_ori != 0, device);
  int nm = m.SearchByProjection(C, A.L, in.mps, th_now, true);
  if (nm < 0) return nm;
  if (nm < 20 && !out->wide_window) {
    for (int j = 0; j < N; j++) mp_c[j] = -1;
    out->wide_window = 1;
    nm = m.SearchByProjection(C, A.L, in.mps, 2 * S.th, true);
    if (nm < 0) return nm;
  }
  out->nmatches_search = nm;
  if (nm < 20) { out->nmatches = nm; out->tracked = 0; out->Tcw = *in.Tcw_pred; return DVM_OK; }
  dvm_track_queries tq;
  A.fill(tq, *in.Tcw_pred, S);           // (pose_in and cam)
  std::vector<double> Xw, obs, w;
  std::vector<int> kp_of;
  for (int j = 0; j < N; j++) {
    if (mp_c[j] < 0) continue;
    for (int k = 0; k < 3; k++) Xw.push_back((double)in.mps[mp_c[j]].pos[k]);
    obs.push_back((double)kps_un[j].x); obs.push_back((double)kps_un[j].y);
    w.push_back((double)S.inv_level_sigma2[kps_un[j].octave]);
    kp_of.push_back(j);
  }
  const int32_t ne = (int32_t)kp_of.size();
  std::vector<uint8_t> rej((size_t)ne);
  int32_t inl = 0;
  const int rc = S.model ? dvm_pose_optimize_cam(device, tq.pose_in, Xw.data(), obs.data(), w.data(), &ne, ne, 1, S.model, out->pose, rej.data(), &inl)
                         : dvm_pose_optimize(device, tq.pose_in, Xw.data(), obs.data(), w.data(), &ne, ne, 1, &tq.cam, out->pose, rej.data(), &inl);
  if (rc != DVM_OK) return rc;
  out->n_inliers = inl;
  int left = nm, nmap = 0;
  for (int e = 0; e < ne; e++) {
    const int j = kp_of[e];
    if (rej[e]) { dropped[j] = mp_c[j]; mp_c[j] = -1; left--; }
    else if (in.mps[mp_c[j]].n_obs > 0) nmap++;
  }
  out->nmatches = left; out->nmatches_map = nmap; out->tracked = 1;
  dvm_host::pose_to_Tcw(out->pose, &out->Tcw);
  return DVM_OK;
}

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

// ---- the one run body: `count` frames through ONE chain of batched launches (dvm_track_begin_batch / dvm_track_finish_batch[_resident]).
// resident: LastFrame's map points are store slots (in[b].store) and the device builds the queries from the entry lists; else they index
// in[b].mps and the host builds them.  imgs NULL: the frames are staged in the extractor's input buffer.
int track_frames(dvm_tracker* t, dvm_orb* h, int device, int count, const uint8_t* imgs, int rows, int cols, int stride, int64_t frame_stride, int lap0, int lap1,
                 const TrackShared& S, bool resident, const LastIn* in, const dvmh_track_out* outs, dvmh_track_result* res) {
  if (!t || !h || (!resident && !S.K) || !S.bounds || !S.scale_factors || !S.inv_level_sigma2 || !in || !outs || !res || count < 1) return DVM_ERR_INVALID;
  for (int b = 0; b < count; b++) {
    if (!in[b].Tcw_pred || (in[b].Nl && (!in[b].kps_l || !in[b].mp_l || !(resident ? (const void*)in[b].store : (const void*)in[b].mps))) || !outs[b].kps ||
        !outs[b].desc || !outs[b].mp_c || !outs[b].dropped)
      return DVM_ERR_INVALID;
    std::memset(&res[b], 0, sizeof(res[b]));
  }
  static const bool timing = std::getenv("DVM_TRACK_BATCH_TIMING") != nullptr;       // host-side phase times of a tick on stderr
  using clk = std::chrono::steady_clock;
  clk::time_point tp0 = clk::now(), tp1, tp2, tp3, tp4;
  // 1. the extraction is on its way ...
  int rc = imgs ? dvm_track_begin_batch(t, h, imgs, count, rows, cols, stride, frame_stride, lap0, lap1) : dvm_track_begin_staged(t, h, count, rows, cols, lap0, lap1);
  if (rc != DVM_OK) return rc;
  tp1 = clk::now();
  // 2. ... while the queries are built (they need LastFrame and the predicted pose only), or the entry lists packed
  // (persistent workers: spawning eight threads per tick and giving each four agents' queries took 0.45 ms of a 1.6 ms tick of 32 frames --
  //  longer than the extraction it was meant to run under)
  std::vector<AgentQueries> AQ(resident ? 0 : (size_t)count);
  std::vector<Entries> E(resident ? (size_t)count : 0);
  auto build_all = [&](float scale, const std::vector<uint8_t>* only) {
    TickPool::get().run(count, 24, [&](int b) {
      if (only && !(*only)[b]) return;
      const LastIn& a = in[b];
      AQ[b].build(*a.Tcw_pred, S.K, S.model, S.bounds, S.scale_factors, S.nlevels, a.Nl, a.kps_l, a.mp_l, a.outlier_l, a.mps, scale * S.th);
    });
  };
  if (resident) {
    TickPool::get().run(count, 24, [&](int b) { E[b].pack(in[b], S.nlevels); });
    for (int b = 0; b < count; b++) if (E[b].bad) return DVM_ERR_INVALID;      // (a LastFrame octave outside the level tables)
  } else {
    build_all(1.0f, nullptr);
  }
  tp2 = clk::now();
  // the chain's per-keypoint outputs of every frame, and mvKeysUn of a frame whose caller wants none (kps_un NULL)
  std::vector<std::vector<int32_t>> assign((size_t)count);
  std::vector<std::vector<uint8_t>> outl((size_t)count);
  std::vector<std::vector<dvm_keypoint>> un_local((size_t)count);
  std::vector<dvm_track_frame_out> fo((size_t)count);
  std::vector<dvm_track_result> tr((size_t)count);
  std::vector<dvm_track_queries> tq(resident ? 0 : (size_t)count);
  std::vector<dvm_track_last> last(resident ? (size_t)count : 0);
  dvm_track_shared sh;
  for (int b = 0; b < count; b++) {
    const int cap = outs[b].cap;
    assign[b].resize((size_t)cap); outl[b].resize((size_t)cap);
    dvm_keypoint* un = outs[b].kps_un;
    if (!un) { un_local[b].resize((size_t)cap); un = un_local[b].data(); }
    fo[b] = dvm_track_frame_out{outs[b].kps, outs[b].desc, cap, un, assign[b].data(), outl[b].data(), nullptr};
  }
  if (resident) {
    std::memset(&sh, 0, sizeof(sh));
    std::memcpy(sh.bounds, S.bounds, 16);
    sh.dist = S.dist; sh.scale_factors = S.scale_factors; sh.inv_level_sigma2 = S.inv_level_sigma2; sh.nlevels = S.nlevels;
    if (S.K) { sh.cam.fx = S.K[0]; sh.cam.fy = S.K[1]; sh.cam.cx = S.K[2]; sh.cam.cy = S.K[3]; }     // (not read under a KannalaBrandt8 tracker)
    sh.cam.huber_delta = 0.0;
    sh.th_high = TH_HIGH; sh.check_ori = S.check_ori; sh.min_matches = 20;
    for (int b = 0; b < count; b++) {
      dvm_track_last& L = last[b];
      L.store = in[b].store; L.n = (int32_t)E[b].slot.size(); L.slot = E[b].slot.data(); L.octave = E[b].octave.data(); L.angle = E[b].angle.data();
      L.Tcw_pred = *in[b].Tcw_pred; L.th = S.th;
    }
  }
  // 3. the chain; then once more for the frames below 20 matches (Tracking.cc:2616-2624: "Not enough matches, wider window search": their
  //    queries rebuilt at the doubled th -- resident: th changes, nothing is rebuilt here; no new extraction)
  std::vector<uint8_t> wide((size_t)count, 0);
  for (int attempt = 0; attempt < 2; attempt++) {
    for (int b = 0; b < count && !resident; b++) AQ[b].fill(tq[b], *in[b].Tcw_pred, S);
    if (attempt == 0) tp3 = clk::now();
    rc = resident ? dvm_track_finish_batch_resident(t, h, count, last.data(), &sh, fo.data(), tr.data())
                  : dvm_track_finish_batch(t, h, count, tq.data(), fo.data(), tr.data());
    if (rc != DVM_OK) return rc;
    if (attempt == 0) tp4 = clk::now();
    bool any = false;
    if (attempt == 0)
      for (int b = 0; b < count; b++) if (tr[b].status == DVM_TRACK_FEW_MATCHES) { wide[b] = 1; any = true; if (resident) last[b].th = 2.0f * S.th; }
    if (!any) break;
    // (all frames run again, a frame handed back as DVM_TRACK_REPLAY_ON_HOST too, with the same result; replay_on_host below relies on
    //  AQ[b] being rebuilt only where wide[b] is set: its th_now is 2 * th exactly for those frames)
    if (!resident) build_all(2.0f, &wide);
  }
  // 4. per frame: the epilogue, or the replay.  (The resident form has no host map points to replay from: a frame handed back as
  //    DVM_TRACK_REPLAY_ON_HOST is settled as not tracked, the matches as the chain left them.)
  for (int b = 0; b < count; b++) {
    if (!resident && tr[b].status == DVM_TRACK_REPLAY_ON_HOST) {
      rc = replay_on_host(device, AQ[b], in[b], S, wide[b] ? 2 * S.th : S.th, tr[b], wide[b], fo[b].kps_un, outs[b].desc, outs[b].mp_c, outs[b].dropped, &res[b]);
      if (rc != DVM_OK) return rc;
      continue;
    }
    if (resident)
      dvm_host::settle_tracked_frame(tr[b], fo[b].assign, fo[b].outlier, dvm_host::SlotIds{E[b].slot.data()}, *in[b].Tcw_pred, wide[b], outs[b].mp_c, outs[b].dropped, &res[b]);
    else
      dvm_host::settle_tracked_frame(tr[b], fo[b].assign, fo[b].outlier, dvm_host::HostIds{in[b].mp_l, AQ[b].Q.qi.data()}, *in[b].Tcw_pred, wide[b], outs[b].mp_c, outs[b].dropped,
                                     &res[b]);
  }
  if (timing) {
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    std::fprintf(stderr, resident ? "track batch of %d (resident): begin (images in + enqueue) %.3f  entry lists %.3f  fill %.3f  finish (wait + results out) %.3f  rest %.3f ms\n"
                                  : "track batch of %d: begin (images in + enqueue) %.3f  queries %.3f  tables + fill %.3f  finish (wait + results out) %.3f  rest %.3f ms\n",
                 count, ms(tp0, tp1), ms(tp1, tp2), ms(tp2, tp3), ms(tp3, tp4), ms(tp4, clk::now()));
  }
  return DVM_OK;
}

// dvmh_track_with_motion_model and _cam: the body on one frame.  model NULL: the pinhole camera K; else as use_camera_model left it
int track_one(dvm_tracker* t, dvm_orb* h, int device, const uint8_t* img, int rows, int cols, int stride, int lap0, int lap1, const dvm_se3f* Tcw_pred,
              const float* K, const dvm_camera_model* model, const float* bounds, const dvm_distortion* dist, const float* scale_factors,
              const float* inv_level_sigma2, int nlevels, int Nl, const dvm_keypoint* kps_l, const int32_t* mp_l, const uint8_t* outlier_l,
              const dvmh_map_point* mps, float th, int check_ori, dvm_keypoint* kps, uint8_t* desc, int cap, dvm_keypoint* kps_un, int32_t* mp_c,
              int32_t* dropped, dvmh_track_result* out) {
  if (!img || !K) return DVM_ERR_INVALID;      // (a NULL image is the batch's "staged"; the rest is checked by the body)
  const TrackShared S{K, model, bounds, scale_factors, inv_level_sigma2, nlevels, dist, th, check_ori};
  const LastIn in{Tcw_pred, Nl, kps_l, mp_l, outlier_l, mps, nullptr};
  const dvmh_track_out o{kps, desc, cap, kps_un, mp_c, dropped};
  return track_frames(t, h, device, 1, img, rows, cols, stride, (int64_t)rows * stride, lap0, lap1, S, false, &in, &o, out);
}

// dvmh_track_with_motion_model_batch and _cam: model as in track_one
int track_batch(dvm_tracker* t, dvm_orb* h, int device, int count, const uint8_t* imgs, int rows, int cols, int stride, int64_t frame_stride, int lap0, int lap1,
                const float* K, const dvm_camera_model* model, const float* bounds, const float* scale_factors, const float* inv_level_sigma2, int nlevels,
                float th, int check_ori, const dvmh_track_in* in, const dvmh_track_out* outs, dvmh_track_result* res) {
  if (!in || !K || count < 1) return DVM_ERR_INVALID;
  std::vector<LastIn> li((size_t)count);
  for (int b = 0; b < count; b++) li[b] = LastIn{in[b].Tcw_pred, in[b].Nl, in[b].kps_l, in[b].mp_l, in[b].outlier_l, in[b].mps, nullptr};
  const TrackShared S{K, model, bounds, scale_factors, inv_level_sigma2, nlevels, nullptr, th, check_ori};
  return track_frames(t, h, device, count, imgs, rows, cols, stride, frame_stride, lap0, lap1, S, false, li.data(), outs, res);
}
}  // namespace

extern "C" int dvmh_track_with_motion_model(dvm_tracker* t, dvm_orb* h, int device, const uint8_t* img, int rows, int cols, int stride, int lap0,
                                            int lap1, const dvm_se3f* Tcw_pred, const float* K, const float* bounds, const dvm_distortion* dist,
                                            const float* scale_factors, const float* inv_level_sigma2, int nlevels, int Nl,
                                            const dvm_keypoint* kps_l, const int32_t* mp_l, const uint8_t* outlier_l, const dvmh_map_point* mps,
                                            float th, int check_ori, dvm_keypoint* kps, uint8_t* desc, int cap, dvm_keypoint* kps_un,
                                            int32_t* mp_c, int32_t* dropped, dvmh_track_result* out) {
  return track_one(t, h, device, img, rows, cols, stride, lap0, lap1, Tcw_pred, K, nullptr, bounds, dist, scale_factors, inv_level_sigma2, nlevels, Nl, kps_l,
                   mp_l, outlier_l, mps, th, check_ori, kps, desc, cap, kps_un, mp_c, dropped, out);
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
  return track_one(t, h, device, img, rows, cols, stride, lap0, lap1, Tcw_pred, Km, cam, bounds, dist, scale_factors, inv_level_sigma2, nlevels, Nl, kps_l,
                   mp_l, outlier_l, mps, th, check_ori, kps, desc, cap, kps_un, mp_c, dropped, out);
}

// ---- K agents' frames at one camera tick: per frame exactly the steps of the single call
extern "C" int dvmh_track_with_motion_model_batch(dvm_tracker* t, dvm_orb* h, int device, int count, const uint8_t* imgs, int rows, int cols, int stride,
                                                  int64_t frame_stride, int lap0, int lap1, const float* K, const float* bounds, const float* scale_factors,
                                                  const float* inv_level_sigma2, int nlevels, float th, int check_ori, const dvmh_track_in* in,
                                                  const dvmh_track_out* outs, dvmh_track_result* res) {
  return track_batch(t, h, device, count, imgs, rows, cols, stride, frame_stride, lap0, lap1, K, nullptr, bounds, scale_factors, inv_level_sigma2, nlevels, th,
                     check_ori, in, outs, res);
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
  return track_batch(t, h, device, count, imgs, rows, cols, stride, frame_stride, lap0, lap1, Km, cam, bounds, scale_factors, inv_level_sigma2, nlevels, th,
                     check_ori, in, outs, res);
}

// ---- the agents' map points resident on the device (dvm_map_store): the batched call with LastFrame's map points given as store slots.
// The host projects nothing: it packs the entry lists and k_track_queries builds the queries from the store.
extern "C" int dvmh_track_with_motion_model_batch_resident(dvm_tracker* t, dvm_orb* h, int device, int count, const uint8_t* imgs, int rows, int cols,
                                                           int stride, int64_t frame_stride, int lap0, int lap1, const float* K, const float* bounds,
                                                           const float* scale_factors, const float* inv_level_sigma2, int nlevels, float th, int check_ori,
                                                           const dvmh_track_in_resident* in, const dvmh_track_out* outs, dvmh_track_result* res) {
  if (!in || count < 1) return DVM_ERR_INVALID;
  std::vector<LastIn> li((size_t)count);
  for (int b = 0; b < count; b++) li[b] = LastIn{in[b].Tcw_pred, in[b].Nl, in[b].kps_l, in[b].mp_l, in[b].outlier_l, nullptr, in[b].store};
  const TrackShared S{K, nullptr, bounds, scale_factors, inv_level_sigma2, nlevels, nullptr, th, check_ori};
  return track_frames(t, h, device, count, imgs, rows, cols, stride, frame_stride, lap0, lap1, S, true, li.data(), outs, res);
}

// The loop header of SearchByProjection(CurrentFrame, LastFrame) on the host for a list of entries whose map points are given as records:
// the builder above on a LastFrame made of the entries, the counterpart of k_track_queries (dvm_track_debug_build_queries).  Returns nq.
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
  AgentQueries A;
  A.build(*Tcw_pred, K, model && model->model == dvm_cam::kKannalaBrandt8 ? model : nullptr, bounds, scale_factors, nlevels, n, kps.data(), mp_l.data(), nullptr,
          mps.data(), th);
  const FrameQueries& Q = A.Q;
  const size_t nq = Q.qi.size();
  for (size_t q = 0; q < nq; q++) q_entry[q] = Q.qi[q];
  if (nq) {
    std::memcpy(qx, Q.qx.data(), nq * 4); std::memcpy(qy, Q.qy.data(), nq * 4); std::memcpy(qr, Q.qr.data(), nq * 4);
    std::memcpy(qmin, Q.qmin.data(), nq * 4); std::memcpy(qmax, Q.qmax.data(), nq * 4); std::memcpy(qdesc, Q.qdesc.data(), nq * 32);
    std::memcpy(q_claims, A.q_claims.data(), nq); std::memcpy(q_angle, A.q_angle.data(), nq * 4); std::memcpy(q_pos, A.q_pos.data(), nq * 12);
  }
  return (int)nq;
}
