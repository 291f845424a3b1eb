// dvm_slam_amd/csrc/track.cpp -- dvm_tracker: ONE enqueue per tracked frame (include/dvmslam_hip.h, "tracking step").
//
// The reference's per-frame hot loop is Frame::Frame -> ExtractORB (src/Frame.cc:371-411) followed by
// Tracking::TrackWithMotionModel (src/Tracking.cc:2584-2667): SearchByProjection(CurrentFrame, LastFrame) (src/ORBmatcher.cc:1553-1748)
// -> Optimizer::PoseOptimization (src/Optimizer.cc:744-1028) -> outlier matches dropped.  Through the three separate calls of this
// library that is three blocking host <-> device round trips with the claim replay, the rotation histogram and the edge gathering on
// the host in between.  Here the whole step is one chain on the extractor's stream:
//   dvm_track_begin    queues the extraction of the frame and returns (the host builds the projection queries meanwhile: they need
//                      LastFrame's map points and the predicted pose, nothing of the new frame)
//   dvm_track_finish   queues [undistortion] -> grid (k_frame_build) -> ranked window search -> k_track_claims -> k_track_gather ->
//                      k_pose_optimize -> k_track_finish behind it, synchronises ONCE and hands everything back
// Results are those of the separate calls bit for bit (tests/test_gpu_track_frame.py).  Two cases are handed back to the caller
// unfinished, flagged in dvm_track_result::status: fewer than min_matches matches (the reference searches again with a doubled window,
// Tracking.cc:2616-2624: call dvm_track_finish again with the wider queries -- no new extraction), and a query whose four ranked
// candidates were all taken by earlier queries (the list may go on: the caller replays the epilogue from the ranked lists on the host).
// The second half (dvm_track_local_map, dvm_track_reference_keyframe) runs as the batch of one frame: the single calls keep their own
// checks and run the chains of dvm_track_local_map_batch / dvm_track_reference_keyframe_batch.
// Both halves also read an agent's map points where they live on the device (dvm_map_store, map_store.cpp): dvm_track_finish_batch_resident
// takes LastFrame's entry lists (slot, octave, angle: 9 B per entry) and k_track_queries builds the query block from the store, beside the
// extraction; dvm_track_local_map_batch_resident takes the tables as slot lists and k_store_gather fills the chain's device table.  Every
// slot is checked on the host against its store before anything is queued.  Behind the query block / the table the chains are the same.
// Every reservation here is a WorkingSet (chain.h, shared with the other chains) whose layout is written once, as a carve_* function of
// track_layout.h: create / reserve_* measure it on a null base at the largest arguments, each call carves the same function at its own
// shape.  Both first-half finishes are finish_run, the three second-half entry points fill a LocalSource per frame and run local_map_run,
// both begins are begin_run; the entry points differ in their argument checks and in what they name in an error.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/dvmslam_hip.h"
#include "ba_kernels.h"
#include "camera_model.h"
#include "chain.h"
#include "match_kernels.h"
#include "orb_pipeline.h"
#include "host_stage.h"   // HostPool
#include "keyframe_store.h"
#include "map_store.h"
#include "track_kernels.h"
#include "track_layout.h"

using namespace dvm;

// what the second half runs on: set by a dvm_track_finish[_batch] that returned DVM_OK, cleared by any begin / finish and by the second
// half itself.  ready: one frame that returned DVM_TRACK_COMPLETE (dvm_track_local_map); batch_ready: any finish (dvm_track_local_map_batch);
// rkb_ready: any finish, until dvm_track_reference_keyframe_batch, the single call or the second half runs on it
struct LocalFrame {
  int ready = 0, batch_ready = 0, rkb_ready = 0;
  int kf_ready = 0;                              // the frames may be promoted (dvm_keyframe_store_put_tracked): set with the fields below, cleared by a begin ONLY
  dvm_orb* h = nullptr; uint64_t serial = 0;     // the extractor and which of its extractions the frame is
  int ocap = 0, nlevels = 0;
  const dvm_keypoint_pod* d_un = nullptr; const int32_t* d_n = nullptr;   // mvKeysUn on the device, the keypoint count
  float bounds[4] = {0, 0, 0, 0}, inv_sigma2[64] = {};
  dvm_ba_camera cam{};
  dvm_camera_model model{};                       // the camera model that finish ran on (dvm_tracker_set_camera_model): the second half runs on it
  int count = 0; int64_t kps_stride = 0;          // the finish's frames: frame b's mvKeysUn at b * kps_stride, its count at d_n[b]
  std::vector<int32_t> ns, status;                // per frame: keypoints, the first half's status
  std::vector<double> poses;                      // [count][7]: the poses the second half starts from (the finish's, or the reference-keyframe chain's)
  std::vector<int32_t> monos;                     // per frame: monoIndex of the extraction
  const uint8_t* d_desc = nullptr; int64_t desc_stride = 0;   // the frames' descriptors on the device: frame b's at b * desc_stride
};

// a TrackReferenceKeyFrame working set: per-frame arrays for the tracker's max_frames frames at its keypoint capacity, keyframes of up to
// `cap` entries per call (each keyframe's rounded up to 64)
struct RefKf {
  WorkingSet ws;                   // device: [upload copy][the frames' transforms, FeatureVectors and match state]; mapped: [upload staging][results]
  int cap = 0;
  RefKfMapped r;                   // [max_frames] slices of the results
};

struct dvm_tracker {
  int device = 0, kp_cap = 0, q_cap = 0, max_frames = 1;
  int q_rcap = 0;                  // q_cap rounded up to 64: the per-frame query capacity of the query block and the ranked lists
  dvm_frame* grid = nullptr;       // max_frames slots
  WorkingSet ws;                   // first half.  device: dv; mapped: [the query block, staging of the one copy: q_bytes][results m]
  TrackerDevice dv{};
  TrackerResults m{};
  // the query block: carved per call (stride = the call's largest nq), built in the mapped buffer (page-locked), copied to the device by
  // ONE asynchronous copy on a side stream while the extraction runs; the kernels read the device copy dv.q (the one-wave claim replay walks
  // it serially: a PCIe read per step would be its chain).  qb: the last call's carve of the mapped buffer.
  QueryBlock qb{};
  size_t q_bytes = 0;              // the block at max_frames frames of q_rcap queries
  hipStream_t cstream = nullptr; hipEvent_t cev = nullptr;
  template <class T> T* qdev(T* host_ptr) const { return rebase(host_ptr, ws.hm, dv.q); }
  int begun = 0;                   // frames of the batch whose extraction is queued
  dvm_camera_model model{};        // dvm_tracker_set_camera_model: 0 (a fresh tracker): the cam of the query / parameter structs; 1: KannalaBrandt8 on model.p
  int rows = 0, cols = 0;
  // ---- the resident first half (dvm_track_finish_batch_resident): the entry lists go up through rw, k_track_queries writes dv.q
  WorkingSet rw;                   // device: the upload copy; mapped: rm
  ResidentMapped rm{};             // mapped: the entry number of every query (max_frames x q_rcap), the frames' query counts
  int64_t up_first = 0, up_second = 0;           // dvm_tracker_last_upload_bytes: what the last finish / local-map call copied up
  int64_t up_refkf = 0;                          // dvm_tracker_last_refkf_upload_bytes: what the last reference-keyframe call copied up
  // ---- the second half (dvm_track_local_map[_batch]): working set of dvm_tracker_reserve_local_map, and what the last finish left for it
  int lm_cap = 0;                  // table entries reserved (a multiple of 64; a batch: all frames' tables, each rounded up to 64)
  WorkingSet lmw;                  // device: [upload region][carve_local_map_work]; mapped: [upload staging][results lm]
  LocalMapResults lm{};            // [max_frames]
  LocalFrame lf;
  // ---- TrackReferenceKeyFrame: the working sets of dvm_tracker_reserve_reference_keyframe (rk, one frame) and of
  //      dvm_tracker_reserve_reference_keyframe_batch (rkb), and when the single call dvm_track_reference_keyframe may run
  int rk_state = 0;                // 1: right after a single-frame begin (form a), 2: right after that frame's finish (form b), else 0
  dvm_orb* rk_h = nullptr; uint64_t rk_serial = 0;   // the extractor and which of its extractions the frame is
  int rk_cap = 0;                  // keyframe keypoints the single call takes (rk.cap: this rounded up to 64)
  RefKf rk, rkb;
  // nothing of the second half may run until the next finish (or begin, for the single reference-keyframe call)
  void clear_next() { lf.ready = 0; lf.batch_ready = 0; lf.rkb_ready = 0; rk_state = 0; }
};

namespace dvm {
uint64_t orb_result_serial(const dvm_orb* h);   // capi.cpp: which extraction the handle's result holds
int vocab_device(const dvm_vocab* v);           // capi.cpp: the vocabulary's device and its transform of device features (count on the device)
void vocab_launch_transform(const dvm_vocab* v, hipStream_t s, const uint8_t* d_feat, int cap, const int32_t* d_n, int levelsup, int32_t* word_id,
                            int32_t* node_id, double* weight, const int32_t* run = nullptr, int nrun = 1, int64_t feat_stride = 0);
}

namespace {
// a reservation that could not be allocated: "<fn>: <what failed>"
int reserve_failed(const char* fn, const char* what) { set_error(std::string(fn) + ": " + what); return DVM_ERR_CAPACITY; }
// PoseOptimization of a chain: k_pose_optimize on cam, or k_pose_optimize_kb8 on M.p under a KannalaBrandt8 model (cam is then not read)
void launch_pose_optimize(hipStream_t s, const dvm_camera_model& M, const dvm_ba_camera& cam, const double* pose_in, const double* Xw, const double* obs,
                          const double* info, const int32_t* n_per_frame, int stride, int batch, double* pose_out, uint8_t* outlier, int32_t* n_inliers,
                          double* chi_scratch) {
  if (M.model == dvm_cam::kKannalaBrandt8)
    ba_launch_pose_optimize_kb8(s, pose_in, Xw, obs, info, n_per_frame, stride, batch, M.p, pose_out, outlier, n_inliers, chi_scratch);
  else
    ba_launch_pose_optimize(s, pose_in, Xw, obs, info, n_per_frame, stride, batch, cam.fx, cam.fy, cam.cx, cam.cy, pose_out, outlier, n_inliers, chi_scratch);
}
// a KannalaBrandt8 frame has mvKeysUn = mvKeys and a zero mDistCoef: distortion coefficients beside such a model are a caller's mistake
bool kb8_with_distortion(const dvm_camera_model& M, const dvm_distortion* dist) { return M.model == dvm_cam::kKannalaBrandt8 && dist && dist->k1 != 0.0f; }
}  // namespace

extern "C" {

int dvm_tracker_create_batch(int device, int max_frames, int max_keypoints, int max_queries, dvm_tracker** out) {
  if (!out || max_keypoints < 1 || max_queries < 1 || max_frames < 1 || max_frames > 256) return DVM_ERR_INVALID;
  *out = nullptr;
  if (max_keypoints > kFrameCap || max_queries > kFrameCap || track_claims_lds(max_keypoints, max_queries) > 150 * 1024) {
    set_error("dvm_tracker_create: capacity beyond what the claim replay keeps in LDS (9 B per keypoint + 21 B per query <= 150 KB)");
    return DVM_ERR_CAPACITY;
  }
  { const int rc = need_device(device); if (rc != DVM_OK) return rc; }
  dvm_tracker* t = new (std::nothrow) dvm_tracker();
  if (!t) return DVM_ERR_INVALID;
  t->device = device; t->kp_cap = max_keypoints; t->q_cap = max_queries; t->max_frames = max_frames; t->q_rcap = (max_queries + 63) & ~63;
  int rc = dvm_frame_create(device, max_keypoints, max_frames, &t->grid);
  if (rc != DVM_OK) { delete t; return rc; }
  // every size from the layouts at the largest call (Q rounded up to 64: dvm_track_finish_batch strides the per-query arrays by the
  // call's largest nq rounded up to 64); the query block's device copy is the device block's last item
  const size_t K = (size_t)max_keypoints, Q = (size_t)t->q_rcap, B = (size_t)max_frames;
  t->q_bytes = carve_query_block(nullptr, B, Q).bytes;
  if (const char* what = t->ws.alloc(carve_tracker_device(nullptr, B, K, Q, t->q_bytes).bytes, t->q_bytes + carve_tracker_results(nullptr, B, K).bytes, t->q_bytes,
                                     /*mapped*/ true, /*zeroed*/ true)) {
    dvm_tracker_destroy(t); set_error(std::string("dvm_tracker_create: ") + what); return DVM_ERR_HIP;
  }
  t->dv = carve_tracker_device(t->ws.d, B, K, Q, t->q_bytes);
  t->m = carve_tracker_results(t->ws.hm + t->q_bytes, B, K);
  {   // the resident first half: 9 bytes per entry (every frame's list rounded up to 64), two level tables, a record per frame
    const ResidentMapped sized = carve_resident_mapped(nullptr, B, Q);
    if (const char* what = t->rw.alloc(sized.up, sized.bytes, sized.up, /*mapped*/ true, /*zeroed*/ true)) {
      dvm_tracker_destroy(t); set_error(std::string("dvm_tracker_create: ") + what); return DVM_ERR_HIP;
    }
    t->rm = carve_resident_mapped(t->rw.hm, B, Q);
  }
  if (hipStreamCreateWithFlags(&t->cstream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&t->cev, hipEventDisableTiming) != hipSuccess) {
    dvm_tracker_destroy(t); set_error("dvm_tracker_create: query block"); return DVM_ERR_HIP;
  }
  *out = t;
  return DVM_OK;
}
int dvm_tracker_create(int device, int max_keypoints, int max_queries, dvm_tracker** out) {
  return dvm_tracker_create_batch(device, 1, max_keypoints, max_queries, out);
}

void dvm_tracker_destroy(dvm_tracker* t) {
  if (!t) return;
  hipSetDevice(t->device);
  if (t->grid) dvm_frame_destroy(t->grid);
  t->lmw.free(); t->rk.ws.free(); t->rkb.ws.free();
  if (t->cev) hipEventDestroy(t->cev);
  if (t->cstream) hipStreamDestroy(t->cstream);
  t->ws.free(); t->rw.free();
  delete t;
}

int dvm_tracker_set_camera_model(dvm_tracker* t, const dvm_camera_model* model) {
  if (!t) return DVM_ERR_INVALID;
  if (model && !dvm_cam::model_ok(model->model, model->p)) { set_error("dvm_tracker_set_camera_model: unknown model or zero focal length"); return DVM_ERR_INVALID; }
  dvm_camera_model M{};            // NULL and model 0: the default (the structs' cam fields; p is not kept)
  if (model && model->model == dvm_cam::kKannalaBrandt8) M = *model;
  t->model = M; t->clear_next();   // (a finish records the model it ran on: nothing prepared under the old one runs on the new)
  return DVM_OK;
}

namespace {
// dvm_track_begin_batch (the caller's frames) and dvm_track_begin_staged (the frames lie in the extractor's input buffer)
int begin_run(const char* fn, bool staged, dvm_tracker* t, dvm_orb* h, const uint8_t* imgs, int count, int rows, int cols, int stride, int64_t frame_stride, int lap0, int lap1) {
  if (!t || !h || count < 1) return DVM_ERR_INVALID;
  if (count > t->max_frames) { set_error(std::string(fn) + ": more frames than the tracker was created for"); return DVM_ERR_CAPACITY; }
  t->begun = 0; t->clear_next(); t->lf.kf_ready = 0;
  const int rc = staged ? dvm_orb_extract_staged(h, count, rows, cols, lap0, lap1) : dvm_orb_extract_batch_host(h, imgs, count, rows, cols, stride, frame_stride, lap0, lap1);
  if (rc != DVM_OK) return rc;
  t->begun = count; t->rows = rows; t->cols = cols;
  if (count == 1 && t->max_frames == 1) { t->rk_state = 1; t->rk_h = h; t->rk_serial = orb_result_serial(h); }
  return DVM_OK;
}
}  // namespace
int dvm_track_begin_batch(dvm_tracker* t, dvm_orb* h, const uint8_t* imgs, int count, int rows, int cols, int stride, int64_t frame_stride, int lap0, int lap1) {
  return begin_run("dvm_track_begin_batch", false, t, h, imgs, count, rows, cols, stride, frame_stride, lap0, lap1);
}
int dvm_track_begin_staged(dvm_tracker* t, dvm_orb* h, int count, int rows, int cols, int lap0, int lap1) {
  return begin_run("dvm_track_begin_staged", true, t, h, nullptr, count, rows, cols, 0, 0, lap0, lap1);
}
int dvm_track_begin(dvm_tracker* t, dvm_orb* h, const uint8_t* img, int rows, int cols, int stride, int lap0, int lap1) {
  return dvm_track_begin_batch(t, h, img, 1, rows, cols, stride, (int64_t)rows * stride, lap0, lap1);
}

namespace {
// what the frames of a finish share: the fields of dvm_track_queries that are not per query (qs[0]'s), or dvm_track_shared -- the two
// structs name them alike
struct FinishShared {
  float bounds[4]; const dvm_distortion* dist; const float* inv_level_sigma2; int nlevels; dvm_ba_camera cam; int th_high, check_ori, min_matches;
};
extern "C++" template <class P> FinishShared finish_shared(const P& p) {
  FinishShared S{};
  std::memcpy(S.bounds, p.bounds, 16); S.dist = p.dist; S.inv_level_sigma2 = p.inv_level_sigma2; S.nlevels = p.nlevels; S.cam = p.cam;
  S.th_high = p.th_high; S.check_ori = p.check_ori; S.min_matches = p.min_matches;
  return S;
}
// the checks of a resident call on its entry lists and shared parameters, before anything is queued; *n_max: the largest entry count
int resident_check(const char* fn, const dvm_tracker* t, int count, const dvm_track_last* last, const dvm_track_shared* p, int* n_max) {
  const std::string who(fn);
  if (p->nlevels < 1 || p->nlevels > 64 || !p->inv_level_sigma2 || !p->scale_factors) { set_error(who + ": bad shared parameters"); return DVM_ERR_INVALID; }
  *n_max = 0;
  for (int b = 0; b < count; b++) {
    const dvm_track_last& L = last[b];
    if (L.n < 0 || (L.n && (!L.store || !L.slot || !L.octave || !L.angle))) return DVM_ERR_INVALID;
    if (L.n > t->q_cap) { set_error(who + ": more LastFrame entries than the tracker's max_queries"); return DVM_ERR_CAPACITY; }
    if (!L.n) continue;
    if (store_device(L.store) != t->device) { set_error(who + ": the store lives on another device"); return DVM_ERR_INVALID; }
    if (!store_slots_ok(L.store, L.slot, L.n)) { set_error(who + ": a slot outside its store or never written"); return DVM_ERR_INVALID; }
    for (int i = 0; i < L.n; i++)
      if ((int)L.octave[i] >= p->nlevels) { set_error(who + ": an octave outside the level tables"); return DVM_ERR_INVALID; }
    *n_max = std::max(*n_max, L.n);
  }
  return DVM_OK;
}
// the entry lists packed, copied up and k_track_queries queued on stream qs (the tracker's side stream: beside the extraction); the query
// block of the call must be carved (t->qb).  *d_inv_sigma2: mvInvLevelSigma2 on the device; *bytes: what was copied up
int resident_queue(dvm_tracker* t, hipStream_t qs, int count, const dvm_track_last* last, const dvm_track_shared* p, int Qs, const float** d_inv_sigma2,
                   size_t* bytes) {
  std::vector<int32_t> eoff((size_t)count);
  size_t E = 0;
  for (int b = 0; b < count; b++) { eoff[b] = (int32_t)E; E += ((size_t)last[b].n + 63) & ~(size_t)63; }
  const ResidentUpload up = carve_resident_upload(t->rw.hm, count, E);
  if (up.bytes > t->rw.up_bytes) { set_error("dvm_track_finish_batch_resident: the entry lists exceed what the tracker was created for"); return DVM_ERR_CAPACITY; }
  for (int k = 0; k < 64; k++) { up.scale[k] = k < p->nlevels ? p->scale_factors[k] : 1.0f; up.inv_sigma2[k] = k < p->nlevels ? p->inv_level_sigma2[k] : 0.0f; }
  HostPool::get().run((size_t)count, count >= 4 ? 8 : 1, [&](size_t b) {
    const dvm_track_last& L = last[b];
    ResidentFrame& fr = up.fr[b];
    fr.store = L.n ? store_records(L.store) : nullptr; fr.n = L.n; fr.th = L.th; fr.off = eoff[b];
    std::memcpy(fr.q, L.Tcw_pred.q, 16); std::memcpy(fr.t, L.Tcw_pred.t, 12);
    const size_t o = (size_t)eoff[b], n = (size_t)L.n;
    if (n) { std::memcpy(up.slot + o, L.slot, n * 4); std::memcpy(up.angle + o, L.angle, n * 4); std::memcpy(up.octave + o, L.octave, n); }
  });
  DVM_HIP(hipMemcpyAsync(t->rw.d, t->rw.hm, up.bytes, hipMemcpyHostToDevice, qs));
  const ResidentUpload dup = carve_resident_upload(t->rw.d, count, E);
  for (int b = 0; b < count; b++)
    if (last[b].n) { const int rc = store_read_begin(last[b].store, qs); if (rc != DVM_OK) return rc; }
  const dvm_camera_model& M = t->model;
  TrackQueryArgs A{};
  A.fx = (float)p->cam.fx; A.fy = (float)p->cam.fy; A.cx = (float)p->cam.cx; A.cy = (float)p->cam.cy;
  A.min_x = p->bounds[0]; A.max_x = p->bounds[1]; A.min_y = p->bounds[2]; A.max_y = p->bounds[3];
  std::memcpy(A.kb8, M.p, sizeof(A.kb8));
  const QueryBlock& qb = t->qb;
  const TrackQueryOut O{t->qdev(qb.qdesc), t->qdev(qb.qx), t->qdev(qb.qy), t->qdev(qb.qr), t->qdev(qb.qmin), t->qdev(qb.qmax), t->qdev(qb.q_claims),
                        t->qdev(qb.q_angle), t->qdev(qb.q_pos), t->qdev(qb.pose_in), t->qdev(qb.nq_arr), t->rw.dev(t->rm.entry), t->rw.dev(t->rm.nq)};
  launch_track_queries(qs, M.model, dup.fr, dup.slot, dup.octave, dup.angle, dup.scale, A, count, Qs, O);
  { const int rc = hip_check(hipGetLastError(), "k_track_queries"); if (rc != DVM_OK) return rc; }
  for (int b = 0; b < count; b++)
    if (last[b].n) { const int rc = store_read_end(last[b].store, qs); if (rc != DVM_OK) return rc; }
  *d_inv_sigma2 = dup.inv_sigma2; *bytes = up.bytes;
  return DVM_OK;
}

// dvm_track_finish_batch (qs: the caller's queries, copied up) and dvm_track_finish_batch_resident (last / p: the queries built on the
// device from the frames' entry lists and stores); one of qs and last is NULL.  Behind the query block the two are one chain.
int finish_run(dvm_tracker* t, dvm_orb* h, int count, const dvm_track_queries* qs, const dvm_track_last* last, const dvm_track_shared* p,
               const dvm_track_frame_out* outs, dvm_track_result* res) {
  t->clear_next();
  if (t->begun != count) { set_error("dvm_track_finish: no matching dvm_track_begin on this tracker"); return DVM_ERR_STATE; }
  const dvm_camera_model M = t->model;
  const bool kb8 = M.model == dvm_cam::kKannalaBrandt8;    // (the cam fields of the queries are then not read)
  const FinishShared S = qs ? finish_shared(qs[0]) : finish_shared(*p);
  int nq_max = 0;
  for (int b = 0; b < count; b++) {
    const dvm_track_frame_out& o = outs[b];
    if (!o.kps || !o.desc || !o.assign || !o.outlier) return DVM_ERR_INVALID;
    if (!qs) continue;
    const dvm_track_queries& q0 = qs[0];
    const dvm_track_queries& q = qs[b];
    if (q.nq < 0 || q.nq > t->q_cap || q.nlevels < 1 || q.nlevels > 64 || !q.inv_level_sigma2) { set_error("dvm_track_finish: bad query set"); return DVM_ERR_INVALID; }
    if (q.nq && (!q.qdesc || !q.qx || !q.qy || !q.qr || !q.qmin || !q.qmax || !q.q_claims || !q.q_angle || !q.q_pos)) return DVM_ERR_INVALID;
    if (kb8_with_distortion(M, q.dist)) {
      set_error("dvm_track_finish: distortion coefficients under a KannalaBrandt8 camera model (such a frame has mvKeysUn = mvKeys, mDistCoef zero)");
      return DVM_ERR_INVALID;
    }
    if (b && (std::memcmp(q.bounds, q0.bounds, 16) != 0 || (!kb8 && std::memcmp(&q.cam, &q0.cam, sizeof(q.cam)) != 0) || q.th_high != q0.th_high || q.check_ori != q0.check_ori ||
              q.min_matches != q0.min_matches || q.nlevels != q0.nlevels || std::memcmp(q.inv_level_sigma2, q0.inv_level_sigma2, (size_t)q.nlevels * 4) != 0)) {
      set_error("dvm_track_finish_batch: the frames of a batch share camera, bounds, level table and matcher thresholds");
      return DVM_ERR_INVALID;
    }
    if (count > 1 && q.dist && q.dist->k1 != 0.0f) { set_error("dvm_track_finish_batch: distorted keypoints take the single-frame call"); return DVM_ERR_INVALID; }
    nq_max = std::max(nq_max, q.nq);
  }
  if (!qs) {
    const int rc = resident_check("dvm_track_finish_batch_resident", t, count, last, p, &nq_max);
    if (rc != DVM_OK) return rc;
    if (kb8_with_distortion(M, S.dist)) {
      set_error("dvm_track_finish_batch_resident: distortion coefficients under a KannalaBrandt8 camera model (such a frame has mvKeysUn = mvKeys, mDistCoef zero)");
      return DVM_ERR_INVALID;
    }
    if (count > 1 && S.dist && S.dist->k1 != 0.0f) { set_error("dvm_track_finish_batch_resident: distorted keypoints take the single-frame call"); return DVM_ERR_INVALID; }
  }
  for (int b = 0; b < count; b++) std::memset(&res[b], 0, sizeof(res[b]));
  DVM_HIP(hipSetDevice(t->device));
  hipStream_t s = (hipStream_t)dvm_orb_stream(h);
  const dvm_keypoint* d_kps = nullptr; const uint8_t* d_desc = nullptr; const int32_t* d_n = nullptr; int ocap = 0;
  int rc = dvm_orb_result_device(h, 0, &d_kps, &d_desc, &d_n, &ocap);
  if (rc != DVM_OK) return rc;
  if (ocap > t->kp_cap) { set_error("dvm_track_finish: the extractor's keypoint capacity exceeds the tracker's"); return DVM_ERR_CAPACITY; }
  int64_t kps_stride = ocap, desc_stride = (int64_t)ocap * 32;
  if (count > 1) {     // the batch layout dvm_orb_result_device exposes: frame i at a constant stride
    const dvm_keypoint* k1 = nullptr; const uint8_t* d1 = nullptr; const int32_t* n1 = nullptr; int c1 = 0;
    if ((rc = dvm_orb_result_device(h, 1, &k1, &d1, &n1, &c1)) != DVM_OK) return rc;
    kps_stride = k1 - d_kps; desc_stride = d1 - d_desc;
    if (n1 != d_n + 1) { set_error("dvm_track_finish_batch: unexpected result layout"); return DVM_ERR_STATE; }
  }
  const int Qs = (std::max(nq_max, 1) + 63) & ~63;      // the per-query arrays' stride for this call
  const TrackerResults& m = t->m;
  // the query block of THIS call, packed: one copy (~75 KB per frame of 1 000 queries)
  // (the block's end and the ranked lists' inside what create sized: refused before anything is written)
  const QueryBlock qb = carve_query_block(t->ws.hm, (size_t)count, (size_t)Qs);
  const size_t q_used = qb.bytes;
  if (q_used > t->q_bytes || (size_t)count * Qs > (size_t)t->max_frames * t->q_rcap) {
    set_error("dvm_track_finish: the query block exceeds what the tracker was created for");
    return DVM_ERR_CAPACITY;
  }
  t->qb = qb;
  const float* d_inv_sigma2 = t->qdev(qb.inv_sigma2);
  if (qs) {
    HostPool::get().run((size_t)count, count >= 4 ? 8 : 1, [&](size_t b) {       // (a batch's query blocks: 2.4 MB for 32 frames)
      const dvm_track_queries& q = qs[b];
      const size_t o = b * Qs, nq = (size_t)q.nq;
      std::memcpy(qb.qdesc + o * 32, q.qdesc, nq * 32); std::memcpy(qb.qx + o, q.qx, nq * 4); std::memcpy(qb.qy + o, q.qy, nq * 4);
      std::memcpy(qb.qr + o, q.qr, nq * 4); std::memcpy(qb.qmin + o, q.qmin, nq * 4); std::memcpy(qb.qmax + o, q.qmax, nq * 4);
      std::memcpy(qb.q_claims + o, q.q_claims, nq); std::memcpy(qb.q_angle + o, q.q_angle, nq * 4); std::memcpy(qb.q_pos + o * 3, q.q_pos, nq * 12);
      std::memcpy(qb.pose_in + 7 * b, q.pose_in, 56);
      qb.nq_arr[b] = q.nq;
    });
    std::memcpy(qb.inv_sigma2, S.inv_level_sigma2, (size_t)S.nlevels * 4);
    DVM_HIP(hipMemcpyAsync(t->dv.q, t->ws.hm, q_used, hipMemcpyHostToDevice, t->cstream));   // beside the extraction, not behind it
    t->up_first = (int64_t)q_used;
  } else {
    // the entry lists (9 B per entry) in place of the queries: k_track_queries writes the block on the device, beside the extraction
    size_t bytes = 0;
    if ((rc = resident_queue(t, t->cstream, count, last, p, Qs, &d_inv_sigma2, &bytes)) != DVM_OK) return rc;
    t->up_first = (int64_t)bytes;
  }
  DVM_HIP(hipEventRecord(t->cev, t->cstream));
  DVM_HIP(hipStreamWaitEvent(s, t->cev, 0));
  // mvKeysUn: the extractor's keypoints themselves without distortion (Frame.cc:791-797), else undistorted on the device (:799-818)
  const bool undist = count == 1 && S.dist && S.dist->k1 != 0.0f;
  const dvm_keypoint* d_un = d_kps;
  if (undist) {
    rc = dvm_undistort_keypoints(S.dist, d_kps, reinterpret_cast<dvm_keypoint*>(t->dv.kps_un), ocap, 1, s);
    if (rc != DVM_OK) return rc;
    d_un = reinterpret_cast<const dvm_keypoint*>(t->dv.kps_un);
    if (outs[0].kps_un) DVM_HIP(hipMemcpyAsync(m.kps_un, t->dv.kps_un, (size_t)ocap * sizeof(dvm_keypoint_pod), hipMemcpyDeviceToHost, s));
  }
  rc = dvm_frame_build_batch(t->grid, 0, count, d_un, kps_stride, d_desc, desc_stride, d_n, S.bounds[0], S.bounds[1], S.bounds[2], S.bounds[3], s);
  if (rc != DVM_OK) return rc;
  const FrameView FV = frame_view_of(t->grid);    // (bounds of the build above)
  launch_match_window_ranked_batch(s, FV, 0, count, nullptr, nullptr, 0, t->qdev(qb.qdesc), t->qdev(qb.qx), t->qdev(qb.qy), t->qdev(qb.qr), t->qdev(qb.qmin),
                                   t->qdev(qb.qmax), t->qdev(qb.nq_arr), Qs, t->dv.ranked);
  TrackBatch TB{count, Qs, kps_stride, t->qdev(qb.nq_arr)};
  TrackRequery rq{};
  rq.F = FV;
  { static const bool no_rq = std::getenv("DVM_TRACK_NO_REQUERY") != nullptr; if (no_rq) rq.F.skp = nullptr; }   /* timing experiment only */
  rq.qdesc = t->qdev(qb.qdesc); rq.qx = t->qdev(qb.qx); rq.qy = t->qdev(qb.qy); rq.qr = t->qdev(qb.qr); rq.qmin = t->qdev(qb.qmin); rq.qmax = t->qdev(qb.qmax);
  launch_track_claims(s, t->dv.ranked, t->qdev(qb.q_claims), t->qdev(qb.q_angle), 0, rq, reinterpret_cast<const dvm_keypoint_pod*>(d_un), d_n, ocap, S.th_high,
                      S.check_ori, t->dv.assign, t->dv.res, t->ws.dev(m.assign), t->ws.dev(m.res), TB);
  launch_track_gather(s, t->dv.assign, reinterpret_cast<const dvm_keypoint_pod*>(d_un), d_n, ocap, t->qdev(qb.q_pos), d_inv_sigma2, S.nlevels, t->dv.Xw,
                      t->dv.obs, t->dv.info, t->dv.edge_kp, t->dv.nedges, t->dv.res, S.min_matches, t->ws.dev(m.nedges), TB);
  launch_pose_optimize(s, M, S.cam, t->qdev(qb.pose_in), t->dv.Xw, t->dv.obs, t->dv.info, t->dv.nedges, ocap, count, t->ws.dev(m.pose_out), t->dv.edge_out,
                       t->ws.dev(m.n_inl), t->dv.chi);
  launch_track_finish(s, t->dv.assign, d_n, ocap, t->dv.edge_kp, t->dv.nedges, t->dv.edge_out, t->qdev(qb.q_claims), t->ws.dev(m.outlier), t->ws.dev(m.fin), t->dv.res, TB);
  // (what the host wants back is written to mapped memory by the kernels themselves: no copy command behind the chain)
  rc = hip_check(hipGetLastError(), "tracking chain launch");
  if (rc != DVM_OK) return rc;
  {   // the extraction's results of all frames: one synchronisation (the whole chain is through), block copies
    std::vector<dvm_keypoint*> kp(count); std::vector<uint8_t*> dp(count); std::vector<int> caps(count), ns(count), monos(count);
    for (int b = 0; b < count; b++) { kp[b] = outs[b].kps; dp[b] = outs[b].desc; caps[b] = outs[b].cap; }
    rc = dvm_orb_download_batch(h, count, kp.data(), dp.data(), caps.data(), ns.data(), monos.data());
    if (rc != DVM_OK) return rc;
    for (int b = 0; b < count; b++) { res[b].n = ns[b]; res[b].mono_index = monos[b]; }
  }
  static const bool debug = std::getenv("DVM_TRACK_DEBUG") != nullptr;       // per-frame counters on stderr
  for (int b = 0; b < count; b++) {
    const int nq_b = qs ? qs[b].nq : t->rm.nq[b];
    const int min_matches = qs ? qs[b].min_matches : S.min_matches;
    const dvm_track_frame_out& o = outs[b];
    dvm_track_result& r = res[b];
    const int n = r.n;
    if (o.kps_un) std::memcpy(o.kps_un, undist ? reinterpret_cast<const dvm_keypoint*>(m.kps_un) : o.kps, (size_t)n * sizeof(dvm_keypoint));
    const size_t ko = (size_t)b * ocap;
    std::memcpy(o.assign, m.assign + ko, (size_t)n * 4);
    if (!qs) {     // the chain's query numbers as entry numbers of last[b] (k_track_queries kept q_entry beside each query)
      const int32_t* qe = t->rm.entry + (size_t)b * Qs;
      for (int j = 0; j < n; j++) if (o.assign[j] >= 0) o.assign[j] = qe[o.assign[j]];
    }
    const int32_t* rs = m.res + 8 * b;
    r.nmatches = rs[0];
    r.nmatches_before_rotation = rs[2];
    r.n_requeried = rs[3];
    if (debug) std::fprintf(stderr, "track: frame %d nq %d rounds %d requeried %d\n", b, nq_b, rs[4], rs[3]);
    if (rs[1]) {                        // a query ran out of ranked candidates and could not be searched again on the device (DVM_TRACK_NO_REQUERY)
      r.status = DVM_TRACK_REPLAY_ON_HOST;
      if (o.ranked && nq_b) DVM_HIP(hipMemcpy(o.ranked, t->dv.ranked + (size_t)b * Qs * 4, (size_t)nq_b * 16, hipMemcpyDeviceToHost));
      std::memset(o.outlier, 0, (size_t)n);
      continue;
    }
    if (r.nmatches < min_matches) { r.status = DVM_TRACK_FEW_MATCHES; std::memset(o.outlier, 0, (size_t)n); continue; }
    r.status = DVM_TRACK_COMPLETE;
    std::memcpy(o.outlier, m.outlier + ko, (size_t)n);
    r.n_edges = m.nedges[b]; r.n_inliers = m.n_inl[b]; r.nmatches_map = m.fin[4 * b]; r.nmatches_after = m.fin[4 * b + 1];
    std::memcpy(r.pose, m.pose_out + 7 * (size_t)b, 56);
  }
  {     // what the second half runs on: the frames' grids (slots 0..count-1) and mvKeysUn
    LocalFrame& f = t->lf;
    f.ready = count == 1 && res[0].status == DVM_TRACK_COMPLETE; f.batch_ready = 1; f.rkb_ready = 1;
    f.h = h; f.serial = orb_result_serial(h); f.ocap = ocap; f.nlevels = S.nlevels;
    f.d_un = reinterpret_cast<const dvm_keypoint_pod*>(d_un); f.d_n = d_n;
    std::memcpy(f.bounds, S.bounds, 16); std::memcpy(f.inv_sigma2, S.inv_level_sigma2, (size_t)S.nlevels * 4); f.cam = S.cam; f.model = M;
    f.count = count; f.kps_stride = kps_stride; f.ns.resize((size_t)count); f.status.resize((size_t)count);
    f.monos.resize((size_t)count); f.poses.assign(m.pose_out, m.pose_out + 7 * (size_t)count);
    for (int b = 0; b < count; b++) { f.ns[b] = res[b].n; f.status[b] = res[b].status; f.monos[b] = res[b].mono_index; }
    f.d_desc = d_desc; f.desc_stride = desc_stride;
    f.kf_ready = 1;
  }
  if (count == 1 && t->max_frames == 1) { t->rk_state = 2; t->rk_h = h; t->rk_serial = orb_result_serial(h); }   // (whatever the status)
  return DVM_OK;
}
}  // namespace

int dvm_track_finish_batch(dvm_tracker* t, dvm_orb* h, int count, const dvm_track_queries* qs, const dvm_track_frame_out* outs, dvm_track_result* res) {
  if (!t || !h || !qs || !outs || !res || count < 1) return DVM_ERR_INVALID;
  return finish_run(t, h, count, qs, nullptr, nullptr, outs, res);
}

int dvm_track_finish_batch_resident(dvm_tracker* t, dvm_orb* h, int count, const dvm_track_last* last, const dvm_track_shared* p,
                                    const dvm_track_frame_out* outs, dvm_track_result* res) {
  if (!t || !h || !last || !p || !outs || !res || count < 1) return DVM_ERR_INVALID;
  return finish_run(t, h, count, nullptr, last, p, outs, res);
}

int dvm_track_debug_build_queries(dvm_tracker* t, int count, const dvm_track_last* last, const dvm_track_shared* p, int32_t* nq, int32_t* q_entry,
                                  float* qx, float* qy, float* qr, int32_t* qmin, int32_t* qmax, uint8_t* q_claims, float* q_angle, float* q_pos,
                                  uint8_t* qdesc, int32_t* stride) {
  if (!t || !last || !p || !nq || !q_entry || !qx || !qy || !qr || !qmin || !qmax || !q_claims || !q_angle || !q_pos || !qdesc || !stride || count < 1)
    return DVM_ERR_INVALID;
  if (count > t->max_frames) { set_error("dvm_track_debug_build_queries: more frames than the tracker was created for"); return DVM_ERR_CAPACITY; }
  int n_max = 0;
  int rc = resident_check("dvm_track_debug_build_queries", t, count, last, p, &n_max);
  if (rc != DVM_OK) return rc;
  DVM_HIP(hipSetDevice(t->device));
  const int Qs = (std::max(n_max, 1) + 63) & ~63;
  const size_t Qn = (size_t)count * Qs;
  const QueryBlock qb = carve_query_block(t->ws.hm, (size_t)count, (size_t)Qs);
  if (qb.bytes > t->q_bytes || Qn > (size_t)t->max_frames * t->q_rcap) {
    set_error("dvm_track_debug_build_queries: the query block exceeds what the tracker was created for");
    return DVM_ERR_CAPACITY;
  }
  t->qb = qb;
  const float* d_inv_sigma2 = nullptr; size_t bytes = 0;
  if ((rc = resident_queue(t, t->cstream, count, last, p, Qs, &d_inv_sigma2, &bytes)) != DVM_OK) return rc;
  DVM_HIP(hipStreamSynchronize(t->cstream));
  DVM_HIP(hipMemcpy(qdesc, t->qdev(qb.qdesc), Qn * 32, hipMemcpyDeviceToHost)); DVM_HIP(hipMemcpy(qx, t->qdev(qb.qx), Qn * 4, hipMemcpyDeviceToHost));
  DVM_HIP(hipMemcpy(qy, t->qdev(qb.qy), Qn * 4, hipMemcpyDeviceToHost)); DVM_HIP(hipMemcpy(qr, t->qdev(qb.qr), Qn * 4, hipMemcpyDeviceToHost));
  DVM_HIP(hipMemcpy(qmin, t->qdev(qb.qmin), Qn * 4, hipMemcpyDeviceToHost)); DVM_HIP(hipMemcpy(qmax, t->qdev(qb.qmax), Qn * 4, hipMemcpyDeviceToHost));
  DVM_HIP(hipMemcpy(q_claims, t->qdev(qb.q_claims), Qn, hipMemcpyDeviceToHost)); DVM_HIP(hipMemcpy(q_angle, t->qdev(qb.q_angle), Qn * 4, hipMemcpyDeviceToHost));
  DVM_HIP(hipMemcpy(q_pos, t->qdev(qb.q_pos), Qn * 12, hipMemcpyDeviceToHost));
  DVM_HIP(hipMemcpy(nq, t->qdev(qb.nq_arr), (size_t)count * 4, hipMemcpyDeviceToHost));
  std::memcpy(q_entry, t->rm.entry, Qn * 4);
  for (int b = 0; b < count; b++)
    if (nq[b] != t->rm.nq[b]) { set_error("dvm_track_debug_build_queries: the device and mapped query counts differ"); return DVM_ERR_STATE; }
  *stride = Qs;
  return DVM_OK;
}

int dvm_tracker_last_upload_bytes(const dvm_tracker* t, int64_t* first_half, int64_t* second_half) {
  if (!t) return DVM_ERR_INVALID;
  if (first_half) *first_half = t->up_first;
  if (second_half) *second_half = t->up_second;
  return DVM_OK;
}

int dvm_track_finish(dvm_tracker* t, dvm_orb* h, const dvm_track_queries* q, dvm_keypoint* kps, uint8_t* desc, int cap, dvm_keypoint* kps_un,
                     int32_t* assign, uint8_t* outlier, uint32_t* ranked, dvm_track_result* res) {
  if (!q || !res) return DVM_ERR_INVALID;
  dvm_track_frame_out o{kps, desc, cap, kps_un, assign, outlier, ranked};
  return dvm_track_finish_batch(t, h, 1, q, &o, res);
}

// ---- the second half: Tracking::TrackLocalMap (src/Tracking.cc:2668-2740) behind the first
int dvm_tracker_reserve_local_map(dvm_tracker* t, int max_points) {
  if (!t || max_points < 1) return DVM_ERR_INVALID;
  // (the prologue is one workgroup per frame: beyond 1 << 20 points per frame it would dominate the chain, so such a table is refused)
  if ((int64_t)max_points > ((int64_t)t->max_frames << 20)) {
    set_error("dvm_tracker_reserve_local_map: more than 1 048 576 local map points per frame"); return DVM_ERR_CAPACITY;
  }
  DVM_HIP(hipSetDevice(t->device));
  t->lm_cap = 0; t->lf.ready = 0; t->lf.batch_ready = 0;
  // P: table entries of one call (a batch: all frames' tables, each rounded up to 64); per keypoint and per frame: max_frames frames
  const size_t P = ((size_t)max_points + 63) & ~(size_t)63, K = (size_t)t->kp_cap, B = (size_t)t->max_frames;
  const size_t up = local_map_upload_capacity(B, P, K);
  if (const char* what = t->lmw.alloc(up + carve_local_map_work(nullptr, B, P, K).bytes, up + carve_local_map_results(nullptr, B, K, P).bytes, up,
                                      /*mapped*/ true, /*zeroed*/ true))
    return reserve_failed("dvm_tracker_reserve_local_map", what);
  t->lm = carve_local_map_results(t->lmw.hm + up, B, K, P);
  t->lm_cap = (int)P;
  return DVM_OK;
}

namespace {
// one frame's local map as the three entry points hand it to local_map_run: the table as records, copied up (dvm_track_local_map[_batch]),
// or as slots of the frame's store, gathered on the device (dvm_track_local_map_batch_resident); the frame's points; SearchByProjection's
// th and far-point filter
struct LocalSource {
  int32_t n; const dvm_local_point* records; const int32_t* slots; const dvm_map_store* store;
  const int32_t* frame_mp; float th; int far_points; float th_far;
};
// TrackLocalMap on the `count` frames of the last finish (t->lf), behind the entry points' state checks: the tables, the frames' points,
// poses and parameters in ONE upload, ONE chain of batched launches, a workgroup (row of workgroups) per frame on grid slots 0..count-1,
// ONE synchronisation.  A frame the first half did not complete is skipped.  resident: every src[b] gives slots and a store, else records
int local_map_run(dvm_tracker* t, dvm_orb* h, int count, bool resident, const LocalSource* src, const dvm_local_map_out* out, dvm_track_local_result* res,
                  int32_t* status) {
  LocalFrame& f = t->lf;
  static const bool timing = std::getenv("DVM_TRACK_BATCH_TIMING") != nullptr;       // host-side phase times on stderr
  using clk = std::chrono::steady_clock;
  const clk::time_point tp0 = clk::now();
  // the frames' table offsets: each frame's span rounded up to 64, back to back; a frame the first half did not complete gets none
  std::vector<int32_t> qoff((size_t)count), nb((size_t)count, 0);
  size_t T = 0, span_max = 64;
  int live = 0;
  for (int b = 0; b < count; b++) {
    qoff[b] = (int32_t)std::min(T, (size_t)INT32_MAX);
    if (f.status[b] != DVM_TRACK_COMPLETE) continue;
    const LocalSource& q = src[b];
    const int N = f.ns[b];
    if (q.n < 0 || (q.n && !(resident ? (const void*)q.slots : (const void*)q.records)) || (N && !q.frame_mp) || !out[b].mp_out || !out[b].outlier) return DVM_ERR_INVALID;
    for (int j = 0; j < N; j++)
      if (q.frame_mp[j] < -1 || q.frame_mp[j] >= q.n) { set_error("dvm_track_local_map_batch: frame_mp names a point outside the table"); return DVM_ERR_INVALID; }
    if (resident && q.n) {     // every slot checked here, on the host: k_store_gather indexes the store with them
      if (!q.store) return DVM_ERR_INVALID;
      if (store_device(q.store) != t->device) { set_error("dvm_track_local_map_batch_resident: the store lives on another device"); return DVM_ERR_INVALID; }
      if (!store_slots_ok(q.store, q.slots, q.n)) {
        set_error("dvm_track_local_map_batch_resident: a slot outside its store or never written"); return DVM_ERR_INVALID;
      }
    }
    const size_t span = ((size_t)q.n + 63) & ~(size_t)63;
    nb[b] = q.n; T += span; span_max = std::max(span_max, span); live++;
  }
  if (T > (size_t)t->lm_cap) { set_error("dvm_track_local_map_batch: more local map points than reserved (each frame's rounded up to 64)"); return DVM_ERR_CAPACITY; }
  for (int b = 0; b < count; b++) { std::memset(&res[b], 0, sizeof(res[b])); status[b] = f.status[b]; }
  if (!live) { f.ready = 0; f.batch_ready = 0; f.rkb_ready = 0; return DVM_OK; }
  const int ocap = f.ocap;
  const size_t Tc = std::max(T, (size_t)64);
  // the upload block of this call in the staging buffer (hm) and, at the same offsets, in its device copy (d); copy_bytes: what goes up
  const auto carve_upload = [&](uint8_t* base) {
    if (resident) return carve_local_map_upload_resident(base, (size_t)count, Tc, (size_t)ocap);
    LocalMapUploadResident r{carve_local_map_upload(base, (size_t)count, Tc, (size_t)ocap), nullptr, nullptr, 0};
    r.copy_bytes = r.u.bytes;
    return r;
  };
  const LocalMapUploadResident rup = carve_upload(t->lmw.hm), drup = carve_upload(t->lmw.d);
  const LocalMapUpload &up = rup.u, &dup = drup.u;
  if (up.bytes > t->lmw.up_bytes) { set_error("dvm_track_local_map_batch: the upload block exceeds the reservation"); return DVM_ERR_CAPACITY; }
  DVM_HIP(hipSetDevice(t->device));
  hipStream_t s = (hipStream_t)dvm_orb_stream(h);
  // 1. the tables, the frames' points, poses and parameters packed into the mapped staging block by the pool threads: ONE copy
  std::vector<float> scale(256, 1.0f);
  int rc = dvm_orb_tables(h, scale.data(), nullptr, nullptr, nullptr, nullptr);
  if (rc != DVM_OK) return rc;
  std::memcpy(up.scale, scale.data(), 64 * 4);
  std::memcpy(up.inv_sigma2, f.inv_sigma2, 64 * 4);
  HostPool::get().run((size_t)count, count >= 4 ? 8 : 1, [&](size_t b) {       // (32 tables of 3 000 points: 7 MB)
    const bool go = f.status[b] == DVM_TRACK_COMPLETE;
    const LocalSource& q = src[b];
    int32_t* fm = up.frame_mp + b * (size_t)ocap;
    std::memcpy(up.pose + 7 * b, f.poses.data() + 7 * b, 56);    // the finish's pose, or the reference-keyframe chain's
    up.fa[b] = go ? LocalFrameArgs{nb[b], q.far_points ? 1 : 0, q.th, q.th_far} : LocalFrameArgs{0, 0, 1.0f, 0.0f};
    up.qoff[b] = qoff[b]; up.skip_on[b] = 1;
    if (resident) rup.stores[b] = go && nb[b] ? store_records(q.store) : nullptr;
    if (go) {
      if (nb[b] && !resident) std::memcpy(up.pts + qoff[b], q.records, (size_t)nb[b] * sizeof(LocalPointPod));
      if (nb[b] && resident) std::memcpy(rup.slots + qoff[b], q.slots, (size_t)nb[b] * 4);
      if (f.ns[b]) std::memcpy(fm, q.frame_mp, (size_t)f.ns[b] * 4);
    } else {
      for (int j = 0; j < ocap; j++) fm[j] = -1;        // a skipped frame holds nothing and searches nothing
    }
  });
  DVM_HIP(hipMemcpyAsync(t->lmw.d, t->lmw.hm, rup.copy_bytes, hipMemcpyHostToDevice, s));
  t->up_second = (int64_t)rup.copy_bytes;
  const clk::time_point tp1 = clk::now();
  if (resident) {     // the device tables from the stores, behind their last updates
    for (int b = 0; b < count; b++)
      if (f.status[b] == DVM_TRACK_COMPLETE && nb[b]) { rc = store_read_begin(src[b].store, s); if (rc != DVM_OK) return rc; }
    launch_store_gather(s, StoreGather{drup.stores, dup.fa, dup.qoff, drup.slots}, dup.pts, count, (int)span_max);
    for (int b = 0; b < count; b++)
      if (f.status[b] == DVM_TRACK_COMPLETE && nb[b]) { rc = store_read_end(src[b].store, s); if (rc != DVM_OK) return rc; }
  }
  // 2. device arrays of this call: per entry at the frames' offsets, per keypoint at b * ocap
  const LocalMapWork W = carve_local_map_work(t->lmw.d + t->lmw.up_bytes, (size_t)count, Tc, (size_t)ocap);
  const LocalQueries& LQ = W.LQ;
  uint32_t* const d_ranked = W.ranked;
  int32_t* const d_lres = W.lres;
  LocalMapArgs A;
  A.fx = (float)f.cam.fx; A.fy = (float)f.cam.fy; A.cx = (float)f.cam.cx; A.cy = (float)f.cam.cy;
  A.min_x = f.bounds[0]; A.max_x = f.bounds[1]; A.min_y = f.bounds[2]; A.max_y = f.bounds[3];
  A.log_scale_factor = f.nlevels > 1 ? (float)std::log((double)scale[1]) : 0.0f;     // Frame::mfLogScaleFactor = log(mfScaleFactor)
  A.n_levels = f.nlevels; A.per_frame = dup.fa;
  std::memcpy(A.kb8, f.model.p, sizeof(A.kb8));
  const TrackBatch TB{count, (int)span_max, f.kps_stride, LQ.nq, dup.qoff};
  auto& r = t->lm;
  // 3. SearchLocalPoints up to the queries
  bool want_tp = false;
  for (int b = 0; b < count; b++) want_tp = want_tp || (f.status[b] == DVM_TRACK_COMPLETE && out[b].track_pts);
  launch_track_local_prologue(s, f.model.model, dup.pts, dup.frame_mp, dup.pose, dup.scale, f.d_n, ocap, A, LQ, want_tp ? t->lmw.dev(r.tp) : nullptr, t->lmw.dev(r.res),
                              TB);
  // 4. the ranked window search on the frames' grids (built by the finish), the keypoints with observed points skipped
  const FrameView FV = frame_view_of(t->grid);
  launch_match_window_ranked_batch(s, FV, 0, count, LQ.skip, dup.skip_on, ocap, LQ.qdesc, LQ.qx, LQ.qy, LQ.qr, LQ.qmin, LQ.qmax, LQ.nq,
                                   (int)span_max, d_ranked, dup.qoff);
  // 5. SearchByProjection(F, points)'s claim replay: mvpMapPoints after the search (device copy for the gather, mapped copy for the host)
  TrackRequery rq{};
  rq.F = FV;
  rq.qdesc = LQ.qdesc; rq.qx = LQ.qx; rq.qy = LQ.qy; rq.qr = LQ.qr; rq.qmin = LQ.qmin; rq.qmax = LQ.qmax;
  launch_track_claims_local(s, d_ranked, LQ, rq, f.d_un, f.d_n, ocap, 100 /* TH_HIGH */, 0.8f, t->dv.assign, d_lres, t->lmw.dev(r.mp),
                            t->lmw.dev(r.res) + 8 * count, TB);
  // 6. PoseOptimization's edges in keypoint order (positions from the table; no min_matches gate: below 3 edges the pose stays), the pose
  //    seeded from the first half's float pose, the outlier flags and mnMatchesInliers
  const TrackBatch TE{count, 0, f.kps_stride, nullptr, dup.qoff};
  launch_track_gather(s, t->dv.assign, f.d_un, f.d_n, ocap, LQ.pos, dup.inv_sigma2, f.nlevels, t->dv.Xw, t->dv.obs, t->dv.info, t->dv.edge_kp,
                      t->dv.nedges, d_lres, 0, t->lmw.dev(r.nedges), TE);
  launch_pose_optimize(s, f.model, f.cam, LQ.pose_in, t->dv.Xw, t->dv.obs, t->dv.info, t->dv.nedges, ocap, count, t->lmw.dev(r.pose), t->dv.edge_out,
                       t->lmw.dev(r.n_inl), t->dv.chi);
  launch_track_finish(s, t->dv.assign, f.d_n, ocap, t->dv.edge_kp, t->dv.nedges, t->dv.edge_out, LQ.claims, t->lmw.dev(r.outlier), t->lmw.dev(r.fin),
                      d_lres, TE);
  t->clear_next();   // once per finish
  rc = hip_check(hipGetLastError(), "local map chain launch");
  if (rc != DVM_OK) return rc;
  // 7. ONE synchronisation, then every completed frame's outputs copied out of mapped memory by the pool threads
  DVM_HIP(hipStreamSynchronize(s));
  const clk::time_point tp2 = clk::now();
  HostPool::get().run((size_t)count, count >= 4 ? 8 : 1, [&](size_t b) {
    if (f.status[b] != DVM_TRACK_COMPLETE) return;
    const int N = f.ns[b], n = nb[b];
    const size_t ko = b * (size_t)ocap;
    const dvm_local_map_out& o = out[b];
    if (N) { std::memcpy(o.mp_out, r.mp + ko, (size_t)N * 4); std::memcpy(o.outlier, r.outlier + ko, (size_t)N); }
    if (o.track_pts && n) std::memcpy(o.track_pts, r.tp + qoff[b], (size_t)n * sizeof(dvm_track_point));
    dvm_track_local_result& q = res[b];
    const int32_t* pr = r.res + 8 * b;
    const int32_t* cr = r.res + 8 * ((size_t)count + b);
    q.n_to_match = pr[0]; q.n_cleared_bad = pr[1]; q.nmatches = cr[0]; q.n_requeried = cr[3];
    q.n_edges = r.nedges[b]; q.n_inliers = r.n_inl[b]; q.matches_inliers = r.fin[4 * b];
    std::memcpy(q.pose, r.pose + 7 * b, 56);
    // Sophus::SE3f(SE3quat_recov.rotation().cast<float>(), SE3quat_recov.translation().cast<float>()) (Optimizer.cc:1023-1025)
    for (int k = 0; k < 3; k++) q.Tcw.t[k] = (float)q.pose[k];
    for (int k = 0; k < 4; k++) q.Tcw.q[k] = (float)q.pose[3 + k];
  });
  if (timing) {
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    std::fprintf(stderr, "track local map batch of %d (%zu entries): pack + enqueue %.3f  wait %.3f  results out %.3f ms\n", count, T, ms(tp0, tp1),
                 ms(tp1, tp2), ms(tp2, clk::now()));
  }
  return DVM_OK;
}
}  // namespace

// the state check the three entry points share: right after `after` on this tracker and extractor (count 0: the single call, on one
// frame that completed), with the working set reserved
static int local_map_state(const char* fn, const char* after, const dvm_tracker* t, const dvm_orb* h, int count) {
  const LocalFrame& f = t->lf;
  if (!(count ? f.batch_ready && f.count == count : f.ready) || f.h != h || orb_result_serial(h) != f.serial) {
    set_error(std::string(fn) + ": not right after a " + after + " (same tracker and extractor)");
    return DVM_ERR_STATE;
  }
  if (!t->lmw.d) { set_error(std::string(fn) + ": no dvm_tracker_reserve_local_map on this tracker"); return DVM_ERR_STATE; }
  return DVM_OK;
}

int dvm_track_local_map(dvm_tracker* t, dvm_orb* h, const dvm_local_point* pts, int n, const int32_t* frame_mp, float th, int far_points,
                        float th_far, int32_t* mp_out, uint8_t* outlier, dvm_track_point* track_pts, dvm_track_local_result* res) {
  if (!t || !h || !mp_out || !outlier || !res || n < 0 || (n && !pts)) return DVM_ERR_INVALID;
  const int rc = local_map_state("dvm_track_local_map", "dvm_track_finish of one frame that returned DVM_TRACK_COMPLETE", t, h, 0);
  if (rc != DVM_OK) return rc;
  if (n > t->lm_cap) { set_error("dvm_track_local_map: more local map points than reserved"); return DVM_ERR_CAPACITY; }
  const int N = t->lf.ns[0];
  if (N && !frame_mp) return DVM_ERR_INVALID;
  for (int j = 0; j < N; j++)
    if (frame_mp[j] < -1 || frame_mp[j] >= n) { set_error("dvm_track_local_map: frame_mp names a point outside the table"); return DVM_ERR_INVALID; }
  // the batch of one frame (ready: its first-half status is DVM_TRACK_COMPLETE)
  const LocalSource src{n, pts, nullptr, nullptr, frame_mp, th, far_points, th_far};
  const dvm_local_map_out out{mp_out, outlier, track_pts};
  int32_t status = 0;
  return local_map_run(t, h, 1, false, &src, &out, res, &status);
}

int dvm_track_local_map_batch(dvm_tracker* t, dvm_orb* h, int count, const dvm_local_map_in* in, const dvm_local_map_out* out,
                              dvm_track_local_result* res, int32_t* status) {
  if (!t || !h || !in || !out || !res || !status || count < 1) return DVM_ERR_INVALID;
  const int rc = local_map_state("dvm_track_local_map_batch", "dvm_track_finish[_batch] of `count` frames", t, h, count);
  if (rc != DVM_OK) return rc;
  std::vector<LocalSource> src((size_t)count);
  for (int b = 0; b < count; b++) src[b] = LocalSource{in[b].n, in[b].pts, nullptr, nullptr, in[b].frame_mp, in[b].th, in[b].far_points, in[b].th_far};
  return local_map_run(t, h, count, false, src.data(), out, res, status);
}

int dvm_track_local_map_batch_resident(dvm_tracker* t, dvm_orb* h, int count, const dvm_local_map_in_resident* in, const dvm_local_map_out* out,
                                       dvm_track_local_result* res, int32_t* status) {
  if (!t || !h || !in || !out || !res || !status || count < 1) return DVM_ERR_INVALID;
  const int rc = local_map_state("dvm_track_local_map_batch_resident", "dvm_track_finish[_batch][_resident] of `count` frames", t, h, count);
  if (rc != DVM_OK) return rc;
  std::vector<LocalSource> src((size_t)count);
  for (int b = 0; b < count; b++) src[b] = LocalSource{in[b].n, nullptr, in[b].slots, in[b].store, in[b].frame_mp, in[b].th, in[b].far_points, in[b].th_far};
  return local_map_run(t, h, count, true, src.data(), out, res, status);
}

// ---- the other way into the second half: Tracking::TrackReferenceKeyFrame (src/Tracking.cc:2461-2520) on the frames of a finish, or on
//      the one frame of a single-frame begin / finish
namespace {
// the checks of dvm_track_reference_keyframe on one frame's keyframe, parameters and outputs (form (b)); cap: keypoints per keyframe.
// kf NULL: a resident keyframe (check_refkf_resident; its FeatureVector passed these checks when it was put)
int check_refkf_frame(const char* fn, const dvm_ref_keyframe* kf, const dvm_track_refkf_params* p, const dvm_track_refkf_out* out, int cap) {
  char msg[256];
  if (!out->mp_out || !out->dropped || !out->outlier) return DVM_ERR_INVALID;
  if (p->nlevels < 1 || p->nlevels > 64 || !p->inv_level_sigma2 || p->th_low < 0 || p->th_low > 255 || p->levelsup < 0 || p->min_matches < 0 ||
      !(p->nnratio >= 0.0f)) {
    std::snprintf(msg, sizeof msg, "%s: bad parameters", fn); set_error(msg); return DVM_ERR_INVALID;
  }
  if (!kf) return DVM_OK;
  const int n = kf->n, nf = kf->fv_n;
  if (n < 0 || nf < 0) return DVM_ERR_INVALID;
  if (n > cap || nf > cap) { std::snprintf(msg, sizeof msg, "%s: more keyframe keypoints than reserved", fn); set_error(msg); return DVM_ERR_CAPACITY; }
  if (n && (!kf->kps_un || !kf->desc || !kf->mp || !kf->mp_pos || !kf->mp_nobs)) return DVM_ERR_INVALID;
  if (nf && (!kf->fv_node || !kf->fv_off || !kf->fv_feat)) return DVM_ERR_INVALID;
  const int nfeat = nf ? kf->fv_off[nf] : 0;
  if (nf && kf->fv_off[0] != 0) return DVM_ERR_INVALID;
  for (int a = 0; a < nf; a++) {
    if (kf->fv_off[a + 1] < kf->fv_off[a] || (a && (uint32_t)kf->fv_node[a] <= (uint32_t)kf->fv_node[a - 1])) {
      std::snprintf(msg, sizeof msg, "%s: mFeatVec offsets must not decrease and its nodes must ascend (as unsigned)", fn); set_error(msg);
      return DVM_ERR_INVALID;
    }
  }
  if (nfeat > n) { std::snprintf(msg, sizeof msg, "%s: mFeatVec lists more features than the keyframe has", fn); set_error(msg); return DVM_ERR_INVALID; }
  for (int k = 0; k < nfeat; k++)
    if (kf->fv_feat[k] < 0 || kf->fv_feat[k] >= n) {
      std::snprintf(msg, sizeof msg, "%s: mFeatVec names a keypoint outside the keyframe", fn); set_error(msg); return DVM_ERR_INVALID;
    }
  return DVM_OK;
}

// one frame's keyframe as the entry points hand it to refkf_enqueue: uploaded whole (dvm_track_reference_keyframe[_batch]), or a
// keyframe-store slot plus its map points as map-store slots, packed on the device (dvm_track_reference_keyframe_batch_resident);
// neither: the frame does not run
struct RefKfSource {
  const dvm_ref_keyframe* kf = nullptr;
  const dvm_kf_resident* r = nullptr; KfSlotView v{};
  bool runs() const { return kf || r; }
  int n() const { return kf ? kf->n : v.n; }
  int fv_n() const { return kf ? kf->fv_n : v.fv_n; }
  const int32_t* mp() const { return kf ? kf->mp : r->mp_slot; }   // the caller's ids of the keyframe's points
};
// a resident keyframe's slot and lists, checked on the host: k_refkf_gather indexes the stores with them; fills q.v
int check_refkf_resident(const char* fn, const dvm_tracker* t, const dvm_keyframe_store* kfs, int b, RefKfSource& q, int cap) {
  const dvm_kf_resident& r = *q.r;
  const std::string w = std::string(fn) + ": frame " + std::to_string(b) + " (slot " + std::to_string(r.slot) + ")";
  if (!kfs_slot_view(kfs, r.slot, &q.v)) { set_error(w + ": slot outside the store, never written or removed"); return DVM_ERR_INVALID; }
  if (q.v.n > cap) { set_error(w + ": more keyframe keypoints than reserved"); return DVM_ERR_CAPACITY; }
  if (q.v.n > 0 && !r.mp_slot) { set_error(w + ": missing mp_slot"); return DVM_ERR_INVALID; }
  if (r.points && store_device(r.points) != t->device) { set_error(w + ": its map store lives on another device"); return DVM_ERR_INVALID; }
  const int bad = store_kf_slots_check(r.points, r.mp_slot, q.v.n, nullptr);
  if (bad == 1) { set_error(w + ": an mp_slot below -1, outside its map store or never written"); return DVM_ERR_INVALID; }
  if (bad == 2) { set_error(w + ": an mp_slot names a point and points is NULL"); return DVM_ERR_INVALID; }
  return DVM_OK;
}

// (re)allocates w for keyframes of R entries per call (a multiple of 64) and the tracker's max_frames frames; fn names the caller's errors
int reserve_refkf(dvm_tracker* t, RefKf& w, size_t R, const char* fn) {
  DVM_HIP(hipSetDevice(t->device));
  w.cap = 0;
  const size_t K = (size_t)t->kp_cap, B = (size_t)t->max_frames;
  const size_t up = carve_keyframe_upload_resident(nullptr, B, R).u.bytes;   // (the uploaded form's block and the resident form's lists)
  if (const char* what = w.ws.alloc(up + carve_refkf_work(nullptr, B, K).bytes, up + carve_refkf_results(nullptr, B, K).bytes, up, /*mapped*/ true, /*zeroed*/ true))
    return reserve_failed(fn, what);
  w.r = carve_refkf_results(w.ws.hm + up, B, K);
  w.cap = (int)R;
  return DVM_OK;
}

// dvm_track_reference_keyframe_batch's chain up to its synchronisation, on the frames of the last finish (t->lf) and the working set w.
// Every keyframe is checked as the single call checks it and the shared parameters equal across the frames that run before anything is
// enqueued (a refused call leaves the finish for a corrected one); then the keyframes packed back to back into w's staging block by the pool
// threads, ONE asynchronous copy, and the chain on the extractor's stream.  *nrun_out: the frames that run (none: nothing enqueued),
// *T_out: their keyframe entries.
// src[b]: frame b's keyframe; the resident ones (all or none of a call) are slots of `store`, filled into the block by k_refkf_gather.
int refkf_enqueue(const char* fn, dvm_tracker* t, RefKf& w, dvm_orb* h, const dvm_vocab* voc, int count, RefKfSource* src, const dvm_keyframe_store* store,
                  int kf_cap, const dvm_track_refkf_params* ps, const dvm_track_refkf_out* outs, dvm_track_refkf_result* res, int32_t* status,
                  int* nrun_out, size_t* T_out) {
  LocalFrame& f = t->lf;
  const bool resident = store != nullptr;
  const std::string sfn = fn;
  if (resident && kfs_device(store) != t->device) { set_error(sfn + ": the keyframe store lives on another device"); return DVM_ERR_INVALID; }
  std::vector<int32_t> qoff((size_t)count, 0), run;
  size_t T = 0;
  const dvm_track_refkf_params* p0 = nullptr;
  for (int b = 0; b < count; b++) {
    qoff[b] = (int32_t)std::min(T, (size_t)INT32_MAX);
    RefKfSource& q = src[b];
    if (!q.runs()) continue;
    const dvm_track_refkf_params* p = &ps[b];
    int rc = check_refkf_frame(fn, q.kf, p, &outs[b], kf_cap);
    if (rc == DVM_OK && q.r) rc = check_refkf_resident(fn, t, store, b, q, kf_cap);
    if (rc != DVM_OK) return rc;
    if (!p0) {
      p0 = p;
    } else if (p->nnratio != p0->nnratio || p->check_ori != p0->check_ori || p->th_low != p0->th_low || p->min_matches != p0->min_matches ||
               p->min_map != p0->min_map || p->levelsup != p0->levelsup || p->nlevels != p0->nlevels ||
               std::memcmp(p->inv_level_sigma2, p0->inv_level_sigma2, (size_t)p->nlevels * 4) != 0 ||
               (f.model.model != dvm_cam::kKannalaBrandt8 && std::memcmp(&p->cam, &p0->cam, sizeof(p->cam)) != 0)) {
      set_error(sfn + ": the frames that run share camera, level table and matcher thresholds");
      return DVM_ERR_INVALID;
    }
    T += ((size_t)std::max(q.n(), q.fv_n()) + 63) & ~(size_t)63;
    run.push_back(b);
  }
  if (p0 && vocab_device(voc) != t->device) { set_error(sfn + ": the vocabulary lives on another device"); return DVM_ERR_INVALID; }
  if (T > (size_t)w.cap) {
    set_error(sfn + ": more keyframe keypoints than reserved (each keyframe's rounded up to 64)"); return DVM_ERR_CAPACITY;
  }
  const int ocap = f.ocap;
  // the upload block of this call in the staging buffer (hm) and, at the same offsets, in its device copy (d); copy_bytes: what goes up
  const auto carve_upload = [&](uint8_t* base) {
    if (resident) return carve_keyframe_upload_resident(base, (size_t)count, std::max(T, (size_t)64));
    KeyframeUploadResident r{carve_keyframe_upload(base, (size_t)count, std::max(T, (size_t)64)), nullptr, nullptr, 0};
    r.copy_bytes = r.u.bytes;
    return r;
  };
  const KeyframeUploadResident rup = carve_upload(w.ws.hm), drup = carve_upload(w.ws.d);
  const KeyframeUpload &up = rup.u, &dup = drup.u;
  if (up.bytes > w.ws.up_bytes || ocap > t->kp_cap) {
    set_error(sfn + ": the upload block exceeds the reservation"); return DVM_ERR_CAPACITY;
  }
  // accepted: once per finish, and the single call no longer runs on it
  for (int b = 0; b < count; b++) { std::memset(&res[b], 0, sizeof(res[b])); status[b] = f.status[b]; }
  f.rkb_ready = 0; t->rk_state = 0;
  const int nrun = (int)run.size();
  *nrun_out = nrun; *T_out = T;
  if (!nrun) return DVM_OK;
  const dvm_track_refkf_params& P0 = *p0;
  DVM_HIP(hipSetDevice(t->device));
  hipStream_t s = (hipStream_t)dvm_orb_stream(h);
  // 1. the keyframes packed back to back into the mapped staging block by the pool threads: ONE asynchronous copy
  std::memset(up.inv_sigma2, 0, 64 * 4);
  std::memcpy(up.inv_sigma2, P0.inv_level_sigma2, (size_t)P0.nlevels * 4);
  int nwg = 0;
  for (int r = 0; r < nrun; r++) { up.run[r] = run[r]; up.wg_base[r] = nwg; nwg += (src[run[r]].fv_n() + 3) / 4; }
  up.wg_base[nrun] = nwg;
  HostPool::get().run((size_t)count, count >= 4 ? 8 : 1, [&](size_t b) {
    const RefKfSource& q = src[b];
    const dvm_ref_keyframe* kf = q.kf;
    const size_t o = (size_t)qoff[b];
    up.qoff[b] = qoff[b];
    int32_t* rs = up.res + 8 * b;
    for (int k = 0; k < 8; k++) rs[k] = 0;
    if (resident) std::memset(&rup.items[b], 0, sizeof(RefKfGatherItem));
    if (!q.runs()) {                      // a frame that does not run: no edges (k_track_gather reads res[1] != 0), the pose left alone
      rs[1] = 1; up.kfv_n[b] = 0;
      std::memcpy(up.pose + 7 * b, f.poses.data() + 7 * b, 56);
      return;
    }
    std::memcpy(up.pose + 7 * b, ps[b].pose_in, 56);
    up.kfv_n[b] = q.fv_n();
    if (q.r) {                            // the slot list goes up; k_refkf_gather packs the rest where the loop below packs it
      const KfSlotView& v = q.v;
      rup.items[b] = RefKfGatherItem{q.r->points ? store_records(q.r->points) : nullptr, v.kps, v.desc, v.fv_node, v.fv_off, v.fv_feat, v.n, v.n_feat};
      if (v.n) std::memcpy(rup.mp_slot + o, q.r->mp_slot, (size_t)v.n * 4);
      return;
    }
    const int n = kf->n, nf = kf->fv_n, nfeat = nf ? kf->fv_off[nf] : 0;
    if (n) std::memcpy(up.desc + o * 32, kf->desc, (size_t)n * 32);
    for (int i = 0; i < n; i++) {
      const int id = kf->mp[i];
      const bool use = id >= 0 && !(kf->mp_bad && kf->mp_bad[i]);      // SearchByBoW: no map point or a bad one -> skipped (:247-252)
      up.angle[o + i] = kf->kps_un[i].angle; up.use[o + i] = use ? 1 : 0;
      up.claims[o + i] = id >= 0 && kf->mp_nobs[i] > 0 ? 1 : 0;
      for (int k = 0; k < 3; k++) up.pos[3 * (o + i) + k] = id >= 0 ? kf->mp_pos[3 * i + k] : 0.0f;
    }
    int32_t* fo = up.fv_off + o + b;
    if (nf) {
      std::memcpy(up.fv_node + o, kf->fv_node, (size_t)nf * 4); std::memcpy(fo, kf->fv_off, ((size_t)nf + 1) * 4);
      std::memcpy(up.fv_feat + o, kf->fv_feat, (size_t)nfeat * 4);
    } else {
      fo[0] = 0;
    }
  });
  DVM_HIP(hipMemcpyAsync(w.ws.d, w.ws.hm, rup.copy_bytes, hipMemcpyHostToDevice, s));
  t->up_refkf = (int64_t)rup.copy_bytes;
  if (resident) {     // the packed keyframes from the stores, behind their last puts and updates; nothing after the gather reads a store
    std::vector<const dvm_map_store*> maps;    // the distinct map stores of the frames that run: one wait and one event each
    for (int r = 0; r < nrun; r++) {
      const dvm_map_store* m = src[run[r]].r->points;
      if (m && std::find(maps.begin(), maps.end(), m) == maps.end()) maps.push_back(m);
    }
    int rc = kfs_read_begin(store, s);
    for (size_t k = 0; k < maps.size() && rc == DVM_OK; k++) rc = store_read_begin(maps[k], s);
    if (rc != DVM_OK) return rc;
    launch_refkf_gather(s, drup.items, drup.mp_slot, dup.run, nrun, dup.qoff, dup.kfv_n,
                        RefKfGatherOut{dup.desc, dup.angle, dup.use, dup.claims, dup.pos, dup.fv_node, dup.fv_feat, dup.fv_off});
    rc = kfs_read_end(store, s);
    for (size_t k = 0; k < maps.size() && rc == DVM_OK; k++) rc = store_read_end(maps[k], s);
    if (rc != DVM_OK) return rc;
  }
  // 2. the chain: ComputeBoW (the transform of all frames that run in one launch, then the BowVector / FeatureVector in LDS, a workgroup per
  //    frame) -> SearchByBoW (each frame's keyframe nodes on their own workgroups) -> rotation check -> PoseOptimization's edges in keypoint
  //    order -> k_pose_optimize seeded from pose_in -> outlier flags and nmatchesMap, as the batched first half runs them (a frame that
  //    does not run: an empty workgroup in each)
  const RefKfWork W = carve_refkf_work(w.ws.d + w.ws.up_bytes, (size_t)t->max_frames, (size_t)t->kp_cap);
  const RefKfMapped& r = w.r;
  RefKfArgs A{};
  A.word = W.word; A.node = W.node; A.w = W.w; A.fv_node = W.fv_node; A.fv_feat = W.fv_feat; A.fv_off = W.fv_off; A.cnt = W.cnt;
  A.match = W.match; A.bin = W.bin; A.res = dup.res;
  A.h_bow_ids = w.ws.dev(r.bow_ids); A.h_bow_vals = w.ws.dev(r.bow_vals); A.h_fv_node = w.ws.dev(r.fv_node); A.h_fv_off = w.ws.dev(r.fv_off);
  A.h_fv_feat = w.ws.dev(r.fv_feat); A.h_match = w.ws.dev(r.match); A.h_cnt = w.ws.dev(r.cnt);
  A.kdesc = dup.desc; A.kangle = dup.angle; A.kuse = dup.use; A.kfv_node = dup.fv_node; A.kfv_off = dup.fv_off; A.kfv_feat = dup.fv_feat;
  A.run = dup.run; A.kqoff = dup.qoff; A.kfv_nb = dup.kfv_n; A.wg_base = dup.wg_base; A.nrun = nrun; A.nwg = nwg;
  A.kps_stride = f.kps_stride; A.desc_stride = f.desc_stride;
  vocab_launch_transform(voc, s, f.d_desc, ocap, f.d_n, P0.levelsup, W.word, W.node, W.w, dup.run, nrun, f.desc_stride);
  launch_refkf_bow(s, A, f.d_n, ocap);
  launch_refkf_search(s, A, f.d_un, f.d_desc, f.d_n, ocap, P0.th_low, P0.nnratio);
  launch_refkf_settle(s, A, f.d_n, ocap, P0.check_ori);
  const TrackBatch TE{count, 0, f.kps_stride, nullptr, dup.qoff};
  launch_track_gather(s, W.match, f.d_un, f.d_n, ocap, dup.pos, dup.inv_sigma2, P0.nlevels, t->dv.Xw, t->dv.obs, t->dv.info, t->dv.edge_kp, t->dv.nedges,
                      dup.res, P0.min_matches, w.ws.dev(r.nedges), TE);
  launch_pose_optimize(s, f.model, P0.cam, dup.pose, t->dv.Xw, t->dv.obs, t->dv.info, t->dv.nedges, ocap, count, w.ws.dev(r.pose), t->dv.edge_out,
                       w.ws.dev(r.n_inl), t->dv.chi);
  launch_track_finish(s, W.match, f.d_n, ocap, t->dv.edge_kp, t->dv.nedges, t->dv.edge_out, dup.claims, w.ws.dev(r.outlier), w.ws.dev(r.fin), dup.res, TE);
  return hip_check(hipGetLastError(), "reference keyframe chain launch");
}

// after refkf_enqueue's chain is through: every frame that ran copied out of w's mapped results by the pool threads, and what the second
// half runs on -- such a frame complete or not by this call's status, seeded from its pose
void refkf_copy_out(dvm_tracker* t, const RefKf& w, int count, const RefKfSource* src, const dvm_track_refkf_params* ps,
                    const dvm_track_refkf_out* outs, dvm_track_refkf_result* res, int32_t* status) {
  LocalFrame& f = t->lf;
  const RefKfMapped& r = w.r;
  const size_t K = (size_t)f.ocap;
  HostPool::get().run((size_t)count, count >= 4 ? 8 : 1, [&](size_t b) {
    if (!src[b].runs()) return;
    const int32_t* kf_mp = src[b].mp();
    const dvm_track_refkf_params* p = &ps[b];
    const dvm_track_refkf_out* out = &outs[b];
    dvm_track_refkf_result* q = &res[b];
    const int N = f.ns[b];
    const int32_t* cnt = r.cnt + 8 * b;
    q->n = N; q->mono_index = f.monos[b];
    q->n_bow = cnt[0]; q->n_fv = cnt[1]; q->nmatches_before_rotation = cnt[2]; q->nmatches = cnt[3];
    const int32_t* fo = r.fv_off + b * (K + 1);
    if (out->bow_ids) std::memcpy(out->bow_ids, r.bow_ids + b * K, (size_t)q->n_bow * 4);
    if (out->bow_vals) std::memcpy(out->bow_vals, r.bow_vals + b * K, (size_t)q->n_bow * 8);
    if (out->fv_node) std::memcpy(out->fv_node, r.fv_node + b * K, (size_t)q->n_fv * 4);
    if (out->fv_off) std::memcpy(out->fv_off, fo, ((size_t)q->n_fv + 1) * 4);
    if (out->fv_feat) std::memcpy(out->fv_feat, r.fv_feat + b * K, (size_t)fo[q->n_fv] * 4);
    // mvpMapPoints: SearchByBoW's matches, those PoseOptimization rejected dropped (Tracking.cc:2486-2516)
    const bool few = q->nmatches < p->min_matches;
    const int32_t* match = r.match + b * K;
    const uint8_t* outl = r.outlier + b * K;
    for (int j = 0; j < N; j++) {
      const int a = match[j];
      const int id = a >= 0 ? kf_mp[a] : -1;
      const bool o = !few && id >= 0 && outl[j];
      out->mp_out[j] = o ? -1 : id; out->dropped[j] = o ? id : -1; out->outlier[j] = o ? 1 : 0;
    }
    if (few) {
      q->status = DVM_TRACK_FEW_MATCHES;
      std::memcpy(q->pose, p->pose_in, 56);
    } else {
      q->n_edges = r.nedges[b]; q->n_inliers = r.n_inl[b]; q->nmatches_map = r.fin[4 * b]; q->nmatches_after = r.fin[4 * b + 1];
      std::memcpy(q->pose, r.pose + 7 * b, 56);
      q->status = q->nmatches_map < p->min_map ? DVM_TRACK_FEW_MAP_MATCHES : DVM_TRACK_COMPLETE;
    }
    for (int k = 0; k < 3; k++) q->Tcw.t[k] = (float)q->pose[k];
    for (int k = 0; k < 4; k++) q->Tcw.q[k] = (float)q->pose[3 + k];
    status[b] = q->status; f.status[b] = q->status;
    std::memcpy(f.poses.data() + 7 * b, q->pose, 56);
  });
  if (count == 1) f.ready = f.status[0] == DVM_TRACK_COMPLETE;     // and dvm_track_local_map on the one frame
}
}  // namespace

int dvm_tracker_reserve_reference_keyframe(dvm_tracker* t, int max_kf_keypoints) {
  if (!t || max_kf_keypoints < 1) return DVM_ERR_INVALID;
  if (t->max_frames != 1) { set_error("dvm_tracker_reserve_reference_keyframe: a single-frame tracker (dvm_tracker_create)"); return DVM_ERR_STATE; }
  if (max_kf_keypoints > kFrameCap) { set_error("dvm_tracker_reserve_reference_keyframe: more than 8 192 keyframe keypoints"); return DVM_ERR_CAPACITY; }
  t->rk_cap = 0;
  const int rc = reserve_refkf(t, t->rk, ((size_t)max_kf_keypoints + 63) & ~(size_t)63, "dvm_tracker_reserve_reference_keyframe");
  if (rc == DVM_OK) t->rk_cap = max_kf_keypoints;
  return rc;
}

int dvm_track_reference_keyframe(dvm_tracker* t, dvm_orb* h, const dvm_vocab* voc, const dvm_ref_keyframe* kf, const dvm_track_refkf_params* p,
                                 dvm_track_refkf_out* out, dvm_track_refkf_result* res) {
  if (!t || !h || !voc || !kf || !p || !out || !res) return DVM_ERR_INVALID;
  if (t->max_frames != 1 || !t->rk_state || t->rk_h != h || orb_result_serial(h) != t->rk_serial) {
    set_error("dvm_track_reference_keyframe: not right after a dvm_track_begin or dvm_track_finish of one frame (single-frame tracker, same "
              "extractor), or already run on that frame");
    return DVM_ERR_STATE;
  }
  if (!t->rk.ws.d) { set_error("dvm_track_reference_keyframe: no dvm_tracker_reserve_reference_keyframe on this tracker"); return DVM_ERR_STATE; }
  const int form = t->rk_state;
  int rc = check_refkf_frame("dvm_track_reference_keyframe", kf, p, out, t->rk_cap);
  if (rc != DVM_OK) return rc;
  if (form == 1 && !(p->bounds[1] > p->bounds[0] && p->bounds[3] > p->bounds[2])) {
    set_error("dvm_track_reference_keyframe: form (a) builds the grid: empty frame bounds"); return DVM_ERR_INVALID;
  }
  if (vocab_device(voc) != t->device) { set_error("dvm_track_reference_keyframe: the vocabulary lives on another device"); return DVM_ERR_INVALID; }
  if (form == 1 && kb8_with_distortion(t->model, p->dist)) {
    set_error("dvm_track_reference_keyframe: distortion coefficients under a KannalaBrandt8 camera model (such a frame has mvKeysUn = mvKeys, mDistCoef zero)");
    return DVM_ERR_INVALID;
  }
  std::memset(res, 0, sizeof(*res));
  t->clear_next();   // once per begin; the second half waits for this call's status
  DVM_HIP(hipSetDevice(t->device));
  hipStream_t s = (hipStream_t)dvm_orb_stream(h);
  LocalFrame& f = t->lf;
  const bool undist = form == 1 && p->dist && p->dist->k1 != 0.0f;
  if (form == 1) {
    // what dvm_track_finish does before its search -- mvKeysUn (Frame.cc:791-818) and AssignFeaturesToGrid -- and what it leaves for the
    // second half, as a finish of one frame (the keypoint count and monoIndex from the download below)
    const dvm_keypoint* d_kps = nullptr; const uint8_t* d_desc = nullptr; const int32_t* d_n = nullptr; int ocap = 0;
    rc = dvm_orb_result_device(h, 0, &d_kps, &d_desc, &d_n, &ocap);
    if (rc != DVM_OK) return rc;
    if (ocap > t->kp_cap) { set_error("dvm_track_reference_keyframe: the extractor's keypoint capacity exceeds the tracker's"); return DVM_ERR_CAPACITY; }
    const dvm_keypoint* un = d_kps;
    if (undist) {
      rc = dvm_undistort_keypoints(p->dist, d_kps, reinterpret_cast<dvm_keypoint*>(t->dv.kps_un), ocap, 1, s);
      if (rc != DVM_OK) return rc;
      un = reinterpret_cast<const dvm_keypoint*>(t->dv.kps_un);
      if (out->kps_un) DVM_HIP(hipMemcpyAsync(t->m.kps_un, t->dv.kps_un, (size_t)ocap * sizeof(dvm_keypoint_pod), hipMemcpyDeviceToHost, s));
    }
    rc = dvm_frame_build_batch(t->grid, 0, 1, un, ocap, d_desc, (int64_t)ocap * 32, d_n, p->bounds[0], p->bounds[1], p->bounds[2], p->bounds[3], s);
    if (rc != DVM_OK) return rc;
    f.h = h; f.serial = orb_result_serial(h); f.ocap = ocap; f.nlevels = p->nlevels;
    f.d_un = reinterpret_cast<const dvm_keypoint_pod*>(un); f.d_n = d_n;
    std::memcpy(f.bounds, p->bounds, 16); std::memset(f.inv_sigma2, 0, sizeof(f.inv_sigma2));
    std::memcpy(f.inv_sigma2, p->inv_level_sigma2, (size_t)p->nlevels * 4); f.cam = p->cam; f.model = t->model;
    f.count = 1; f.kps_stride = ocap; f.d_desc = d_desc; f.desc_stride = (int64_t)ocap * 32;
    f.ns.assign(1, 0); f.status.assign(1, 0); f.monos.assign(1, 0); f.poses.assign(7, 0.0);
    f.kf_ready = 1;
  }
  // the batched chain on the one frame
  int32_t status = 0;
  int nrun = 0;
  size_t T = 0;
  RefKfSource src;
  src.kf = kf;
  rc = refkf_enqueue("dvm_track_reference_keyframe", t, t->rk, h, voc, 1, &src, nullptr, t->rk_cap, p, out, res, &status, &nrun, &T);
  if (rc != DVM_OK) return rc;
  // ONE synchronisation (behind the download of the extraction in form (a))
  if (form == 1) {
    // (without kps but with kps_un and no distortion: mvKeysUn = mvKeys is downloaded into kps_un directly)
    dvm_keypoint* kp = out->kps ? out->kps : undist ? nullptr : out->kps_un;
    uint8_t* dp = out->desc;
    const int cap = kp || dp ? out->cap : f.ocap;
    rc = dvm_orb_download_batch(h, 1, &kp, &dp, &cap, f.ns.data(), f.monos.data());
    if (rc != DVM_OK) return rc;
    if (out->kps_un && kp != out->kps_un)
      std::memcpy(out->kps_un, undist ? reinterpret_cast<const dvm_keypoint*>(t->m.kps_un) : out->kps, (size_t)f.ns[0] * sizeof(dvm_keypoint));
  } else {
    DVM_HIP(hipStreamSynchronize(s));
  }
  refkf_copy_out(t, t->rk, 1, &src, p, out, res, &status);
  return DVM_OK;
}

int dvm_tracker_reserve_reference_keyframe_batch(dvm_tracker* t, int max_total_kf_keypoints) {
  if (!t || max_total_kf_keypoints < 1) return DVM_ERR_INVALID;
  if ((int64_t)max_total_kf_keypoints > (int64_t)t->max_frames * kFrameCap) {
    set_error("dvm_tracker_reserve_reference_keyframe_batch: more than 8 192 keyframe keypoints per frame"); return DVM_ERR_CAPACITY;
  }
  return reserve_refkf(t, t->rkb, ((size_t)max_total_kf_keypoints + 63) & ~(size_t)63, "dvm_tracker_reserve_reference_keyframe_batch");
}

namespace {
// both batched entry points behind their argument checks: the state rules, the chain, ONE synchronisation, the results
int refkf_batch_run(const char* fn, dvm_tracker* t, dvm_orb* h, const dvm_vocab* voc, int count, std::vector<RefKfSource>& src, const dvm_keyframe_store* store,
                    const dvm_track_refkf_params* ps, const dvm_track_refkf_out* outs, dvm_track_refkf_result* res, int32_t* status) {
  LocalFrame& f = t->lf;
  const std::string sfn = fn;
  if (!f.rkb_ready || f.h != h || orb_result_serial(h) != f.serial || f.count != count) {
    set_error(sfn + ": not right after a dvm_track_finish[_batch] of `count` frames (same tracker and extractor), or already run on that finish");
    return DVM_ERR_STATE;
  }
  if (!t->rkb.ws.d) { set_error(sfn + ": no dvm_tracker_reserve_reference_keyframe_batch on this tracker"); return DVM_ERR_STATE; }
  static const bool timing = std::getenv("DVM_TRACK_BATCH_TIMING") != nullptr;       // host-side phase times on stderr
  using clk = std::chrono::steady_clock;
  const clk::time_point tp0 = clk::now();
  int nrun = 0;
  size_t T = 0;
  int rc = refkf_enqueue(fn, t, t->rkb, h, voc, count, src.data(), store, kFrameCap, ps, outs, res, status, &nrun, &T);
  if (rc != DVM_OK || !nrun) return rc;
  const clk::time_point tp1 = clk::now();
  DVM_HIP(hipStreamSynchronize((hipStream_t)dvm_orb_stream(h)));
  const clk::time_point tp2 = clk::now();
  refkf_copy_out(t, t->rkb, count, src.data(), ps, outs, res, status);
  if (timing) {
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    std::fprintf(stderr, "track reference keyframe batch of %d (%d run, %zu entries): pack + enqueue %.3f  wait %.3f  results out %.3f ms\n", count,
                 nrun, T, ms(tp0, tp1), ms(tp1, tp2), ms(tp2, clk::now()));
  }
  return DVM_OK;
}
}  // namespace

int dvm_track_reference_keyframe_batch(dvm_tracker* t, dvm_orb* h, const dvm_vocab* voc, int count, const dvm_ref_keyframe* const* kfs,
                                       const dvm_track_refkf_params* ps, const dvm_track_refkf_out* outs, dvm_track_refkf_result* res, int32_t* status) {
  if (!t || !h || !voc || !kfs || !ps || !outs || !res || !status || count < 1) return DVM_ERR_INVALID;
  std::vector<RefKfSource> src((size_t)count);
  for (int b = 0; b < count; b++) src[b].kf = kfs[b];
  return refkf_batch_run("dvm_track_reference_keyframe_batch", t, h, voc, count, src, nullptr, ps, outs, res, status);
}

int dvm_track_reference_keyframe_batch_resident(dvm_tracker* t, dvm_orb* h, const dvm_vocab* voc, const dvm_keyframe_store* kfs, int count,
                                                const dvm_kf_resident* const* kf, const dvm_track_refkf_params* ps, const dvm_track_refkf_out* outs,
                                                dvm_track_refkf_result* res, int32_t* status) {
  if (!t || !h || !voc || !kfs || !kf || !ps || !outs || !res || !status || count < 1) return DVM_ERR_INVALID;
  std::vector<RefKfSource> src((size_t)count);
  for (int b = 0; b < count; b++) src[b].r = kf[b];
  return refkf_batch_run("dvm_track_reference_keyframe_batch_resident", t, h, voc, count, src, kfs, ps, outs, res, status);
}

// Tracking::CreateNewKeyFrame on frames of the last finish: dvm_keyframe_store_put_device (keyframe_store.cpp) on the frames' mvKeysUn and
// descriptors where the finish left them, behind the extractor's stream.  The flag is LocalFrame::kf_ready: only a begin clears it.
int dvm_keyframe_store_put_tracked(dvm_keyframe_store* st, dvm_tracker* t, dvm_orb* h, const dvm_vocab* voc, int levelsup, int n, const int32_t* frames,
                                   const int32_t* slots, const dvm_kfs_device_keyframe* tables, dvm_kfs_bow_out* outs) {
  const char* fn = "dvm_keyframe_store_put_tracked";
  if (!st || !t || !h || !voc || n < 0 || (n && (!frames || !slots || !tables))) { set_error(std::string(fn) + ": missing argument"); return DVM_ERR_INVALID; }
  const LocalFrame& f = t->lf;
  if (!f.kf_ready || f.h != h || orb_result_serial(h) != f.serial) {
    set_error(std::string(fn) + ": not after a dvm_track_finish[_batch] or form (a) of dvm_track_reference_keyframe on this tracker and extractor, "
                                "or a begin has run since");
    return DVM_ERR_STATE;
  }
  if (kfs_device(st) != t->device) { set_error(std::string(fn) + ": the store lives on another device"); return DVM_ERR_INVALID; }
  std::vector<dvm_kfs_device_keyframe> kfs((size_t)n);
  for (int k = 0; k < n; k++) {
    const int b = frames[k];
    if (b < 0 || b >= f.count) { set_error(std::string(fn) + ": keyframe " + std::to_string(k) + ": frame outside [0, count)"); return DVM_ERR_INVALID; }
    kfs[k] = tables[k];
    kfs[k].d_kps = reinterpret_cast<const dvm_keypoint*>(f.d_un + (size_t)b * f.kps_stride);
    kfs[k].d_desc = f.d_desc + (size_t)b * f.desc_stride;
    kfs[k].d_n = f.d_n + b;
    kfs[k].n = f.ocap;
  }
  return kfs_put_device_run(fn, st, voc, levelsup, (hipStream_t)dvm_orb_stream(h), n, slots, kfs.data(), outs);
}

int dvm_tracker_last_refkf_upload_bytes(const dvm_tracker* t, int64_t* bytes) {
  if (!t || !bytes) return DVM_ERR_INVALID;
  *bytes = t->up_refkf;
  return DVM_OK;
}

}  // extern "C"
