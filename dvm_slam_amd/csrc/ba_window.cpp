// dvm_slam_amd/csrc/ba_window.cpp -- the C entry points of the window optimizers (dvm_ba_optimize_windows, dvm_ba_optimize_windows_fast[_cam],
// dvm_ba_pool_*, dvm_ba_resident_*) and the host bookkeeping of a call that both launchers share (WinCall, ba_window_common.h).  The kernels and their
// launchers: ba_window_seq.hip (g2o's summation order, the oracle's bits) and ba_window_cluster.hip (tree sums, G workgroups per window);
// ba_window_resident.hip: the gather and prepare kernels of the windows that read resident stores.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "ba_kernels.h"
#include "ba_resident_lists.h"
#include "ba_window_common.h"
#include "chain.h"
#include "group_commit.h"
#include "keyframe_store.h"
#include "map_store.h"

using namespace dvm;

namespace {
struct StopWord {                      // a word of page-locked host memory the kernel polls; the host copies the caller's flag into it
  int* h = nullptr; int* d = nullptr;
  ~StopWord() { if (h) hipHostFree(h); }
  int ensure() {
    if (h) return DVM_OK;
    int rc = hip_check(hipHostMalloc(reinterpret_cast<void**>(&h), 64, hipHostMallocMapped), "hipHostMalloc(stop word)");
    if (rc != DVM_OK) { h = nullptr; return rc; }
    return hip_check(hipHostGetDevicePointer(reinterpret_cast<void**>(&d), h, 0), "hipHostGetDevicePointer");
  }
};
}  // namespace

int WinCall::arm(int** stop_dev) {
  thread_local StopWord sw;
  const int rc = sw.ensure();
  if (rc != DVM_OK) return rc;
  *sw.h = (stop_flag && *stop_flag) ? 1 : 0;
  stop_host = sw.h;
  *stop_dev = sw.d;
  return DVM_OK;
}
// one contiguous span to fetch, straight into the caller's arrays where it gave any
void WinCall::add_outputs(Stage& st) {
  static const bool want_prof = std::getenv("DVM_BA_WINDOW_PROF") != nullptr;
  sl.resize(K); st_out.resize(K); prof_out.assign(K, std::vector<unsigned long long>(16, 0)); prof_zero.assign(16, 0);
  for (int k = 0; k < K; k++) {
    const dvm_ba_window& w = windows[k];
    Slots& s = sl[k];
    const size_t P = w.n_poses, L = w.n_points, E = w.n_edges;
    s.out_poses = (w.poses_out && P) ? st.out(w.poses_out, 56 * P) : st.scratch(56 * P);
    s.out_pts = (w.points_out && L) ? st.out(w.points_out, 24 * L) : st.scratch(24 * L);
    s.echi = (w.edge_chi2_out && E) ? st.out(w.edge_chi2_out, 8 * E) : st.scratch(8 * E);
    s.edepth = (w.depth_positive_out && E) ? st.out(w.depth_positive_out, E) : st.scratch(E);
    s.stats = st.out(&st_out[k], sizeof(dvm_ba_stats));
    s.prof = want_prof ? st.add(prof_zero.data(), prof_out[k].data(), 128) : -1;
  }
}
static double ms(WinCall::clock::time_point a, WinCall::clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
int WinCall::wait(Stage& st, int G) {
  if (stop_flag) {                     // g2o's forceStopFlag: written by another thread while the optimisation runs (LocalMapping.cc:305,359)
    hipEvent_t ev;
    DVM_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    DVM_HIP(hipEventRecord(ev, st.stream()));
    while (hipEventQuery(ev) == hipErrorNotReady) *stop_host = *stop_flag ? 1 : 0;
    hipEventDestroy(ev);
  }
  mark(6);
  const int rc = st.download();
  mark(7);
  if (rc == DVM_OK && std::getenv("DVM_BA_WINDOW_TIMING"))
    std::fprintf(stderr, "windows K=%d G=%d: build %.2f  register %.2f  layout %.2f  views %.2f  upload(memcpy + enqueue) %.2f  launch %.2f  wait + download %.2f ms\n", K, G,
                 ms(t[0], t[1]), ms(t[1], t[2]), ms(t[2], t[3]), ms(t[3], t[4]), ms(t[4], t[5]), ms(t[5], t[6]), ms(t[6], t[7]));
  return rc;
}
void WinCall::finish(dvm_ba_stats* stats, const char* const* phase_names, int kernel_us) {
  for (int i = 0; i < 16; i++)        // (all zeros without DVM_BA_WINDOW_PROF)
    if (prof_out[0][i]) std::fprintf(stderr, "window 0: %-24s %10.1f us\n", phase_names[i], prof_out[0][i] / 2400.0);   // s_memtime ticks at the shader clock (MI355X_MICROARCH.md): us at 2.4 GHz
  for (int k = 0; stats && k < K; k++) {
    stats[k] = st_out[k];
    if (kernel_us >= 0) stats[k].kernel_us = kernel_us;
    stats[k].ms_structure = ms(t[0], t[1]) / K;
    stats[k].ms_optimize = ms(t[1], t[7]);     // the whole batch: upload, the one launch, download
  }
}

extern "C" {

int dvm_ba_optimize_windows(int device, const dvm_ba_window* windows, int K, const volatile uint8_t* stop_flag, dvm_ba_stats* stats) {
  return ba_windows_seq(device, windows, K, stop_flag, stats, /*normalize_input=*/true);
}
int dvm_ba_optimize_windows_fast(int device, const dvm_ba_window* windows, int K, const volatile uint8_t* stop_flag, dvm_ba_stats* stats) {
  // DVM_BA_SPLIT: a batch of 64 or more windows in two halves, the second on a persistent helper thread with its own staging buffers and
  // stream; the two launches (G workgroups per window each) share the chip.  Every window's result is independent of its batch and of G, so
  // the split changes nothing but the time.  It was the default while the host side of such a call (tables, 60+ MB through a staging copy)
  // was as long as its kernel (128 windows: 23 -> 18 ms); with the tables sent from the builders' threads the one launch is the faster and
  // the steadier form (128 windows: 17.0-17.2 ms against 15.5-19.5).
  const bool split = std::getenv("DVM_BA_SPLIT") != nullptr;       // (read at every call: the tests take both paths)
  if (K >= 64 && split) {
    if (K < 0 || !windows) { set_error("dvm_ba_optimize_windows: null windows"); return DVM_ERR_INVALID; }
    HelperThread& H = HelperThread::get();
    std::unique_lock<std::mutex> user(H.use, std::try_to_lock);
    if (user.owns_lock()) {
      const int K0 = (K + 1) / 2, K1 = K - K0;
      // the cluster size of BOTH launches from the whole batch: their workgroups must all be resident together (two half grids that each
      // filled the chip would starve each other's barriers)
      const int G = ba_cluster_size(device, 8 * ((K0 + 7) / 8) + 8 * ((K1 + 7) / 8), 0);
      int rc1 = DVM_OK;
      std::string err1;
      H.submit([&, K0, K1, G] {
        rc1 = ba_windows_cluster(device, windows + K0, K1, stop_flag, stats ? stats + K0 : nullptr, G, nullptr);
        if (rc1 != DVM_OK) err1 = last_error_cstr();
      });
      const int rc0 = ba_windows_cluster(device, windows, K0, stop_flag, stats, G, nullptr);
      H.wait();
      if (rc0 != DVM_OK) return rc0;
      if (rc1 != DVM_OK) { set_error(err1); return rc1; }
      return DVM_OK;
    }
  }
  return ba_windows_cluster(device, windows, K, stop_flag, stats, 0, nullptr);
}
// dvm_ba_optimize_windows_fast with a camera model per window.  A model 0 window becomes the pinhole window of (double)p[0..3]: from there on it
// IS a window of dvm_ba_optimize_windows_fast.  (DVM_BA_SPLIT is not honoured here.)
int dvm_ba_optimize_windows_fast_cam(int device, const dvm_ba_window* windows, const dvm_camera_model* models, int K, const volatile uint8_t* stop_flag,
                                     dvm_ba_stats* stats) {
  if (K < 0 || (K && (!windows || !models))) { set_error("dvm_ba_optimize_windows_fast_cam: NULL windows or models"); return DVM_ERR_INVALID; }
  for (int k = 0; k < K; k++)
    if (!dvm_cam::model_ok(models[k].model, models[k].p)) { set_error("dvm_ba_optimize_windows_fast_cam: unknown model or zero focal length (window " + std::to_string(k) + ")"); return DVM_ERR_INVALID; }
  if (K == 0) return DVM_OK;
  std::vector<dvm_ba_window> w(windows, windows + K);
  for (int k = 0; k < K; k++)
    if (models[k].model == dvm_cam::kPinhole) { w[k].cam.fx = (double)models[k].p[0]; w[k].cam.fy = (double)models[k].p[1]; w[k].cam.cx = (double)models[k].p[2]; w[k].cam.cy = (double)models[k].p[3]; }
  return ba_windows_cluster(device, w.data(), K, stop_flag, stats, 0, models);
}

// ---- dvm_ba_pool_*: the LocalBundleAdjustment calls of several agents' LocalMapping threads (one per agent in the reference:
// LocalMapping.cc:172 -> Optimizer.cc:1030-1387), each a BLOCKING call with its own window, batched behind the boundary into one launch
// of the cluster form (group commit, as dvm_orb_pool / dvm_match_pool / dvm_pose_pool do it for the tracking threads' per-frame calls).
// A window's result does not depend on the batch it rode in (k_ba_window_cluster): every caller gets the bits of a solo
// dvm_ba_optimize_windows_fast call.
struct dvm_ba_pool {
  int device = 0;
  GroupCommit gc;
  std::vector<dvm_ba_window> win[GroupCommit::kLanes];
  std::vector<dvm_ba_stats> st[GroupCommit::kLanes];
  std::vector<dvm_camera_model> mod[GroupCommit::kLanes];   // the windows' models (model 0 with cam as the window has it: a call without one)
};
int dvm_ba_pool_create(int device, int max_batch, int window_us, dvm_ba_pool** out) {
  if (!out || max_batch < 1 || max_batch > 256) return DVM_ERR_INVALID;
  *out = nullptr;
  int rc = dvm_set_device(device);
  if (rc != DVM_OK) return rc;
  dvm_ba_pool* p = new (std::nothrow) dvm_ba_pool();
  if (!p) return DVM_ERR_INVALID;
  p->device = device;
  p->gc.max_batch = max_batch;
  p->gc.window_us = window_us >= 0 ? window_us : 300;     // a LocalBundleAdjustment call takes milliseconds: 0.3 ms of collecting costs little
  for (int l = 0; l < GroupCommit::kLanes; l++) { p->win[l].resize((size_t)max_batch); p->st[l].resize((size_t)max_batch); p->mod[l].resize((size_t)max_batch); }
  *out = p;
  return DVM_OK;
}
void dvm_ba_pool_destroy(dvm_ba_pool* pool) { delete pool; }
// one window through the pool; model NULL: the pinhole camera of w->cam.  Calls of every model type collect in the same lane: the batch is one
// call of the cluster form, which groups its windows by type
static int ba_pool_optimize(dvm_ba_pool* pool, const dvm_ba_window* w, const dvm_camera_model* model, dvm_ba_stats* stats, int* batch_size) {
  if (!pool || !w) return DVM_ERR_INVALID;
  if (w->n_poses < 1 || w->n_points < 0 || w->n_edges < 0 || w->iterations < 0 || !w->poses || !w->fixed || (w->n_points && !w->points) || (w->n_edges && !w->edges)) {
    set_error("dvm_ba_pool_optimize: the window is incomplete");
    return DVM_ERR_INVALID;
  }
  const int64_t key[4] = {0, 0, 0, 0};
  int li = 0, slot = 0;
  int rc = pool->gc.join(key, [](int) { return 0; }, li, slot);
  if (rc != 0) return rc;
  pool->win[li][(size_t)slot] = *w;                       // (the arrays stay the caller's: it is blocked here until the batch is through)
  dvm_camera_model& sm = pool->mod[li][(size_t)slot];
  std::memset(&sm, 0, sizeof(sm));
  if (model) {
    sm = *model;
    if (model->model == dvm_cam::kPinhole) {
      dvm_ba_camera& c = pool->win[li][(size_t)slot].cam;
      c.fx = (double)model->p[0]; c.fy = (double)model->p[1]; c.cx = (double)model->p[2]; c.cy = (double)model->p[3];
    }
  }
  if (pool->gc.arrive(li, slot)) {
    const int count = pool->gc.batch_count(li);
    // the batch runs on the library's helper thread, whichever caller leads it: ONE set of page-locked / device staging buffers and
    // window tables for the service instead of one per agent thread (they are thread-local: ~5 MB per window of the largest batch)
    int brc = DVM_OK;
    std::string berr;
    {
      HelperThread& H = HelperThread::get();
      std::lock_guard<std::mutex> user(H.use);
      H.submit([&] {
        brc = dvm_set_device(pool->device);
        bool any_kb8 = false;
        for (int k = 0; k < count; k++) any_kb8 = any_kb8 || pool->mod[li][(size_t)k].model == dvm_cam::kKannalaBrandt8;
        if (brc == DVM_OK)
          brc = any_kb8 ? ba_windows_cluster(pool->device, pool->win[li].data(), count, nullptr, pool->st[li].data(), 0, pool->mod[li].data())
                        : dvm_ba_optimize_windows_fast(pool->device, pool->win[li].data(), count, nullptr, pool->st[li].data());
        if (brc != DVM_OK) berr = last_error_cstr();
      });
      H.wait();
    }
    pool->gc.publish(li, brc, berr);
  }
  std::string err;
  int count = 0;
  rc = pool->gc.result(li, &err, &count);
  if (rc == DVM_OK && stats) *stats = pool->st[li][(size_t)slot];
  if (batch_size) *batch_size = count;
  pool->gc.finish(li);
  if (rc != DVM_OK) set_error("dvm_ba_pool_optimize: " + err);
  return rc;
}

int dvm_ba_pool_optimize(dvm_ba_pool* pool, const dvm_ba_window* w, dvm_ba_stats* stats, int* batch_size) {
  return ba_pool_optimize(pool, w, nullptr, stats, batch_size);
}
int dvm_ba_pool_optimize_cam(dvm_ba_pool* pool, const dvm_ba_window* w, const dvm_camera_model* model, dvm_ba_stats* stats, int* batch_size) {
  if (!model || !dvm_cam::model_ok(model->model, model->p)) { set_error("dvm_ba_pool_optimize_cam: NULL model, unknown model or zero focal length"); return DVM_ERR_INVALID; }
  return ba_pool_optimize(pool, w, model, stats, batch_size);
}

// ---- dvm_ba_resident_*: LocalBundleAdjustment windows that read the keyframe store and the map store and commit to the map store on the
// device (include/dvmslam_hip.h).  This file: the handle, every check -- all on the host, before anything is queued --, the commit's
// bookkeeping.  The kernels: ba_window_resident.hip; the launcher: ba_windows_cluster with a ResidentCall; the scatter: map_store.cpp.
struct dvm_ba_resident {
  int device = 0;
  uint8_t* d = nullptr; size_t dcap = 0;          // what the prepare kernels leave and a commit reads, all windows of the last optimize
  struct Win { dvm_map_store* store; float* geom; uint8_t* state; int32_t* slot; float* ow; int32_t L; bool has_ref, committed; };
  std::vector<Win> win;
  bool valid = false;                             // the last optimize succeeded
  std::vector<hipEvent_t> ev; int n_pending = 0;  // behind the queued commits' scatters: the next optimize's prepare kernels wait for them
  int64_t h2d = 0, d2h = 0;
  // per-call scratch, kept with the handle
  std::vector<std::vector<ResidentKf>> kf;
  std::vector<ResidentLists> lists;
};

int dvm_ba_resident_create(int device, dvm_ba_resident** out) {
  if (!out) return DVM_ERR_INVALID;
  *out = nullptr;
  const int rc = need_device(device);
  if (rc != DVM_OK) return rc;
  dvm_ba_resident* h = new (std::nothrow) dvm_ba_resident();
  if (!h) return DVM_ERR_INVALID;
  h->device = device;
  *out = h;
  return DVM_OK;
}
void dvm_ba_resident_destroy(dvm_ba_resident* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  for (int i = 0; i < h->n_pending; i++) (void)hipEventSynchronize(h->ev[i]);     // a queued commit still reads h->d
  for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
  if (h->d) (void)hipFree(h->d);
  delete h;
}

static int resident_refuse(int k, const std::string& what) {
  set_error("dvm_ba_resident_optimize: window " + std::to_string(k) + ": " + what);
  return DVM_ERR_INVALID;
}

int dvm_ba_resident_optimize(dvm_ba_resident* h, const dvm_ba_window_resident* windows, const dvm_camera_model* models, int K,
                             const volatile uint8_t* stop_flag, dvm_ba_stats* stats) {
  if (!h) return DVM_ERR_INVALID;
  h->valid = false;
  if (K < 0 || (K && !windows)) { set_error("dvm_ba_resident_optimize: NULL windows"); return DVM_ERR_INVALID; }
  for (int k = 0; models && k < K; k++)
    if (!dvm_cam::model_ok(models[k].model, models[k].p)) return resident_refuse(k, "unknown model or zero focal length");
  // every check of every window, on the host, before the device is touched
  if ((int)h->kf.size() < K) { h->kf.resize(K); h->lists.resize(K); }
  std::vector<dvm_ba_window> win(K);
  // (the windows are independent: checked by the pooled host threads that build their tables later -- 32 windows of 15 000 edges
  //  checked one after the other cost more than a millisecond of a 5 ms call)
  auto check = [&](int k) -> int {
    const dvm_ba_window_resident& w = windows[k];
    const int P = w.n_poses, L = w.n_points, E = w.n_edges;
    if (P < 0 || L < 0 || E < 0 || w.iterations < 0) return resident_refuse(k, "a negative count");
    if ((P && (!w.poses || !w.fixed || !w.keyframes || !w.kf_slot)) || (L && (!w.points || !w.mp_slot)) || (E && !w.obs)) return resident_refuse(k, "a NULL array");
    if (P && kfs_device(w.keyframes) != h->device) return resident_refuse(k, "the keyframe store lies on another device");
    if (L && store_device(w.points) != h->device) return resident_refuse(k, "the map store lies on another device");
    std::vector<ResidentKf>& kf = h->kf[k];
    kf.resize(P);
    static thread_local std::vector<int32_t> n_kp, sorted;
    n_kp.resize(P);
    for (int p = 0; p < P; p++) {
      KfSlotView v;
      if (!kfs_slot_view(w.keyframes, w.kf_slot[p], &v)) return resident_refuse(k, "keyframe slot " + std::to_string(w.kf_slot[p]) + " lies outside the store, was never written or has been removed");
      kf[p] = ResidentKf{v.kps, v.inv_sigma2, v.sf, v.n_levels, 0};
      n_kp[p] = v.n;
    }
    if (resident_lists_build(w.obs, P, L, E, h->lists[k]) != 0) return resident_refuse(k, "edge index out of range");
    for (int e = 0; e < E; e++)
      if (w.obs[e].kp < 0 || w.obs[e].kp >= n_kp[w.obs[e].pose]) return resident_refuse(k, "edge " + std::to_string(e) + ": keypoint " + std::to_string(w.obs[e].kp) + " outside its keyframe's [0, n)");
    if (L && !store_slots_ok(w.points, w.mp_slot, L)) return resident_refuse(k, "a map slot outside [0, capacity) or never written");
    sorted.assign(w.mp_slot, w.mp_slot + L);
    std::sort(sorted.begin(), sorted.end());
    for (int l = 1; l < L; l++) if (sorted[l] == sorted[l - 1]) return resident_refuse(k, "map slot " + std::to_string(sorted[l]) + " named twice");
    if (w.ref_edge) {
      int at = 0;
      const int bad = resident_ref_check(w.obs, L, E, h->lists[k], w.ref_edge, &at);
      if (bad) return resident_refuse(k, "ref_edge of point " + std::to_string(at) + (bad == 1 ? " out of range" : bad == 2 ? " is not an edge of that point" : " is -1 on a point that has edges"));
    }
    dvm_ba_window& o = win[k];
    std::memset(&o, 0, sizeof(o));
    o.n_poses = P; o.n_points = L; o.n_edges = E; o.iterations = w.iterations;
    o.poses = w.poses; o.fixed = w.fixed; o.cam = w.cam;
    if (models && models[k].model == dvm_cam::kPinhole) { o.cam.fx = (double)models[k].p[0]; o.cam.fy = (double)models[k].p[1]; o.cam.cx = (double)models[k].p[2]; o.cam.cy = (double)models[k].p[3]; }
    o.poses_out = w.poses_out; o.points_out = w.points_out; o.edge_chi2_out = w.edge_chi2_out; o.depth_positive_out = w.depth_positive_out;
    return win_graph(o, true, nullptr, resident_obs(w));     // (the limit of 30 free cameras)
  };
  {
    std::vector<int> rcs(K, DVM_OK);
    std::vector<std::string> errs(K);
    HostPool::get().run((size_t)K, 32, [&](size_t k) { if ((rcs[k] = check((int)k)) != DVM_OK) errs[k] = last_error_cstr(); });
    for (int k = 0; k < K; k++) if (rcs[k] != DVM_OK) { set_error(errs[k]); return rcs[k]; }     // (the first refused window names itself)
  }
  std::vector<const dvm_keyframe_store*> kf_stores;
  std::vector<const dvm_map_store*> map_stores;
  for (int k = 0; k < K; k++) {
    const dvm_ba_window_resident& w = windows[k];
    if (w.n_poses && std::find(kf_stores.begin(), kf_stores.end(), w.keyframes) == kf_stores.end()) kf_stores.push_back(w.keyframes);
    if (w.n_points && std::find(map_stores.begin(), map_stores.end(), w.points) == map_stores.end()) map_stores.push_back(w.points);
  }
  h->win.clear();
  h->h2d = h->d2h = 0;
  if (K == 0) { h->valid = true; return DVM_OK; }
  { const int rc = hip_check(hipSetDevice(h->device), "hipSetDevice"); if (rc != DVM_OK) return rc; }
  // the handle's block: per window geom [L][8], state [L], slot [L], ow [P][3]
  Cursor<256> cur{nullptr};
  for (int k = 0; k < K; k++) { cur.carve<float>(8 * (size_t)windows[k].n_points); cur.carve<uint8_t>((size_t)windows[k].n_points); cur.carve<int32_t>((size_t)windows[k].n_points); cur.carve<float>(3 * (size_t)windows[k].n_poses); }
  if (cur.used() > h->dcap) {
    for (int i = 0; i < h->n_pending; i++) DVM_HIP(hipEventSynchronize(h->ev[i]));     // a queued commit still reads the old block
    h->n_pending = 0;
    if (h->d) (void)hipFree(h->d);
    h->d = nullptr; h->dcap = 0;
    const size_t cap = std::max<size_t>(cur.used() * 2, (size_t)1 << 16);
    { const int rc = hip_check(hipMalloc(reinterpret_cast<void**>(&h->d), cap), "hipMalloc(prepared windows)"); if (rc != DVM_OK) { h->d = nullptr; return rc; } }
    h->dcap = cap;
  }
  std::vector<WinResident> src(K);
  std::vector<dvm_ba_resident::Win> prepared(K);
  cur = Cursor<256>{h->d};
  for (int k = 0; k < K; k++) {
    const dvm_ba_window_resident& w = windows[k];
    WinResident& r = src[k];
    r.w = &w; r.kf = h->kf[k].data(); r.records = w.n_points ? reinterpret_cast<const dvm_local_point*>(store_records(w.points)) : nullptr;
    r.pe_start = h->lists[k].pe_start.data(); r.pe_edges = h->lists[k].pe_edges.data();
    r.geom = cur.carve<float>(8 * (size_t)w.n_points); r.state = cur.carve<uint8_t>((size_t)w.n_points);
    r.slot = cur.carve<int32_t>((size_t)w.n_points); r.ow = cur.carve<float>(3 * (size_t)w.n_poses);
    prepared[k] = dvm_ba_resident::Win{w.points, r.geom, r.state, r.slot, r.ow, w.n_points, w.ref_edge != nullptr, false};
  }
  ResidentCall call;
  call.win = src.data();
  call.kf_stores = kf_stores.data(); call.n_kf_stores = (int)kf_stores.size();
  call.map_stores = map_stores.data(); call.n_map_stores = (int)map_stores.size();
  call.wait_ev = h->ev.data(); call.n_wait = h->n_pending;
  call.h2d = &h->h2d; call.d2h = &h->d2h;
  const int rc = ba_windows_cluster(h->device, win.data(), K, stop_flag, stats, 0, models, &call);
  if (rc != DVM_OK) return rc;
  h->n_pending = 0;                    // (the call's stream waited for them, and the call for its stream)
  h->win.swap(prepared);
  h->valid = true;
  return DVM_OK;
}

int dvm_ba_resident_commit(dvm_ba_resident* h, int k) {
  if (!h) return DVM_ERR_INVALID;
  if (!h->valid) { set_error("dvm_ba_resident_commit: no optimize has run on the handle, or the last one failed"); return DVM_ERR_STATE; }
  const int K = (int)h->win.size();
  if (k < -1 || k >= K) { set_error("dvm_ba_resident_commit: window " + std::to_string(k) + " outside the last optimize's [0, " + std::to_string(K) + ")"); return DVM_ERR_INVALID; }
  if (k >= 0 && h->win[k].committed) { set_error("dvm_ba_resident_commit: window " + std::to_string(k) + " has been committed"); return DVM_ERR_STATE; }
  if (k >= 0 && !h->win[k].has_ref) { set_error("dvm_ba_resident_commit: window " + std::to_string(k) + " was given no ref_edge"); return DVM_ERR_STATE; }
  std::vector<int> todo;
  for (int i = (k < 0 ? 0 : k); i < (k < 0 ? K : k + 1); i++)
    if (!h->win[i].committed && h->win[i].has_ref) todo.push_back(i);
  std::vector<dvm_map_store*> stores;
  for (int i : todo) if (h->win[i].L > 0 && std::find(stores.begin(), stores.end(), h->win[i].store) == stores.end()) stores.push_back(h->win[i].store);
  { const int rc = hip_check(hipSetDevice(h->device), "hipSetDevice"); if (rc != DVM_OK) return rc; }
  while (h->ev.size() < (size_t)h->n_pending + stores.size()) {
    hipEvent_t e = nullptr;
    DVM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    h->ev.push_back(e);
  }
  for (dvm_map_store* st : stores) {                // one scatter per distinct store
    std::vector<StoreCommitRange> ranges;
    for (int i : todo) if (h->win[i].store == st && h->win[i].L > 0) ranges.push_back(StoreCommitRange{h->win[i].geom, h->win[i].state, h->win[i].slot, h->win[i].L, 0});
    const int rc = store_commit_geometry(st, ranges.data(), (int)ranges.size(), h->ev[h->n_pending]);
    if (rc != DVM_OK) { h->valid = false; return rc; }
    h->n_pending++;
    for (int i : todo) if (h->win[i].store == st) h->win[i].committed = true;
  }
  for (int i : todo) h->win[i].committed = true;   // (windows without points)
  return DVM_OK;
}

int dvm_ba_resident_last_bytes(const dvm_ba_resident* h, int64_t* host_to_device, int64_t* device_to_host) {
  if (!h) return DVM_ERR_INVALID;
  if (host_to_device) *host_to_device = h->h2d;
  if (device_to_host) *device_to_host = h->d2h;
  return DVM_OK;
}

}  // extern "C"
