// dvm_slam_amd/csrc/ba_window.cpp -- the C entry points of the window optimizers (dvm_ba_optimize_windows, dvm_ba_optimize_windows_fast[_cam],
// dvm_ba_pool_*) and the host bookkeeping of a call that both launchers share (WinCall, ba_window_common.h).  The kernels and their
// launchers: ba_window_seq.hip (g2o's summation order, the oracle's bits) and ba_window_cluster.hip (tree sums, G workgroups per window).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "ba_kernels.h"
#include "ba_window_common.h"
#include "group_commit.h"

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

}  // extern "C"
