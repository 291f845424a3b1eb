// dvm_slam_amd/csrc/fuse_targets.cpp -- dvm_fuse_targets: the Fuse searches of LocalMapping::SearchInNeighbors against all target keyframes
// as one chain (include/dvmslam_hip.h; kernels in fuse_targets_kernels.hip).  The handle owns a stream and one reserved working set: a device
// block [target upload][grid spans][point table + mask][results] and a page-locked block [target staging][point staging][results].
// set: validates, packs every target back to back into the staging region, sends it with ONE copy and builds all grids with ONE launch; it
// does not wait.  run: packs the point table and the mask, ONE copy, ONE launch over (target, point), ONE copy back, ONE synchronisation.
#include <cstring>
#include <new>
#include <string>

#include "../../include/dvmslam_hip.h"
#include "fuse_targets_kernels.h"
#include "orb_pipeline.h"

using namespace dvm;

struct dvm_fuse_targets {
  int device = 0;
  hipStream_t s = nullptr;
  uint8_t *d = nullptr, *hp = nullptr;
  // device block: [tgt_bytes][grid_bytes][pts_bytes][res_bytes]; page-locked block: [tgt_bytes][pts_bytes][res_bytes]
  size_t tgt_bytes = 0, grid_bytes = 0, pts_bytes = 0, res_bytes = 0;
  int max_points = 0, max_targets = 0, max_total = 0;
  int n_targets = -1;                           // of the last set; -1: none yet
  int profiling = 0, build_timed = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  float last_ms[2] = {0, 0};
  void release() {
    if (d) hipFree(d);
    if (hp) hipHostFree(hp);
    d = hp = nullptr; tgt_bytes = grid_bytes = pts_bytes = res_bytes = 0; max_points = max_targets = max_total = 0; n_targets = -1;
  }
};

namespace {
constexpr size_t kAlign = 64;
constexpr int kMaxTargets = 65535;              // gridDim.y
constexpr int64_t kMaxEntries = (int64_t)1 << 27;   // target x point entries of one run
size_t al(size_t b) { return (b + kAlign - 1) & ~(kAlign - 1); }
// upload bytes of a target of n keypoints at most: keypoints, descriptors; two level tables of 64 and the rounding of its four arrays
constexpr size_t kUpPerKeypoint = sizeof(dvm_keypoint_pod) + 32, kUpFixed = 2 * 64 * 4 + 4 * kAlign;
// grid bytes: sorted keypoint, index, descriptor; cellx_start[80], the three counters and the rounding of its five arrays
constexpr size_t kGridPerKeypoint = sizeof(float4) + 4 + 32, kGridFixed = 80 * 4 + 5 * kAlign;
constexpr size_t kPointBytes = 12 + 12 + 4 + 4 + 32 + 1;

int fail(const char* fn, int rc, const std::string& msg) { set_error(std::string(fn) + ": " + msg); return rc; }
}  // namespace

extern "C" {

int dvm_fuse_targets_create(int device, dvm_fuse_targets** out) {
  if (!out) return DVM_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_error("no HIP device visible (libdvmslam_hip has no CPU path)"); return DVM_ERR_NO_DEVICE; }
  if (device < 0 || device >= n) { set_error("device index out of range"); return DVM_ERR_INVALID; }
  DVM_HIP(hipSetDevice(device));
  dvm_fuse_targets* h = new (std::nothrow) dvm_fuse_targets;
  if (!h) return DVM_ERR_INVALID;
  h->device = device;
  int rc = hip_check(hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking), "hipStreamCreate");
  if (rc != DVM_OK) { delete h; return rc; }
  *out = h;
  return DVM_OK;
}

void dvm_fuse_targets_destroy(dvm_fuse_targets* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->s) { hipStreamSynchronize(h->s); hipStreamDestroy(h->s); }
  for (hipEvent_t e : h->ev) if (e) hipEventDestroy(e);
  h->release();
  delete h;
}

int dvm_fuse_targets_reserve(dvm_fuse_targets* h, int max_points, int max_targets, int max_total_target_keypoints) {
  if (!h || max_points < 0 || max_targets < 0 || max_targets > kMaxTargets || max_total_target_keypoints < 0 ||
      (int64_t)max_total_target_keypoints > (int64_t)max_targets * kFrameCap || (int64_t)max_points * max_targets > kMaxEntries)
    return fail("dvm_fuse_targets_reserve", DVM_ERR_INVALID, "bad sizes");
  if (max_points <= h->max_points && max_targets <= h->max_targets && max_total_target_keypoints <= h->max_total) return DVM_OK;
  DVM_HIP(hipSetDevice(h->device));
  DVM_HIP(hipStreamSynchronize(h->s));
  const int np = std::max(max_points, h->max_points), nt = std::max(max_targets, h->max_targets), tot = std::max(max_total_target_keypoints, h->max_total);
  if ((int64_t)np * nt > kMaxEntries) return fail("dvm_fuse_targets_reserve", DVM_ERR_INVALID, "bad sizes");
  h->release();                                  // (the targets of an earlier set go with the block: set again)
  const size_t tgt = al(al((size_t)nt * sizeof(FtTargetDev)) + (size_t)tot * kUpPerKeypoint + (size_t)nt * kUpFixed);
  const size_t grid = al((size_t)tot * kGridPerKeypoint + (size_t)nt * kGridFixed + kAlign);
  const size_t pts = al((size_t)np * kPointBytes + 7 * kAlign + al((size_t)np * nt));
  const size_t res = 2 * al((size_t)np * nt * 4);
  if (hipMalloc(reinterpret_cast<void**>(&h->d), tgt + grid + pts + res) != hipSuccess) {
    h->d = nullptr;
    return fail("dvm_fuse_targets_reserve", DVM_ERR_HIP, "hipMalloc failed");
  }
  if (hipHostMalloc(reinterpret_cast<void**>(&h->hp), tgt + pts + res, hipHostMallocDefault) != hipSuccess) {
    h->hp = nullptr;
    h->release();
    return fail("dvm_fuse_targets_reserve", DVM_ERR_HIP, "page-locked host memory failed");
  }
  h->tgt_bytes = tgt; h->grid_bytes = grid; h->pts_bytes = pts; h->res_bytes = res;
  h->max_points = np; h->max_targets = nt; h->max_total = tot;
  return DVM_OK;
}

int dvm_fuse_targets_profiling(dvm_fuse_targets* h, int enable) {
  if (!h) return DVM_ERR_INVALID;
  DVM_HIP(hipSetDevice(h->device));
  if (enable)
    for (hipEvent_t& e : h->ev) if (!e) DVM_HIP(hipEventCreate(&e));
  h->profiling = enable != 0;
  return DVM_OK;
}
int dvm_fuse_targets_last_kernel_ms(dvm_fuse_targets* h, float* ms) {
  if (!h || !ms) return DVM_ERR_INVALID;
  ms[0] = h->last_ms[0]; ms[1] = h->last_ms[1];
  return DVM_OK;
}

int dvm_fuse_targets_set(dvm_fuse_targets* h, int n_targets, const dvm_ft_target* targets) {
  static_assert(sizeof(dvm_keypoint) == sizeof(dvm_keypoint_pod), "layout");
  const char* fn = "dvm_fuse_targets_set";
  if (!h || n_targets < 0 || (n_targets > 0 && !targets)) return fail(fn, DVM_ERR_INVALID, "missing argument");
  int64_t total = 0;
  for (int t = 0; t < n_targets; t++) {
    const dvm_ft_target& k = targets[t];
    const std::string w = "target " + std::to_string(t);
    if (k.n < 0 || k.n > kFrameCap) return fail(fn, DVM_ERR_INVALID, w + ": n outside [0, 8192]");
    if (k.n_levels < 1 || k.n_levels > 64) return fail(fn, DVM_ERR_INVALID, w + ": n_levels outside [1, 64]");
    if (!k.scale_factors || !k.inv_level_sigma2) return fail(fn, DVM_ERR_INVALID, w + ": missing level table");
    if (!(k.fx != 0.0f) || !(k.fy != 0.0f)) return fail(fn, DVM_ERR_INVALID, w + ": zero focal length");
    if (!(k.max_x > k.min_x) || !(k.max_y > k.min_y)) return fail(fn, DVM_ERR_INVALID, w + ": image bounds empty");
    if (k.n > 0 && (!k.kps || !k.desc)) return fail(fn, DVM_ERR_INVALID, w + ": missing keypoint array");
    // a candidate's octave indexes the level tables on the device (the 5.99 gate reads mvInvLevelSigma2[octave])
    for (int i = 0; i < k.n; i++)
      if ((uint32_t)k.kps[i].octave >= (uint32_t)k.n_levels) return fail(fn, DVM_ERR_INVALID, w + ": a keypoint's octave outside the level tables");
    total += k.n;
  }
  if (n_targets > h->max_targets || total > h->max_total)
    return fail(fn, DVM_ERR_CAPACITY, "beyond the reservation (dvm_fuse_targets_reserve): " + std::to_string(n_targets) + " targets with " +
                                          std::to_string(total) + " keypoints");
  h->n_targets = n_targets;
  if (n_targets == 0) return DVM_OK;
  DVM_HIP(hipSetDevice(h->device));
  DVM_HIP(hipStreamSynchronize(h->s));           // the staging region may still feed the copy of an earlier set (idle after a run: free)

  FtTargetDev* tab = reinterpret_cast<FtTargetDev*>(h->hp);
  size_t up = al((size_t)n_targets * sizeof(FtTargetDev));       // offset inside the upload region
  size_t go = h->tgt_bytes;                                      // offset of the grid spans inside the device block
  auto put = [&](const void* src, size_t bytes) {
    const size_t o = up;
    if (bytes) std::memcpy(h->hp + o, src, bytes);
    up = o + al(bytes);
    return h->d + o;
  };
  auto carve = [&](size_t bytes) { uint8_t* q = h->d + go; go += al(bytes); return q; };
  int32_t* n_overflow = reinterpret_cast<int32_t*>(carve(4));   // (never counted: every span holds its target exactly)
  for (int t = 0; t < n_targets; t++) {
    const dvm_ft_target& k = targets[t];
    FtTargetDev& D = tab[t];
    std::memset(&D, 0, sizeof(D));
    const size_t n = (size_t)k.n;
    D.kps = reinterpret_cast<const dvm_keypoint_pod*>(put(k.kps, n * sizeof(dvm_keypoint_pod)));
    D.desc = put(k.desc, n * 32);
    D.sf = reinterpret_cast<const float*>(put(k.scale_factors, (size_t)k.n_levels * 4));
    D.inv_sigma2 = reinterpret_cast<const float*>(put(k.inv_level_sigma2, (size_t)k.n_levels * 4));
    D.n = k.n;
    FrameView& F = D.F;
    F.skp = reinterpret_cast<float4*>(carve(n * sizeof(float4)));
    F.sidx = reinterpret_cast<int32_t*>(carve(n * 4));
    F.sdesc = carve(n * 32);
    F.cellx_start = reinterpret_cast<int32_t*>(carve(80 * 4));
    F.n_sorted = reinterpret_cast<int32_t*>(carve(8));
    F.n_total = F.n_sorted + 1;
    F.n_overflow = n_overflow;
    F.cap = k.n;
    F.minX = k.min_x; F.minY = k.min_y;
    F.wInv = static_cast<float>(64) / static_cast<float>(k.max_x - k.min_x);   // Frame.cc:443-444, as dvm_frame_build
    F.hInv = static_cast<float>(48) / static_cast<float>(k.max_y - k.min_y);
    ProjectCam& C = D.C;
    std::memcpy(C.q, k.Tcw.q, 16); std::memcpy(C.t, k.Tcw.t, 12); std::memcpy(C.Ow, k.Ow, 12);
    C.fx = k.fx; C.fy = k.fy; C.cx = k.cx; C.cy = k.cy;
    C.min_x = k.min_x; C.max_x = k.max_x; C.min_y = k.min_y; C.max_y = k.max_y;
    C.log_scale_factor = k.log_scale_factor; C.n_levels = k.n_levels; C.sim3_pair = 0;
  }
  if (up > h->tgt_bytes || go > h->tgt_bytes + h->grid_bytes) return fail(fn, DVM_ERR_STATE, "packed targets exceed the reserved regions");   // (an internal error: the constants bound every target)
  DVM_HIP(hipMemcpyAsync(h->d, h->hp, up, hipMemcpyHostToDevice, h->s));
  const bool prof = h->profiling != 0;
  if (prof) DVM_HIP(hipEventRecord(h->ev[0], h->s));
  launch_ft_build(h->s, reinterpret_cast<const FtTargetDev*>(h->d), n_targets);
  if (prof) DVM_HIP(hipEventRecord(h->ev[1], h->s));
  h->build_timed = prof;
  return hip_check(hipGetLastError(), "dvm_fuse_targets_set launch");
}

int dvm_fuse_targets_run(dvm_fuse_targets* h, const dvm_ft_points* P, const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist) {
  const char* fn = "dvm_fuse_targets_run";
  if (!h || !P) return fail(fn, DVM_ERR_INVALID, "missing argument");
  if (h->n_targets < 0) return fail(fn, DVM_ERR_INVALID, "no targets (dvm_fuse_targets_set comes first)");
  if (P->n < 0) return fail(fn, DVM_ERR_INVALID, "negative point count");
  if (P->n > h->max_points) return fail(fn, DVM_ERR_CAPACITY, "beyond the reservation (dvm_fuse_targets_reserve): " + std::to_string(P->n) + " points");
  const int T = h->n_targets, n = P->n;
  if (T == 0 || n == 0) return DVM_OK;
  if (!P->pos || !P->normal || !P->min_dist || !P->max_dist || !P->desc || !best_idx) return fail(fn, DVM_ERR_INVALID, "missing array");
  DVM_HIP(hipSetDevice(h->device));
  const size_t N = (size_t)n, E = N * (size_t)T;
  uint8_t* stage = h->hp + h->tgt_bytes;
  uint8_t* dev = h->d + h->tgt_bytes + h->grid_bytes;
  size_t off = 0;
  auto put = [&](const void* src, size_t bytes) {
    const size_t o = off;
    std::memcpy(stage + o, src, bytes);
    off = o + al(bytes);
    return dev + o;
  };
  FtPoints A{};
  A.pos = reinterpret_cast<const float*>(put(P->pos, N * 12));
  A.normal = reinterpret_cast<const float*>(put(P->normal, N * 12));
  A.min_dist = reinterpret_cast<const float*>(put(P->min_dist, N * 4));
  A.max_dist = reinterpret_cast<const float*>(put(P->max_dist, N * 4));
  A.desc = put(P->desc, N * 32);
  A.valid = P->valid ? put(P->valid, N) : nullptr;
  A.skip = skip ? put(skip, E) : nullptr;
  A.n = n;
  if (off > h->pts_bytes) return fail(fn, DVM_ERR_STATE, "packed points exceed the reserved region");   // (an internal error)
  int32_t* d_idx = reinterpret_cast<int32_t*>(dev + h->pts_bytes);
  int32_t* d_dist = reinterpret_cast<int32_t*>(dev + h->pts_bytes + al(E * 4));
  uint8_t* h_res = stage + h->pts_bytes;
  const size_t back = best_dist ? al(E * 4) + E * 4 : E * 4;

  DVM_HIP(hipMemcpyAsync(dev, stage, off, hipMemcpyHostToDevice, h->s));
  const bool prof = h->profiling != 0;
  if (prof) DVM_HIP(hipEventRecord(h->ev[2], h->s));
  launch_ft_search(h->s, reinterpret_cast<const FtTargetDev*>(h->d), T, A, th, d_idx, d_dist);
  if (prof) DVM_HIP(hipEventRecord(h->ev[3], h->s));
  int rc = hip_check(hipGetLastError(), "dvm_fuse_targets_run launch");
  if (rc == DVM_OK) rc = hip_check(hipMemcpyAsync(h_res, d_idx, back, hipMemcpyDeviceToHost, h->s), "dvm_fuse_targets_run copy");
  const int rs = hip_check(hipStreamSynchronize(h->s), "dvm_fuse_targets_run sync");
  if (rc != DVM_OK) return rc;
  if (rs != DVM_OK) return rs;
  if (prof) {
    if (h->build_timed) { DVM_HIP(hipEventElapsedTime(&h->last_ms[0], h->ev[0], h->ev[1])); h->build_timed = 0; }
    DVM_HIP(hipEventElapsedTime(&h->last_ms[1], h->ev[2], h->ev[3]));
  }
  std::memcpy(best_idx, h_res, E * 4);
  if (best_dist) std::memcpy(best_dist, h_res + al(E * 4), E * 4);
  return DVM_OK;
}

}  // extern "C"
