// dvm_slam_amd/csrc/fuse_targets.cpp -- dvm_fuse_targets: the Fuse searches of LocalMapping::SearchInNeighbors against all target keyframes
// as one chain (include/dvmslam_hip.h; kernels in fuse_targets_kernels.hip; the handle's stream, working set, packing cursor and kernel
// times: chain.h).  The working set: a device block [target upload][grid spans][point table + mask][results] and a page-locked block
// [target staging][point staging][results].
// set: validates, packs every target back to back into the staging region, sends it with ONE copy and builds all grids with ONE launch; it
// does not wait.  run: packs the point table and the mask, ONE copy, ONE launch over (target, point) per camera model present, ONE copy
// back, ONE synchronisation.  run_hits: the same search, then the compaction of the dense rows on the device (three launches) straight
// into a mapped page-locked block [hit_off][hits] of its own (reserve_hits), and ONE synchronisation: nothing of size T x n comes back.
// set_resident: the targets are slots of a dvm_keyframe_store (keyframe_store.h): the table's pointers go into the store, the table and
// the model order list are the whole upload, and no grid is built; a run brackets its search with kfs_read_begin / kfs_read_end.
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dvmslam_hip.h"
#include "camera_model.h"
#include "chain.h"
#include "fuse_targets_kernels.h"
#include "keyframe_store.h"
#include "orb_pipeline.h"

using namespace dvm;

struct dvm_fuse_targets : Chain {
  // ws.d: [tgt_bytes][grid_bytes][pts_bytes][res_bytes]; ws.hm (page-locked, not mapped): [tgt_bytes][pts_bytes][res_bytes]
  size_t tgt_bytes = 0, grid_bytes = 0, pts_bytes = 0, res_bytes = 0;
  int max_points = 0, max_targets = 0, max_total = 0;
  int n_targets = -1;                           // of the last set; -1: none yet
  int n_pinhole = 0, n_kb8 = 0;                 // of the last set: its targets by camera model ...
  const int32_t* order = nullptr;               // ... and their indices in that order (device, inside the target upload)
  // the mapped block of run_hits: [hit_off: hit_targets + 1 entries, rounded up to 64 bytes][hits: max_hits]; max_hits = -1: none yet
  uint8_t *hit_hm = nullptr, *hit_dev = nullptr;
  int max_hits = -1, hit_targets = 0;
  int build_timed = 0;                          // marks 0 / 1 hold a set's grid build that no run has read yet
  float last_ms[2] = {0, 0};
  // a resident set: the store its targets live in and every named slot's generation at the set; null: the targets were uploaded
  const dvm_keyframe_store* store = nullptr;
  std::vector<std::pair<int32_t, uint32_t>> slot_gen;
  int64_t set_bytes = 0, run_bytes = 0;         // host-to-device bytes queued by the last set / run
};

namespace {
using Cursor64 = Cursor<64>;                    // every item of the uploads, the grid spans and the results starts at a multiple of 64 bytes
constexpr int kMaxTargets = 65535;              // gridDim.y
constexpr int64_t kMaxEntries = (int64_t)1 << 27;   // target x point entries of one run
// upload bytes of a target of n keypoints at most: keypoints, descriptors; two level tables of 64 and the rounding of its four arrays
constexpr size_t kUpPerKeypoint = sizeof(dvm_keypoint_pod) + 32, kUpFixed = 2 * 64 * 4 + 4 * 64;
// grid bytes: sorted keypoint, index, descriptor; cell_start[kCellStartStride], the three counters and the rounding of its five arrays
constexpr size_t kGridPerKeypoint = sizeof(float4) + 4 + 32, kGridFixed = (size_t)kCellStartStride * 4 + 5 * 64;
constexpr size_t kPointBytes = 12 + 12 + 4 + 4 + 32 + 1;

int fail(const char* fn, int rc, const std::string& msg) { set_error(std::string(fn) + ": " + msg); return rc; }

void free_hits(dvm_fuse_targets* h) {
  if (h->hit_hm) hipHostFree(h->hit_hm);
  h->hit_hm = h->hit_dev = nullptr; h->max_hits = -1; h->hit_targets = 0;
}
// replaces the mapped block by one for max_hits hits of n_targets targets; on failure the handle holds none
int alloc_hits(dvm_fuse_targets* h, const char* fn, int max_hits, int n_targets) {
  free_hits(h);
  const size_t bytes = pad<64>(((size_t)n_targets + 1) * 4) + pad<64>((size_t)max_hits * sizeof(FtHit));
  if (hipHostMalloc(reinterpret_cast<void**>(&h->hit_hm), bytes, hipHostMallocMapped) != hipSuccess) {
    h->hit_hm = nullptr;
    return fail(fn, DVM_ERR_HIP, "mapped host memory failed");
  }
  if (hipHostGetDevicePointer(reinterpret_cast<void**>(&h->hit_dev), h->hit_hm, 0) != hipSuccess) {
    free_hits(h);
    return fail(fn, DVM_ERR_HIP, "mapped host memory failed");
  }
  h->max_hits = max_hits; h->hit_targets = n_targets;
  return DVM_OK;
}
}  // namespace

extern "C" {

int dvm_fuse_targets_create(int device, dvm_fuse_targets** out) { return chain_create(device, out); }
void dvm_fuse_targets_destroy(dvm_fuse_targets* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->s) hipStreamSynchronize(h->s);          // (the kernels of a run_hits write the mapped block)
  free_hits(h);
  chain_destroy(h);
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
  // (the targets of an earlier set go with the block: set again; a failed allocation leaves the handle holding nothing)
  h->tgt_bytes = h->grid_bytes = h->pts_bytes = h->res_bytes = 0; h->max_points = h->max_targets = h->max_total = 0; h->n_targets = -1;
  h->store = nullptr; h->slot_gen.clear();
  const size_t tgt = pad<64>(pad<64>((size_t)nt * sizeof(FtTargetDev)) + pad<64>((size_t)nt * 4) + (size_t)tot * kUpPerKeypoint + (size_t)nt * kUpFixed);
  const size_t grid = pad<64>((size_t)tot * kGridPerKeypoint + (size_t)nt * kGridFixed + 64);
  const size_t pts = pad<64>((size_t)np * kPointBytes + 7 * 64 + pad<64>((size_t)np * nt));
  const size_t res = 2 * pad<64>((size_t)np * nt * 4) + 2 * pad<64>(((size_t)nt + 1) * 4);   // best_idx, best_dist; run_hits' counts and offsets
  if (const char* what = h->ws.alloc(tgt + grid + pts + res, tgt + pts + res, tgt, /*mapped*/ false, /*zeroed*/ false))
    return fail("dvm_fuse_targets_reserve", DVM_ERR_HIP, std::string(what) + " failed");
  h->tgt_bytes = tgt; h->grid_bytes = grid; h->pts_bytes = pts; h->res_bytes = res;
  h->max_points = np; h->max_targets = nt; h->max_total = tot;
  if (h->max_hits >= 0 && nt > h->hit_targets) return alloc_hits(h, "dvm_fuse_targets_reserve", h->max_hits, nt);   // hit_off follows the targets
  return DVM_OK;
}

int dvm_fuse_targets_reserve_hits(dvm_fuse_targets* h, int max_hits) {
  const char* fn = "dvm_fuse_targets_reserve_hits";
  if (!h || max_hits < 0 || (int64_t)max_hits > kMaxEntries) return fail(fn, DVM_ERR_INVALID, "bad size");
  if (max_hits <= h->max_hits) return DVM_OK;
  DVM_HIP(hipSetDevice(h->device));
  DVM_HIP(hipStreamSynchronize(h->s));
  return alloc_hits(h, fn, max_hits, h->max_targets);
}

int dvm_fuse_targets_profiling(dvm_fuse_targets* h, int enable) {
  if (!h) return DVM_ERR_INVALID;
  DVM_HIP(hipSetDevice(h->device));
  return h->timer.enable(enable != 0);
}
int dvm_fuse_targets_last_kernel_ms(dvm_fuse_targets* h, float* ms) {
  if (!h || !ms) return DVM_ERR_INVALID;
  ms[0] = h->last_ms[0]; ms[1] = h->last_ms[1];
  return DVM_OK;
}
int dvm_fuse_targets_last_upload_bytes(const dvm_fuse_targets* h, int64_t* set_bytes, int64_t* run_bytes) {
  if (!h) return DVM_ERR_INVALID;
  if (set_bytes) *set_bytes = h->set_bytes;
  if (run_bytes) *run_bytes = h->run_bytes;
  return DVM_OK;
}

}  // extern "C"

// dvm_fuse_targets_set (models = forms = nullptr) and dvm_fuse_targets_set_cam
static int set_targets(const char* fn, dvm_fuse_targets* h, int n_targets, const dvm_ft_target* targets, const dvm_camera_model* models,
                       const uint8_t* forms) {
  static_assert(sizeof(dvm_keypoint) == sizeof(dvm_keypoint_pod), "layout");
  static_assert(sizeof(dvm_ft_hit) == sizeof(FtHit), "layout");
  if (!h || n_targets < 0 || (n_targets > 0 && !targets)) return fail(fn, DVM_ERR_INVALID, "missing argument");
  int64_t total = 0;
  int n_kb8 = 0;
  for (int t = 0; t < n_targets; t++) {
    const dvm_ft_target& k = targets[t];
    const std::string w = "target " + std::to_string(t);
    const bool scw = forms && forms[t] == DVM_FT_FORM_SCW;
    if (forms && forms[t] != DVM_FT_FORM_POINTS && forms[t] != DVM_FT_FORM_SCW) return fail(fn, DVM_ERR_INVALID, w + ": form outside {0, 1}");
    if (models && models[t].model != dvm_cam::kPinhole && models[t].model != dvm_cam::kKannalaBrandt8)
      return fail(fn, DVM_ERR_INVALID, w + ": camera model outside {0, 1}");
    if (models && !dvm_cam::model_ok(models[t].model, models[t].p)) return fail(fn, DVM_ERR_INVALID, w + ": zero focal length of the camera model");
    if (k.n < 0 || k.n > kFrameCap) return fail(fn, DVM_ERR_INVALID, w + ": n outside [0, 8192]");
    if (k.n_levels < 1 || k.n_levels > 64) return fail(fn, DVM_ERR_INVALID, w + ": n_levels outside [1, 64]");
    if (!k.scale_factors || (!scw && !k.inv_level_sigma2)) return fail(fn, DVM_ERR_INVALID, w + ": missing level table");
    if (!models && (!(k.fx != 0.0f) || !(k.fy != 0.0f))) return fail(fn, DVM_ERR_INVALID, w + ": zero focal length");
    n_kb8 += models && models[t].model == dvm_cam::kKannalaBrandt8 ? 1 : 0;
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
  h->store = nullptr; h->slot_gen.clear(); h->set_bytes = 0;
  if (n_targets == 0) return DVM_OK;
  DVM_HIP(hipSetDevice(h->device));
  DVM_HIP(hipStreamSynchronize(h->s));           // the staging region may still feed the copy of an earlier set (idle after a run: free)

  const WorkingSet& ws = h->ws;
  Cursor64 up{ws.hm, ws.d};                                      // the upload region: staging -> device
  Cursor64 grid{ws.d + h->tgt_bytes};                            // the grid spans behind it, device only
  FtTargetDev* tab = up.carve<FtTargetDev>((size_t)n_targets);
  int32_t* order = up.carve<int32_t>((size_t)n_targets);         // the pinhole targets' indices, then the KannalaBrandt8 targets'
  h->order = rebase(order, ws.hm, ws.d);
  h->n_kb8 = n_kb8; h->n_pinhole = n_targets - n_kb8;
  int32_t* n_overflow = grid.carve<int32_t>(1);                  // (never counted: every span holds its target exactly)
  for (int t = 0, at0 = 0, at1 = h->n_pinhole; t < n_targets; t++) {
    const dvm_ft_target& k = targets[t];
    FtTargetDev& D = tab[t];
    std::memset(&D, 0, sizeof(D));
    const bool kb8 = models && models[t].model == dvm_cam::kKannalaBrandt8;
    order[kb8 ? at1++ : at0++] = t;
    D.model = kb8 ? dvm_cam::kKannalaBrandt8 : dvm_cam::kPinhole;
    if (kb8) std::memcpy(D.kb8, models[t].p, sizeof(D.kb8));
    const size_t n = (size_t)k.n;
    D.kps = reinterpret_cast<const dvm_keypoint_pod*>(up.put(k.kps, n * sizeof(dvm_keypoint_pod)));
    D.desc = up.put(k.desc, n * 32);
    D.sf = reinterpret_cast<const float*>(up.put(k.scale_factors, (size_t)k.n_levels * 4));
    if (!(forms && forms[t] == DVM_FT_FORM_SCW))                  // (null: project_row skips the gate)
      D.inv_sigma2 = reinterpret_cast<const float*>(up.put(k.inv_level_sigma2, (size_t)k.n_levels * 4));
    D.n = k.n;
    FrameView& F = D.F;
    F.skp = grid.carve<float4>(n);
    F.sidx = grid.carve<int32_t>(n);
    F.sdesc = grid.carve<uint8_t>(n * 32);
    F.cell_start = grid.carve<int32_t>(kCellStartStride);
    F.n_sorted = grid.carve<int32_t>(2);
    F.n_total = F.n_sorted + 1;
    F.n_overflow = n_overflow;
    F.cap = k.n;
    F.minX = k.min_x; F.minY = k.min_y;
    F.wInv = static_cast<float>(64) / static_cast<float>(k.max_x - k.min_x);   // Frame.cc:443-444, as dvm_frame_build
    F.hInv = static_cast<float>(48) / static_cast<float>(k.max_y - k.min_y);
    ProjectCam& C = D.C;
    std::memcpy(C.q, k.Tcw.q, 16); std::memcpy(C.t, k.Tcw.t, 12); std::memcpy(C.Ow, k.Ow, 12);
    if (models) { C.fx = models[t].p[0]; C.fy = models[t].p[1]; C.cx = models[t].p[2]; C.cy = models[t].p[3]; }   // (a given model replaces the target's own)
    else { C.fx = k.fx; C.fy = k.fy; C.cx = k.cx; C.cy = k.cy; }
    C.min_x = k.min_x; C.max_x = k.max_x; C.min_y = k.min_y; C.max_y = k.max_y;
    C.log_scale_factor = k.log_scale_factor; C.n_levels = k.n_levels; C.sim3_pair = 0;
  }
  if (up.used() > h->tgt_bytes || grid.used() > h->grid_bytes) return fail(fn, DVM_ERR_STATE, "packed targets exceed the reserved regions");   // (an internal error: the constants bound every target)
  DVM_HIP(hipMemcpyAsync(ws.d, ws.hm, up.used(), hipMemcpyHostToDevice, h->s));
  h->set_bytes = (int64_t)up.used();
  DVM_HIP(h->timer.mark(0, h->s));
  launch_ft_build(h->s, reinterpret_cast<const FtTargetDev*>(ws.d), n_targets);
  DVM_HIP(h->timer.mark(1, h->s));
  h->build_timed = h->timer.on;
  return hip_check(hipGetLastError(), "dvm_fuse_targets_set launch");
}

// dvm_fuse_targets_set_resident: set_targets with every target's arrays and grid in a store slot
static int set_resident(const char* fn, dvm_fuse_targets* h, const dvm_keyframe_store* st, int n_targets, const dvm_ft_target_resident* targets,
                        const dvm_camera_model* models, const uint8_t* forms) {
  if (!h || !st || n_targets < 0 || (n_targets > 0 && !targets)) return fail(fn, DVM_ERR_INVALID, "missing argument");
  if (kfs_device(st) != h->device) return fail(fn, DVM_ERR_INVALID, "the store lives on another device than the handle");
  std::vector<KfSlotView> views((size_t)n_targets);
  int n_kb8 = 0;
  for (int t = 0; t < n_targets; t++) {
    const std::string w = "target " + std::to_string(t);
    if (forms && forms[t] != DVM_FT_FORM_POINTS && forms[t] != DVM_FT_FORM_SCW) return fail(fn, DVM_ERR_INVALID, w + ": form outside {0, 1}");
    if (models && models[t].model != dvm_cam::kPinhole && models[t].model != dvm_cam::kKannalaBrandt8)
      return fail(fn, DVM_ERR_INVALID, w + ": camera model outside {0, 1}");
    if (models && !dvm_cam::model_ok(models[t].model, models[t].p)) return fail(fn, DVM_ERR_INVALID, w + ": zero focal length of the camera model");
    if (!kfs_slot_view(st, targets[t].slot, &views[t]))
      return fail(fn, DVM_ERR_INVALID, w + ": slot " + std::to_string(targets[t].slot) + " outside the store, never written or removed");
    if (!models && (!(views[t].fx != 0.0f) || !(views[t].fy != 0.0f))) return fail(fn, DVM_ERR_INVALID, w + ": zero focal length");
    n_kb8 += models && models[t].model == dvm_cam::kKannalaBrandt8 ? 1 : 0;
  }
  if (n_targets > h->max_targets)
    return fail(fn, DVM_ERR_CAPACITY, "beyond the reservation (dvm_fuse_targets_reserve): " + std::to_string(n_targets) + " targets");
  h->n_targets = n_targets;
  h->store = nullptr; h->slot_gen.clear(); h->set_bytes = 0;
  if (n_targets == 0) return DVM_OK;
  DVM_HIP(hipSetDevice(h->device));
  DVM_HIP(hipStreamSynchronize(h->s));           // the staging region may still feed the copy of an earlier set (idle after a run: free)

  const WorkingSet& ws = h->ws;
  Cursor64 up{ws.hm, ws.d};
  FtTargetDev* tab = up.carve<FtTargetDev>((size_t)n_targets);
  int32_t* order = up.carve<int32_t>((size_t)n_targets);         // the pinhole targets' indices, then the KannalaBrandt8 targets'
  h->order = rebase(order, ws.hm, ws.d);
  h->n_kb8 = n_kb8; h->n_pinhole = n_targets - n_kb8;
  for (int t = 0, at0 = 0, at1 = h->n_pinhole; t < n_targets; t++) {
    const dvm_ft_target_resident& k = targets[t];
    const KfSlotView& V = views[t];
    FtTargetDev& D = tab[t];
    std::memset(&D, 0, sizeof(D));
    const bool kb8 = models && models[t].model == dvm_cam::kKannalaBrandt8;
    order[kb8 ? at1++ : at0++] = t;
    D.model = kb8 ? dvm_cam::kKannalaBrandt8 : dvm_cam::kPinhole;
    if (kb8) std::memcpy(D.kb8, models[t].p, sizeof(D.kb8));
    D.kps = V.kps; D.desc = V.desc; D.sf = V.sf;
    D.inv_sigma2 = forms && forms[t] == DVM_FT_FORM_SCW ? nullptr : V.inv_sigma2;   // (null: project_row skips the gate)
    D.n = V.n;
    D.F = V.F;
    ProjectCam& C = D.C;
    std::memcpy(C.q, k.Tcw.q, 16); std::memcpy(C.t, k.Tcw.t, 12); std::memcpy(C.Ow, k.Ow, 12);
    if (models) { C.fx = models[t].p[0]; C.fy = models[t].p[1]; C.cx = models[t].p[2]; C.cy = models[t].p[3]; }   // (a given model replaces the slot's own)
    else { C.fx = V.fx; C.fy = V.fy; C.cx = V.cx; C.cy = V.cy; }
    C.min_x = V.min_x; C.max_x = V.max_x; C.min_y = V.min_y; C.max_y = V.max_y;
    C.log_scale_factor = V.log_scale_factor; C.n_levels = V.n_levels; C.sim3_pair = 0;
    h->slot_gen.emplace_back(k.slot, V.gen);
  }
  if (up.used() > h->tgt_bytes) return fail(fn, DVM_ERR_STATE, "the target table exceeds the reserved region");   // (an internal error)
  DVM_HIP(hipMemcpyAsync(ws.d, ws.hm, up.used(), hipMemcpyHostToDevice, h->s));
  h->set_bytes = (int64_t)up.used();
  h->store = st;
  h->build_timed = 0; h->last_ms[0] = 0;         // (no grid was built)
  return DVM_OK;
}

// what a run returns: the dense rows (dvm_fuse_targets_run: best_idx, best_dist) or the hits (dvm_fuse_targets_run_hits: the rest)
struct FtResult {
  int32_t *best_idx = nullptr, *best_dist = nullptr;
  bool want_hits = false;
  int32_t* hit_off = nullptr;
  dvm_ft_hit* hits = nullptr;
  int hit_cap = 0;
  int32_t* n_hits = nullptr;
};
static int run_points(const char* fn, dvm_fuse_targets* h, const dvm_ft_points* P, const uint8_t* skip, float th, const FtResult& out) {
  if (!h || !P) return fail(fn, DVM_ERR_INVALID, "missing argument");
  if (h->n_targets < 0) return fail(fn, DVM_ERR_INVALID, "no targets (dvm_fuse_targets_set comes first)");
  if (h->store)                                 // a resident set: its slots still hold the keyframes it was made on
    for (const auto& sg : h->slot_gen)
      if (kfs_generation(h->store, sg.first) != sg.second) return fail(fn, DVM_ERR_STATE, "a target's slot was written since the set");
  if (P->n < 0) return fail(fn, DVM_ERR_INVALID, "negative point count");
  if (P->n > h->max_points) return fail(fn, DVM_ERR_CAPACITY, "beyond the reservation (dvm_fuse_targets_reserve): " + std::to_string(P->n) + " points");
  const int T = h->n_targets, n = P->n;
  if (out.want_hits) {
    if (h->max_hits < 0) return fail(fn, DVM_ERR_INVALID, "no hit block (dvm_fuse_targets_reserve_hits comes first)");
    if (!out.hit_off || out.hit_cap < 0 || (out.hit_cap > 0 && !out.hits)) return fail(fn, DVM_ERR_INVALID, "missing array");
  }
  if (T == 0 || n == 0) {
    if (out.want_hits) {
      std::memset(out.hit_off, 0, ((size_t)T + 1) * 4);
      if (out.n_hits) *out.n_hits = 0;
    }
    return DVM_OK;
  }
  if (!P->pos || !P->normal || !P->min_dist || !P->max_dist || !P->desc || (!out.want_hits && !out.best_idx)) return fail(fn, DVM_ERR_INVALID, "missing array");
  if (out.want_hits && T > h->hit_targets) return fail(fn, DVM_ERR_STATE, "the hit block holds fewer targets than the set");   // (an internal error: reserve keeps it in step)
  DVM_HIP(hipSetDevice(h->device));
  const size_t N = (size_t)n, E = N * (size_t)T;
  const WorkingSet& ws = h->ws;
  uint8_t* stage = ws.hm + h->tgt_bytes;
  uint8_t* dev = ws.d + h->tgt_bytes + h->grid_bytes;
  Cursor64 up{stage, dev};
  FtPoints A{};
  A.pos = reinterpret_cast<const float*>(up.put(P->pos, N * 12));
  A.normal = reinterpret_cast<const float*>(up.put(P->normal, N * 12));
  A.min_dist = reinterpret_cast<const float*>(up.put(P->min_dist, N * 4));
  A.max_dist = reinterpret_cast<const float*>(up.put(P->max_dist, N * 4));
  A.desc = up.put(P->desc, N * 32);
  A.valid = P->valid ? up.put(P->valid, N) : nullptr;
  A.skip = skip ? up.put(skip, E) : nullptr;
  A.n = n;
  if (up.used() > h->pts_bytes) return fail(fn, DVM_ERR_STATE, "packed points exceed the reserved region");   // (an internal error)
  int32_t* d_idx = reinterpret_cast<int32_t*>(dev + h->pts_bytes);
  int32_t* d_dist = reinterpret_cast<int32_t*>(dev + h->pts_bytes + pad<64>(E * 4));
  int32_t* d_cnt = reinterpret_cast<int32_t*>(dev + h->pts_bytes + 2 * pad<64>(E * 4));
  int32_t* d_off = reinterpret_cast<int32_t*>(dev + h->pts_bytes + 2 * pad<64>(E * 4) + pad<64>(((size_t)T + 1) * 4));
  uint8_t* h_res = stage + h->pts_bytes;
  const size_t back = out.best_dist ? pad<64>(E * 4) + E * 4 : E * 4;
  // the mapped block of the hits: what the kernels write to, and where the host reads it after the synchronisation
  const size_t hit_at = pad<64>(((size_t)h->hit_targets + 1) * 4);
  const int cap = out.want_hits ? std::min(out.hit_cap, h->max_hits) : 0;

  DVM_HIP(hipMemcpyAsync(dev, stage, up.used(), hipMemcpyHostToDevice, h->s));
  h->run_bytes = (int64_t)up.used();
  if (h->store) { const int rb = kfs_read_begin(h->store, h->s); if (rb != DVM_OK) return rb; }
  const EventTimer& tm = h->timer;
  DVM_HIP(tm.mark(2, h->s));
  launch_ft_search(h->s, reinterpret_cast<const FtTargetDev*>(ws.d), h->order, h->n_pinhole, h->n_kb8, A, th, d_idx, d_dist);
  DVM_HIP(tm.mark(3, h->s));
  if (h->store) { const int re = kfs_read_end(h->store, h->s); if (re != DVM_OK) return re; }
  if (out.want_hits)
    launch_ft_hits(h->s, d_idx, d_dist, T, n, d_cnt, d_off, reinterpret_cast<int32_t*>(h->hit_dev), reinterpret_cast<FtHit*>(h->hit_dev + hit_at), cap);
  int rc = hip_check(hipGetLastError(), "dvm_fuse_targets_run launch");
  if (rc == DVM_OK && !out.want_hits) rc = hip_check(hipMemcpyAsync(h_res, d_idx, back, hipMemcpyDeviceToHost, h->s), "dvm_fuse_targets_run copy");
  const int rs = hip_check(hipStreamSynchronize(h->s), "dvm_fuse_targets_run sync");
  if (rc != DVM_OK) return rc;
  if (rs != DVM_OK) return rs;
  if (tm.on) {
    if (h->build_timed) { DVM_HIP(tm.elapsed(0, 1, &h->last_ms[0])); h->build_timed = 0; }
    DVM_HIP(tm.elapsed(2, 3, &h->last_ms[1]));
  }
  if (out.want_hits) {
    const int32_t* off = reinterpret_cast<const int32_t*>(h->hit_hm);
    const int total = off[T];
    std::memcpy(out.hit_off, off, ((size_t)T + 1) * 4);
    if (out.n_hits) *out.n_hits = total;
    if (total > cap)
      return fail(fn, DVM_ERR_CAPACITY, std::to_string(total) + " hits beyond hit_cap or the reservation (dvm_fuse_targets_reserve_hits): " + std::to_string(cap));
    if (total > 0) std::memcpy(out.hits, h->hit_hm + hit_at, (size_t)total * sizeof(dvm_ft_hit));
    return DVM_OK;
  }
  std::memcpy(out.best_idx, h_res, E * 4);
  if (out.best_dist) std::memcpy(out.best_dist, h_res + pad<64>(E * 4), E * 4);
  return DVM_OK;
}

extern "C" {

int dvm_fuse_targets_set(dvm_fuse_targets* h, int n_targets, const dvm_ft_target* targets) {
  return set_targets("dvm_fuse_targets_set", h, n_targets, targets, nullptr, nullptr);
}
int dvm_fuse_targets_set_cam(dvm_fuse_targets* h, int n_targets, const dvm_ft_target* targets, const dvm_camera_model* models, const uint8_t* forms) {
  return set_targets("dvm_fuse_targets_set_cam", h, n_targets, targets, models, forms);
}
int dvm_fuse_targets_set_resident(dvm_fuse_targets* h, const dvm_keyframe_store* store, int n_targets, const dvm_ft_target_resident* targets,
                                  const dvm_camera_model* models, const uint8_t* forms) {
  return set_resident("dvm_fuse_targets_set_resident", h, store, n_targets, targets, models, forms);
}
int dvm_fuse_targets_run(dvm_fuse_targets* h, const dvm_ft_points* P, const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist) {
  FtResult out;
  out.best_idx = best_idx; out.best_dist = best_dist;
  return run_points("dvm_fuse_targets_run", h, P, skip, th, out);
}
int dvm_fuse_targets_run_hits(dvm_fuse_targets* h, const dvm_ft_points* P, const uint8_t* skip, float th, int32_t* hit_off, dvm_ft_hit* hits,
                              int hit_cap, int32_t* n_hits) {
  FtResult out;
  out.want_hits = true; out.hit_off = hit_off; out.hits = hits; out.hit_cap = hit_cap; out.n_hits = n_hits;
  return run_points("dvm_fuse_targets_run_hits", h, P, skip, th, out);
}

}  // extern "C"
