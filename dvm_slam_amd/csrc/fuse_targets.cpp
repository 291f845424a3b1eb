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
// run[_hits]_resident: the points are slots of a dvm_map_store (map_store.h): the slots (and the masks) are the whole upload, ONE launch
// (k_ft_gather, fuse_points_kernels.hip) fills the point table from the records, and the run goes on as above, bracketed by
// store_read_begin / store_read_end.  run_hits_candidates: the flat slot lists of the target keyframes go up, the device makes the
// candidate list of SearchInNeighbors' second direction (k_ft_cand_*), gathers and searches it; list and hits come down through mapped
// blocks.  Every slot list is checked on the host first (fuse_points_lists.h).
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dvmslam_hip.h"
#include "camera_model.h"
#include "chain.h"
#include "fuse_points_lists.h"
#include "fuse_targets_kernels.h"
#include "keyframe_store.h"
#include "map_store.h"
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
  // the blocks of run_hits_candidates (reserve_candidates); max_entries = -1: none yet.  cand_d (device): [first: map_capacity words, idle
  // kFtFirstIdle][mark: map_capacity bytes, idle 0][the upload: flat lists, exclude list][cand: max_entries][cnt: blocks][off: blocks + 1];
  // cand_hm (mapped): [the staging of the upload][off_out: blocks + 1][cand_out: max_entries]
  uint8_t *cand_d = nullptr, *cand_hm = nullptr, *cand_hm_dev = nullptr;
  int max_entries = -1, map_capacity = 0;
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
constexpr size_t kSlotBytes = 4 + 1;            // a resident run's slot and caller's valid flag, in front of the gathered table

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

// the two blocks of run_hits_candidates, walked by one layout each (a null base measures)
// (up: the upload region, the flat lists then the exclude list, packed by a cursor of its own at equal offsets of both blocks)
struct CandDev { int32_t* first; uint8_t* mark; int32_t *up, *cand, *cnt, *off; size_t bytes; };
struct CandHost { int32_t *up, *off_out, *cand_out; size_t bytes; };
size_t cand_blocks(int entries) { return ((size_t)entries + 255) / 256; }
CandDev cand_dev_layout(uint8_t* base, int max_entries, int map_capacity) {
  Cursor64 c{base};
  CandDev L{};
  const size_t me = (size_t)max_entries, nb = cand_blocks(max_entries);
  L.first = c.carve<int32_t>((size_t)map_capacity); L.mark = c.carve<uint8_t>((size_t)map_capacity);
  L.up = c.carve<int32_t>(2 * me + 32);
  L.cand = c.carve<int32_t>(me); L.cnt = c.carve<int32_t>(nb); L.off = c.carve<int32_t>(nb + 1);
  L.bytes = c.used();
  return L;
}
CandHost cand_host_layout(uint8_t* base, int max_entries) {
  Cursor64 c{base};
  CandHost L{};
  const size_t me = (size_t)max_entries;
  L.up = c.carve<int32_t>(2 * me + 32);
  L.off_out = c.carve<int32_t>(cand_blocks(max_entries) + 1); L.cand_out = c.carve<int32_t>(me);
  L.bytes = c.used();
  return L;
}
void free_candidates(dvm_fuse_targets* h) {
  if (h->cand_d) hipFree(h->cand_d);
  if (h->cand_hm) hipHostFree(h->cand_hm);
  h->cand_d = h->cand_hm = h->cand_hm_dev = nullptr; h->max_entries = -1; h->map_capacity = 0;
}
}  // namespace

extern "C" {

int dvm_fuse_targets_create(int device, dvm_fuse_targets** out) { return chain_create(device, out); }
void dvm_fuse_targets_destroy(dvm_fuse_targets* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->s) hipStreamSynchronize(h->s);          // (the kernels of a run_hits write the mapped block)
  free_hits(h);
  free_candidates(h);
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
  const size_t pts = pad<64>((size_t)np * (kPointBytes + kSlotBytes) + 9 * 64 + pad<64>((size_t)np * nt));
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

int dvm_fuse_targets_reserve_candidates(dvm_fuse_targets* h, int max_entries, int map_capacity) {
  const char* fn = "dvm_fuse_targets_reserve_candidates";
  if (!h || max_entries < 0 || (int64_t)max_entries > kMaxEntries || map_capacity < 0) return fail(fn, DVM_ERR_INVALID, "bad size");
  if (max_entries <= h->max_entries && map_capacity <= h->map_capacity) return DVM_OK;
  DVM_HIP(hipSetDevice(h->device));
  DVM_HIP(hipStreamSynchronize(h->s));
  const int me = std::max(max_entries, h->max_entries), mc = std::max(map_capacity, h->map_capacity);
  free_candidates(h);                             // (a failed allocation leaves the handle holding none)
  const CandDev D = cand_dev_layout(nullptr, me, mc);
  const CandHost H = cand_host_layout(nullptr, me);
  const char* what = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&h->cand_d), D.bytes) != hipSuccess) { h->cand_d = nullptr; what = "hipMalloc"; }
  else if (hipHostMalloc(reinterpret_cast<void**>(&h->cand_hm), H.bytes, hipHostMallocMapped) != hipSuccess) { h->cand_hm = nullptr; what = "mapped host memory"; }
  else if (hipHostGetDevicePointer(reinterpret_cast<void**>(&h->cand_hm_dev), h->cand_hm, 0) != hipSuccess) what = "mapped host memory";
  if (what) {
    (void)hipGetLastError();
    free_candidates(h);
    return fail(fn, DVM_ERR_HIP, std::string(what) + " failed");
  }
  // both tables idle, once: every call puts back what it touched
  const CandDev L = cand_dev_layout(h->cand_d, me, mc);
  int rc = DVM_OK;
  if (mc > 0) rc = hip_check(hipMemsetAsync(L.first, 0x7f, (size_t)mc * 4, h->s), "dvm_fuse_targets_reserve_candidates memset");
  if (mc > 0 && rc == DVM_OK) rc = hip_check(hipMemsetAsync(L.mark, 0, (size_t)mc, h->s), "dvm_fuse_targets_reserve_candidates memset");
  if (rc == DVM_OK) rc = hip_check(hipStreamSynchronize(h->s), "dvm_fuse_targets_reserve_candidates sync");
  if (rc != DVM_OK) { free_candidates(h); return rc; }
  h->max_entries = me; h->map_capacity = mc;
  return DVM_OK;
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

// where a run's point table comes from -- exactly one is set: the caller's arrays (dvm_fuse_targets_run[_hits]), the records of a map
// store under the caller's slots (_resident), or under the candidate list the device makes of the caller's lists (_candidates)
struct FtSource {
  const dvm_ft_points* table = nullptr;
  const dvm_ft_points_resident* slots = nullptr;
  const dvm_ft_candidates* cand = nullptr;
};
// what a run returns: the dense rows (dvm_fuse_targets_run: best_idx, best_dist) or the hits (dvm_fuse_targets_run_hits: the rest); a
// candidates run returns its list as well
struct FtResult {
  int32_t *best_idx = nullptr, *best_dist = nullptr;
  bool want_hits = false;
  int32_t* hit_off = nullptr;
  dvm_ft_hit* hits = nullptr;
  int hit_cap = 0;
  int32_t* n_hits = nullptr;
  int32_t* cand_slot = nullptr;
  int cand_cap = 0;
  int32_t* n_cand = nullptr;
};
static std::string fpl_message(const FplVerdict& v, int n_lists) {
  const std::string where = v.list < 0 ? std::string() : (v.list == n_lists && n_lists > 0 ? "the exclude list" : "list " + std::to_string(v.list)) +
                                                             (v.at >= 0 ? ", entry " + std::to_string(v.at) : std::string()) + ": ";
  switch (v.fault) {
    case kFplNull: return where + "missing array";
    case kFplCount: return where + "negative count";
    case kFplPoints: return "beyond the reservation (dvm_fuse_targets_reserve): more points than max_points";
    case kFplEntries: return "beyond the reservation (dvm_fuse_targets_reserve_candidates): more entries than max_entries";
    case kFplTable: return "beyond the reservation (dvm_fuse_targets_reserve_candidates): the store holds more slots than map_capacity";
    case kFplNoStore: return where + "a slot names a point and the store is NULL";
    default: return where + "a slot below -1, outside the store's capacity or never written";
  }
}
static int run_points(const char* fn, dvm_fuse_targets* h, const FtSource& src, const uint8_t* skip, float th, const FtResult& out) {
  const dvm_ft_points* P = src.table;
  if (!h || (!P && !src.slots && !src.cand)) return fail(fn, DVM_ERR_INVALID, "missing argument");
  if (h->n_targets < 0) return fail(fn, DVM_ERR_INVALID, "no targets (dvm_fuse_targets_set comes first)");
  if (h->store)                                 // a resident set: its slots still hold the keyframes it was made on
    for (const auto& sg : h->slot_gen)
      if (kfs_generation(h->store, sg.first) != sg.second) return fail(fn, DVM_ERR_STATE, "a target's slot was written since the set");
  // the source's own refusals; n: the rows of the search
  const dvm_map_store* st = P ? nullptr : src.slots ? src.slots->points : src.cand->points;
  int n = 0;
  if (P) {
    if (P->n < 0) return fail(fn, DVM_ERR_INVALID, "negative point count");
    if (P->n > h->max_points) return fail(fn, DVM_ERR_CAPACITY, "beyond the reservation (dvm_fuse_targets_reserve): " + std::to_string(P->n) + " points");
    n = P->n;
  } else {
    if (src.cand && h->max_entries < 0) return fail(fn, DVM_ERR_INVALID, "no candidate blocks (dvm_fuse_targets_reserve_candidates comes first)");
    if (st && store_device(st) != h->device) return fail(fn, DVM_ERR_INVALID, "the map store lives on another device than the handle");
    const FplStore fs{st ? dvm_map_store_capacity(st) : -1, st ? store_written(st) : nullptr};
    const FplVerdict v = src.slots ? fpl_check_points(*src.slots, fs, h->max_points) : fpl_check_candidates(*src.cand, fs, h->max_points, h->max_entries, h->map_capacity);
    if (v.fault != kFplOk) return fail(fn, v.rc(), fpl_message(v, src.cand ? src.cand->n_lists : 0));
    n = src.slots ? src.slots->n : (int)v.total;
  }
  const int T = h->n_targets;
  if (out.want_hits) {
    if (h->max_hits < 0) return fail(fn, DVM_ERR_INVALID, "no hit block (dvm_fuse_targets_reserve_hits comes first)");
    if (!out.hit_off || out.hit_cap < 0 || (out.hit_cap > 0 && !out.hits)) return fail(fn, DVM_ERR_INVALID, "missing array");
  }
  if (src.cand && (!out.n_cand || out.cand_cap < 0 || (out.cand_cap > 0 && !out.cand_slot))) return fail(fn, DVM_ERR_INVALID, "missing array");
  if (n == 0 || (T == 0 && !src.cand)) {          // (a candidates run without targets still makes its list)
    if (out.want_hits) {
      std::memset(out.hit_off, 0, ((size_t)T + 1) * 4);
      if (out.n_hits) *out.n_hits = 0;
    }
    if (src.cand) *out.n_cand = 0;
    return DVM_OK;
  }
  if (P && (!P->pos || !P->normal || !P->min_dist || !P->max_dist || !P->desc)) return fail(fn, DVM_ERR_INVALID, "missing array");
  if (!out.want_hits && !out.best_idx) return fail(fn, DVM_ERR_INVALID, "missing array");
  if (out.want_hits && T > h->hit_targets) return fail(fn, DVM_ERR_STATE, "the hit block holds fewer targets than the set");   // (an internal error: reserve keeps it in step)
  DVM_HIP(hipSetDevice(h->device));
  const size_t N = (size_t)n, E = N * (size_t)T;
  const WorkingSet& ws = h->ws;
  uint8_t* stage = ws.hm + h->tgt_bytes;
  uint8_t* dev = ws.d + h->tgt_bytes + h->grid_bytes;
  Cursor64 up{stage, dev};
  FtPoints A{};
  FtGather G{};
  if (P) {
    A.pos = reinterpret_cast<const float*>(up.put(P->pos, N * 12));
    A.normal = reinterpret_cast<const float*>(up.put(P->normal, N * 12));
    A.min_dist = reinterpret_cast<const float*>(up.put(P->min_dist, N * 4));
    A.max_dist = reinterpret_cast<const float*>(up.put(P->max_dist, N * 4));
    A.desc = up.put(P->desc, N * 32);
    A.valid = P->valid ? up.put(P->valid, N) : nullptr;
  } else if (src.slots) {
    G.slot = reinterpret_cast<const int32_t*>(up.put(src.slots->slot, N * 4));
    G.valid_in = src.slots->valid ? up.put(src.slots->valid, N) : nullptr;
  }
  A.skip = skip ? up.put(skip, E) : nullptr;
  A.n = n;
  Cursor64 tab{dev, nullptr, up.used()};          // a gathered table: device memory only, behind the upload
  if (!P) {
    G.records = reinterpret_cast<const uint32_t*>(st ? store_records(st) : nullptr);   // (no store: no slot names a point, nothing is read)
    G.pos = tab.carve<uint32_t>(N * 3); G.normal = tab.carve<uint32_t>(N * 3);
    G.min_dist = tab.carve<uint32_t>(N); G.max_dist = tab.carve<uint32_t>(N);
    G.desc = tab.carve<uint32_t>(N * 8); G.valid = tab.carve<uint8_t>(N);
    G.n = n;
    A.pos = reinterpret_cast<const float*>(G.pos); A.normal = reinterpret_cast<const float*>(G.normal);
    A.min_dist = reinterpret_cast<const float*>(G.min_dist); A.max_dist = reinterpret_cast<const float*>(G.max_dist);
    A.desc = reinterpret_cast<const uint8_t*>(G.desc); A.valid = G.valid;
  }
  if (tab.used() > h->pts_bytes) return fail(fn, DVM_ERR_STATE, "packed points exceed the reserved region");   // (an internal error)
  int32_t* d_idx = reinterpret_cast<int32_t*>(dev + h->pts_bytes);
  int32_t* d_dist = reinterpret_cast<int32_t*>(dev + h->pts_bytes + pad<64>(E * 4));
  int32_t* d_cnt = reinterpret_cast<int32_t*>(dev + h->pts_bytes + 2 * pad<64>(E * 4));
  int32_t* d_off = reinterpret_cast<int32_t*>(dev + h->pts_bytes + 2 * pad<64>(E * 4) + pad<64>(((size_t)T + 1) * 4));
  uint8_t* h_res = stage + h->pts_bytes;
  const size_t back = out.best_dist ? pad<64>(E * 4) + E * 4 : E * 4;
  // the mapped block of the hits: what the kernels write to, and where the host reads it after the synchronisation
  const size_t hit_at = pad<64>(((size_t)h->hit_targets + 1) * 4);
  const int cap = out.want_hits ? std::min(out.hit_cap, h->max_hits) : 0;
  // a candidates run: its lists packed flat, then the exclude list, into the staging of its own blocks
  FtCand C{};
  CandDev CD{};
  CandHost CH{};
  const size_t cblocks = cand_blocks(n);
  const int ccap = src.cand ? std::min(out.cand_cap, h->max_entries) : 0;
  int64_t up_bytes = (int64_t)up.used();
  if (src.cand) {
    CD = cand_dev_layout(h->cand_d, h->max_entries, h->map_capacity);
    CH = cand_host_layout(h->cand_hm, h->max_entries);
    Cursor64 cu{reinterpret_cast<uint8_t*>(CH.up), reinterpret_cast<uint8_t*>(CD.up)};
    int32_t* flat = cu.carve<int32_t>(N);
    fpl_flatten(*src.cand, flat);
    C.entry = rebase(flat, cu.base, cu.twin);
    C.exclude = reinterpret_cast<const int32_t*>(cu.put(src.cand->exclude, (size_t)src.cand->n_exclude * 4));
    C.n_entries = n; C.n_exclude = src.cand->n_exclude;
    C.records = G.records; C.first = CD.first; C.mark = CD.mark;
    G.slot = CD.cand; G.n_live = CD.off + cblocks; G.mark = CD.mark;
    DVM_HIP(hipMemcpyAsync(CD.up, CH.up, cu.used(), hipMemcpyHostToDevice, h->s));
    up_bytes += (int64_t)cu.used();
  }

  if (up.used()) DVM_HIP(hipMemcpyAsync(dev, stage, up.used(), hipMemcpyHostToDevice, h->s));
  h->run_bytes = up_bytes;
  if (h->store) { const int rb = kfs_read_begin(h->store, h->s); if (rb != DVM_OK) return rb; }
  if (st) { const int rb = store_read_begin(st, h->s); if (rb != DVM_OK) return rb; }
  if (src.cand)                                  // (off_out and cand_out: the mapped block, as the hits)
    launch_ft_candidates(h->s, C, CD.cnt, CD.off, rebase(CH.off_out, h->cand_hm, h->cand_hm_dev), CD.cand, rebase(CH.cand_out, h->cand_hm, h->cand_hm_dev), ccap);
  if (!P) launch_ft_gather(h->s, G);
  if (src.cand) launch_ft_cand_reset(h->s, C);   // (behind the gather: it reads the exclude marks)
  const EventTimer& tm = h->timer;
  DVM_HIP(tm.mark(2, h->s));
  if (T > 0)                                     // (T = 0 gets here in a candidates run only; n_pinhole / n_kb8 are those of the last set WITH targets)
    launch_ft_search(h->s, reinterpret_cast<const FtTargetDev*>(ws.d), h->order, h->n_pinhole, h->n_kb8, A, th, d_idx, d_dist);
  DVM_HIP(tm.mark(3, h->s));
  if (st) { const int re = store_read_end(st, h->s); if (re != DVM_OK) return re; }
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
  int n_c = 0;
  if (src.cand) {
    n_c = CH.off_out[cblocks];
    *out.n_cand = n_c;
    if (n_c <= ccap && n_c > 0) std::memcpy(out.cand_slot, CH.cand_out, (size_t)n_c * 4);
  }
  if (out.want_hits) {
    const int32_t* off = reinterpret_cast<const int32_t*>(h->hit_hm);
    const int total = T > 0 ? off[T] : 0;
    if (T > 0) std::memcpy(out.hit_off, off, ((size_t)T + 1) * 4); else out.hit_off[0] = 0;
    if (out.n_hits) *out.n_hits = total;
    if (n_c > ccap)
      return fail(fn, DVM_ERR_CAPACITY, std::to_string(n_c) + " candidates beyond cand_cap or the reservation (dvm_fuse_targets_reserve_candidates): " + std::to_string(ccap));
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
  FtSource src;
  src.table = P;
  FtResult out;
  out.best_idx = best_idx; out.best_dist = best_dist;
  return run_points("dvm_fuse_targets_run", h, src, skip, th, out);
}
int dvm_fuse_targets_run_hits(dvm_fuse_targets* h, const dvm_ft_points* P, const uint8_t* skip, float th, int32_t* hit_off, dvm_ft_hit* hits,
                              int hit_cap, int32_t* n_hits) {
  FtSource src;
  src.table = P;
  FtResult out;
  out.want_hits = true; out.hit_off = hit_off; out.hits = hits; out.hit_cap = hit_cap; out.n_hits = n_hits;
  return run_points("dvm_fuse_targets_run_hits", h, src, skip, th, out);
}
int dvm_fuse_targets_run_resident(dvm_fuse_targets* h, const dvm_ft_points_resident* P, const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist) {
  FtSource src;
  src.slots = P;
  FtResult out;
  out.best_idx = best_idx; out.best_dist = best_dist;
  return run_points("dvm_fuse_targets_run_resident", h, src, skip, th, out);
}
int dvm_fuse_targets_run_hits_resident(dvm_fuse_targets* h, const dvm_ft_points_resident* P, const uint8_t* skip, float th, int32_t* hit_off,
                                       dvm_ft_hit* hits, int hit_cap, int32_t* n_hits) {
  FtSource src;
  src.slots = P;
  FtResult out;
  out.want_hits = true; out.hit_off = hit_off; out.hits = hits; out.hit_cap = hit_cap; out.n_hits = n_hits;
  return run_points("dvm_fuse_targets_run_hits_resident", h, src, skip, th, out);
}
int dvm_fuse_targets_run_hits_candidates(dvm_fuse_targets* h, const dvm_ft_candidates* C, float th, int32_t* cand_slot, int cand_cap, int32_t* n_cand,
                                         int32_t* hit_off, dvm_ft_hit* hits, int hit_cap, int32_t* n_hits) {
  FtSource src;
  src.cand = C;
  FtResult out;
  out.want_hits = true; out.hit_off = hit_off; out.hits = hits; out.hit_cap = hit_cap; out.n_hits = n_hits;
  out.cand_slot = cand_slot; out.cand_cap = cand_cap; out.n_cand = n_cand;
  return run_points("dvm_fuse_targets_run_hits_candidates", h, src, nullptr, th, out);
}

}  // extern "C"
