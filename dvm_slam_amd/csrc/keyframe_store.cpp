// dvm_slam_amd/csrc/keyframe_store.cpp -- dvm_keyframe_store (include/dvmslam_hip.h): an agent's keyframes resident on the device.
//
// What a KeyFrame holds once ComputeBoW has run -- mvKeysUn, mDescriptors, the level tables, mFeatVec, the image bounds and the feature
// grid -- lives in one device block of `capacity` slots (kf_store_layout.h) that never moves.  LocalMapping puts a keyframe once; the
// Fuse chain and the CreateNewMapPoints chain read it step after step (fuse_targets.cpp: dvm_fuse_targets_set_resident; new_points.cpp:
// dvm_create_new_map_points_resident) and send only what changes, the pose and mvpMapPoints.
//
// Ordering is map_store.cpp's -- the store's own stream plus two events:
//   put      validates the whole batch, then in rounds: packs keyframes into the page-locked staging block ([items][arrays]), makes the
//            store's stream wait for `read_ev` (the last kernel a chain queued to read the store), sends ONE copy to the staging block's
//            device twin, launches k_kfs_put there and records `write_ev`.  It returns without waiting; the next round (or put) waits on
//            the host for `write_ev` before it touches the staging block again.
//   put_device  the keyframe's arrays are in device memory (kfs_put_device_run; keyframe_put_kernels.hip): the same wait for `read_ev`, an
//            event behind the stream that produced the arrays, ONE copy of the item records and level tables, the launches, `write_ev`
//            -- and then ONE synchronisation, because the host record of a slot (n, fv_n, n_feat) and the BowVector / FeatureVector the
//            caller gets come from mapped memory the kernels wrote.  A call the first kernel refuses changes no slot and no record.
//   a chain  kfs_read_begin: its stream waits for `write_ev`; kfs_read_end: `read_ev` recorded behind its reading kernels.
//   rows     (set_rows / patch_rows, below) two int32 rows per slot in blocks of their own, made by the first call that sets one: staged and
//            queued exactly as a put -- the staging block, the store's stream behind `read_ev`, `write_ev` --, and unset by every put,
//            put_device and remove of the slot (the slot's device length goes back to 0 on the store's stream).
// Safety: per slot the host keeps a written flag, a generation and the counts the kernels index with; every slot a call names is checked
// BEFORE anything is queued, and every count of a put is bounded by slot_keypoints, so no kernel runs on an unchecked value.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/dvmslam_hip.h"
#include "chain.h"
#include "fuse_points_lists.h"
#include "fv_once.h"
#include "keyframe_store.h"
#include "map_store.h"

using namespace dvm;

namespace {
constexpr int kStageKeyframes = 32;              // keyframes of the largest size one round holds (smaller ones: more)
struct SlotMeta {
  uint8_t written = 0;
  uint8_t fv_once = 0;                             // the FeatureVector lists every feature at most once (fv_once.h): what the BoW-targets search needs
  uint32_t gen = 0;
  int32_t n = 0, fv_n = 0, n_feat = 0, n_levels = 0;
  float fx = 0, fy = 0, cx = 0, cy = 0, min_x = 0, max_x = 0, min_y = 0, max_y = 0, log_scale_factor = 0;
};
int fail(const char* fn, int rc, const std::string& msg) { set_error(std::string(fn) + ": " + msg); return rc; }
}  // namespace

struct dvm_keyframe_store {
  int device = 0, capacity = 0, K = 0;
  KfSlotLayout L{};
  uint8_t* d = nullptr;                            // [capacity] slots of L.stride bytes
  uint8_t *hs = nullptr, *ds = nullptr;            // staging: page-locked, and its device twin; [items: capacity][arrays]
  size_t item_bytes = 0, stage_bytes = 0;
  hipStream_t s = nullptr;
  hipEvent_t write_ev = nullptr, read_ev = nullptr;
  bool write_pending = false, read_pending = false;
  std::vector<SlotMeta> meta;
  std::vector<uint32_t> stamp; uint32_t call = 0;  // per slot: the put call that named it last (a slot named twice in one call)
  std::vector<uint8_t> seen;                       // [K] scratch of the listed-once scan
  int64_t last_h2d = 0;                            // dvm_keyframe_store_last_put_bytes
  // ---- put_device (allocated by the first one): the upload ([KfsDevHead][capacity KfsDevItem], page-locked + device twin), the
  // transform's scratch for a round of keyframes, the mapped results of every keyframe a call can name, the event behind the caller's stream
  uint8_t *dv_hup = nullptr, *dv_dup = nullptr;
  uint8_t* dv_scratch = nullptr; int dv_round = 0;
  uint8_t *dv_hout = nullptr, *dv_dout = nullptr; size_t dv_out_stride = 0;
  hipEvent_t src_ev = nullptr;
  hipEvent_t tev[5] = {}; bool timing = false; float last_ms[4] = {0, 0, 0, 0};
  // ---- the rows (DVM_KFS_ROW_MATCHES, DVM_KFS_ROW_OBSERVED), per kind: the device block and the per-slot lengths (allocated by the first
  // call that sets a row of the kind), per slot whether its row is set and which map store its values name, and how many set rows name
  // each map store (a handful of stores at most: one agent, one map)
  struct RowMeta { uint8_t set = 0; const dvm_map_store* points = nullptr; };
  int32_t* rows_d[2] = {nullptr, nullptr}; int32_t* rowlen_d[2] = {nullptr, nullptr};
  size_t row_words = 0;
  std::vector<RowMeta> rowmeta[2];
  std::vector<std::pair<const dvm_map_store*, int>> row_stores[2];
  std::vector<int32_t> edit_order; std::vector<KfsRowEdit> edit_keep;   // patch_rows: the call's edits collapsed to one per cell
  void row_count(int which, const dvm_map_store* p, int d) {
    for (auto& e : row_stores[which])
      if (e.first == p) { e.second += d; return; }
    row_stores[which].emplace_back(p, d);
  }
  // the host half of unsetting slot's rows; true: a device length has to go back to 0
  bool rows_forget(int32_t sl) {
    bool any = false;
    for (int w = 0; w < 2; w++) {
      if (!rows_d[w] || !rowmeta[w][sl].set) continue;
      row_count(w, rowmeta[w][sl].points, -1);
      rowmeta[w][sl] = RowMeta();
      any = true;
    }
    return any;
  }
  // the device half, on the store's stream (the caller has made it wait for `read_ev` and records `write_ev` behind it): the lengths of
  // slots[0 .. n) back to 0, one memset per run of consecutive slots
  int rows_unset_device(const int32_t* slots, int n) {
    for (int w = 0; w < 2; w++) {
      if (!rowlen_d[w]) continue;
      for (int k = 0; k < n;) {
        int m = 1;
        while (k + m < n && slots[k + m] == slots[k] + m) m++;
        DVM_HIP(hipMemsetAsync(rowlen_d[w] + slots[k], 0, (size_t)m * 4, s));
        k += m;
      }
    }
    return DVM_OK;
  }
  uint8_t* slot_base(int32_t sl) const { return d + (size_t)sl * L.stride; }
  // the staging block is the host's again: the last round's copy has read it
  int staging_free() {
    if (write_pending) { DVM_HIP(hipEventSynchronize(write_ev)); write_pending = false; }
    return DVM_OK;
  }
};

namespace dvm {
int kfs_device(const dvm_keyframe_store* st) { return st->device; }
bool kfs_slot_view(const dvm_keyframe_store* st, int32_t slot, KfSlotView* v) {
  if ((uint32_t)slot >= (uint32_t)st->capacity || !st->meta[slot].written) return false;
  const SlotMeta& m = st->meta[slot];
  const KfSlotLayout& L = st->L;
  uint8_t* b = st->slot_base(slot);
  v->kps = reinterpret_cast<const dvm_keypoint_pod*>(b + L.kps);
  v->desc = b + L.desc;
  v->fv_node = reinterpret_cast<const int32_t*>(b + L.fv_node);
  v->fv_off = reinterpret_cast<const int32_t*>(b + L.fv_off);
  v->fv_feat = reinterpret_cast<const int32_t*>(b + L.fv_feat);
  v->sf = reinterpret_cast<const float*>(b + L.sf);
  v->sigma2 = reinterpret_cast<const float*>(b + L.sigma2);
  v->inv_sigma2 = reinterpret_cast<const float*>(b + L.inv_sigma2);
  FrameView& F = v->F;
  F.skp = reinterpret_cast<float4*>(b + L.skp);
  F.sidx = reinterpret_cast<int32_t*>(b + L.sidx);
  F.sdesc = b + L.sdesc;
  F.cell_start = reinterpret_cast<int32_t*>(b + L.cell_start);
  F.n_sorted = reinterpret_cast<int32_t*>(b + L.counters);
  F.n_total = F.n_sorted + 1;
  F.n_overflow = F.n_sorted + 2;
  F.cap = m.n;
  F.minX = m.min_x; F.minY = m.min_y;
  F.wInv = static_cast<float>(64) / static_cast<float>(m.max_x - m.min_x);   // Frame.cc:443-444, as dvm_frame_build
  F.hInv = static_cast<float>(48) / static_cast<float>(m.max_y - m.min_y);
  v->n = m.n; v->fv_n = m.fv_n; v->n_feat = m.n_feat; v->n_levels = m.n_levels;
  v->fx = m.fx; v->fy = m.fy; v->cx = m.cx; v->cy = m.cy;
  v->min_x = m.min_x; v->max_x = m.max_x; v->min_y = m.min_y; v->max_y = m.max_y; v->log_scale_factor = m.log_scale_factor;
  v->gen = m.gen; v->fv_once = m.fv_once != 0;
  return true;
}
uint32_t kfs_generation(const dvm_keyframe_store* st, int32_t slot) { return (uint32_t)slot < (uint32_t)st->capacity ? st->meta[slot].gen : 0u; }
int kfs_capacity(const dvm_keyframe_store* st) { return st->capacity; }
KfsRowsView kfs_rows_view(const dvm_keyframe_store* st, int which) { return KfsRowsView{st->rows_d[which], st->rowlen_d[which], st->row_words}; }
bool kfs_row_info(const dvm_keyframe_store* st, int which, int32_t slot, int32_t* n, const dvm_map_store** points) {
  if ((uint32_t)slot >= (uint32_t)st->capacity || !st->meta[slot].written || !st->rows_d[which] || !st->rowmeta[which][slot].set) return false;
  *n = st->meta[slot].n; *points = st->rowmeta[which][slot].points;
  return true;
}
bool kfs_rows_all_name(const dvm_keyframe_store* st, int which, const dvm_map_store* points) {
  for (const auto& e : st->row_stores[which])
    if (e.second > 0 && e.first != points) return false;
  return true;
}
KfsBlockView kfs_block_view(const dvm_keyframe_store* st) { return KfsBlockView{st->d, st->L.stride, st->L.kps, st->L.desc, st->L.sf}; }
int kfs_read_begin(const dvm_keyframe_store* cst, hipStream_t s) {
  dvm_keyframe_store* st = const_cast<dvm_keyframe_store*>(cst);
  if (!st->write_pending) return DVM_OK;
  if (hipEventQuery(st->write_ev) == hipSuccess) { st->write_pending = false; return DVM_OK; }   // (a put that has run needs no wait, now or later)
  (void)hipGetLastError();     // hipErrorNotReady is no error
  DVM_HIP(hipStreamWaitEvent(s, st->write_ev, 0));
  return DVM_OK;
}
int kfs_read_end(const dvm_keyframe_store* cst, hipStream_t s) {
  dvm_keyframe_store* st = const_cast<dvm_keyframe_store*>(cst);
  DVM_HIP(hipEventRecord(st->read_ev, s));
  st->read_pending = true;
  return DVM_OK;
}
}  // namespace dvm

namespace {
// everything dvm_fuse_targets_set and dvm_create_new_map_points check of a keyframe per call, once
int check_keyframe(const char* fn, const dvm_kfs_keyframe& k, const std::string& w, int K) {
  if (k.n < 0) return fail(fn, DVM_ERR_INVALID, w + ": negative n");
  if (k.n > K) return fail(fn, DVM_ERR_CAPACITY, w + ": " + std::to_string(k.n) + " keypoints beyond slot_keypoints " + std::to_string(K));
  if (k.n_levels < 1 || k.n_levels > 64) return fail(fn, DVM_ERR_INVALID, w + ": n_levels outside [1, 64]");
  if (!k.scale_factors || !k.level_sigma2 || !k.inv_level_sigma2) return fail(fn, DVM_ERR_INVALID, w + ": missing level table");
  if (!(k.max_x > k.min_x) || !(k.max_y > k.min_y)) return fail(fn, DVM_ERR_INVALID, w + ": image bounds empty");
  if (k.n > 0 && (!k.kps || !k.desc)) return fail(fn, DVM_ERR_INVALID, w + ": missing keypoint array");
  for (int i = 0; i < k.n; i++)
    if ((uint32_t)k.kps[i].octave >= (uint32_t)k.n_levels) return fail(fn, DVM_ERR_INVALID, w + ": a keypoint's octave outside the level tables");
  if (k.fv_n < 0) return fail(fn, DVM_ERR_INVALID, w + ": negative fv_n");
  if (k.fv_n > K) return fail(fn, DVM_ERR_CAPACITY, w + ": " + std::to_string(k.fv_n) + " FeatureVector nodes beyond slot_keypoints " + std::to_string(K));
  if (k.fv_n > k.n) return fail(fn, DVM_ERR_INVALID, w + ": more FeatureVector nodes than keypoints");
  if (k.fv_n > 0) {
    if (!k.fv_node || !k.fv_off || !k.fv_feat) return fail(fn, DVM_ERR_INVALID, w + ": missing FeatureVector array");
    if (k.fv_off[0] != 0) return fail(fn, DVM_ERR_INVALID, w + ": FeatureVector offsets do not start at 0");
    for (int a = 0; a < k.fv_n; a++) {
      if (k.fv_off[a + 1] < k.fv_off[a]) return fail(fn, DVM_ERR_INVALID, w + ": FeatureVector offsets not monotone");
      if (a > 0 && (uint32_t)k.fv_node[a] <= (uint32_t)k.fv_node[a - 1])
        return fail(fn, DVM_ERR_INVALID, w + ": FeatureVector nodes not ascending (as unsigned: node -1 is last)");
    }
    const int nf = k.fv_off[k.fv_n];
    if (nf > k.n) return fail(fn, DVM_ERR_INVALID, w + ": more FeatureVector features than keypoints");
    for (int f = 0; f < nf; f++)
      if (k.fv_feat[f] < 0 || k.fv_feat[f] >= k.n) return fail(fn, DVM_ERR_INVALID, w + ": FeatureVector feature index out of range");
  }
  return DVM_OK;
}

// ---- put_device
// one keyframe's mapped results: the counts, then the BowVector and the FeatureVector, each sized for K keypoints and rounded up
dvm::KfsDevOut carve_dev_out(uint8_t* base, size_t K, size_t* bytes) {
  Cursor<kKfsAlign> c{base};
  KfsDevOut o{};
  o.res = c.carve<KfsDevRes>(1);
  o.bow_ids = c.carve<int32_t>(K); o.bow_vals = c.carve<double>(K);
  o.fv_node = c.carve<int32_t>(K); o.fv_off = c.carve<int32_t>(K + 1); o.fv_feat = c.carve<int32_t>(K);
  if (bytes) *bytes = c.used();
  return o;
}
KfsDevScratch carve_dev_scratch(uint8_t* base, size_t round, size_t K, size_t* bytes) {
  Cursor<kKfsAlign> c{base};
  KfsDevScratch w{};
  w.w = c.carve<double>(round * K); w.word = c.carve<int32_t>(round * K); w.node = c.carve<int32_t>(round * K);
  if (bytes) *bytes = c.used();
  return w;
}
// the first put_device of a store reserves what the form needs
int dev_reserve(const char* fn, dvm_keyframe_store* st) {
  if (st->dv_hup) return DVM_OK;
  const size_t C = (size_t)st->capacity, K = (size_t)st->K, up = sizeof(KfsDevHead) + C * sizeof(KfsDevItem);
  size_t out_stride = 0, scratch = 0;
  carve_dev_out(nullptr, K, &out_stride);
  const int round = std::min(st->capacity, kStageKeyframes);
  carve_dev_scratch(nullptr, (size_t)round, K, &scratch);
  uint8_t *hup = nullptr, *dup = nullptr, *sc = nullptr, *hout = nullptr, *dout = nullptr;
  hipEvent_t ev = nullptr;
  const bool ok = hipHostMalloc(reinterpret_cast<void**>(&hup), up, hipHostMallocDefault) == hipSuccess &&
                  hipMalloc(reinterpret_cast<void**>(&dup), up) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&sc), scratch) == hipSuccess &&
                  hipHostMalloc(reinterpret_cast<void**>(&hout), C * out_stride, hipHostMallocMapped) == hipSuccess &&
                  hipHostGetDevicePointer(reinterpret_cast<void**>(&dout), hout, 0) == hipSuccess &&
                  hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    if (hup) (void)hipHostFree(hup);
    if (dup) (void)hipFree(dup);
    if (sc) (void)hipFree(sc);
    if (hout) (void)hipHostFree(hout);
    if (ev) (void)hipEventDestroy(ev);
    return fail(fn, DVM_ERR_CAPACITY, "the working set of the device put (item table, transform scratch, mapped results)");
  }
  std::memset(hout, 0, C * out_stride);
  st->dv_hup = hup; st->dv_dup = dup; st->dv_scratch = sc; st->dv_round = round; st->dv_hout = hout; st->dv_dout = dout; st->dv_out_stride = out_stride;
  st->src_ev = ev;
  return DVM_OK;
}
}  // namespace

namespace dvm {
int vocab_device(const dvm_vocab* v);           // capi.cpp: the vocabulary's device and its transform of device features (count on the device)
void vocab_launch_transform(const dvm_vocab* v, hipStream_t s, const uint8_t* d_feat, int cap, const int32_t* d_n, int levelsup, int32_t* word_id,
                            int32_t* node_id, double* weight, const int32_t* run, int nrun, int64_t feat_stride);

int kfs_put_device_run(const char* fn, dvm_keyframe_store* st, const dvm_vocab* voc, int levelsup, hipStream_t src, int n, const int32_t* slots,
                       const dvm_kfs_device_keyframe* kfs, dvm_kfs_bow_out* outs) {
  if (!st || !voc || n < 0 || (n && (!slots || !kfs))) return fail(fn, DVM_ERR_INVALID, "missing argument");
  if (n == 0) return DVM_OK;
  // what the host can see of the batch is decided before anything is queued
  if (++st->call == 0) { std::fill(st->stamp.begin(), st->stamp.end(), 0u); st->call = 1; }
  const int K = st->K;
  for (int k = 0; k < n; k++) {
    const int32_t sl = slots[k];
    const dvm_kfs_device_keyframe& f = kfs[k];
    const std::string w = "keyframe " + std::to_string(k) + " (slot " + std::to_string(sl) + ")";
    if (sl < 0 || sl >= st->capacity) return fail(fn, DVM_ERR_INVALID, w + ": slot outside [0, capacity)");
    if (st->stamp[sl] == st->call) return fail(fn, DVM_ERR_INVALID, w + ": slot named twice in one call");
    st->stamp[sl] = st->call;
    if (f.n < 0) return fail(fn, DVM_ERR_INVALID, w + ": negative n");
    if (!f.d_n && f.n > K) return fail(fn, DVM_ERR_CAPACITY, w + ": " + std::to_string(f.n) + " keypoints beyond slot_keypoints " + std::to_string(K));
    if (f.n_levels < 1 || f.n_levels > 64) return fail(fn, DVM_ERR_INVALID, w + ": n_levels outside [1, 64]");
    if (!f.scale_factors || !f.level_sigma2 || !f.inv_level_sigma2) return fail(fn, DVM_ERR_INVALID, w + ": missing level table");
    if (!(f.max_x > f.min_x) || !(f.max_y > f.min_y)) return fail(fn, DVM_ERR_INVALID, w + ": image bounds empty");
    if (f.n > 0 && (!f.d_kps || !f.d_desc)) return fail(fn, DVM_ERR_INVALID, w + ": missing keypoint array");
    if (((reinterpret_cast<uintptr_t>(f.d_kps) | reinterpret_cast<uintptr_t>(f.d_desc) | reinterpret_cast<uintptr_t>(f.d_n)) & 3) != 0)
      return fail(fn, DVM_ERR_INVALID, w + ": an array not aligned to 4 bytes");
  }
  if (vocab_device(voc) != st->device) return fail(fn, DVM_ERR_INVALID, "the vocabulary lives on another device");
  DVM_HIP(hipSetDevice(st->device));
  { const int rc = dev_reserve(fn, st); if (rc != DVM_OK) return rc; }
  // the one upload: the flag, then per keyframe the item record and the three level tables
  KfsDevHead* hh = reinterpret_cast<KfsDevHead*>(st->dv_hup);
  KfsDevItem* hi = reinterpret_cast<KfsDevItem*>(st->dv_hup + sizeof(KfsDevHead));
  KfsDevHead* dh = reinterpret_cast<KfsDevHead*>(st->dv_dup);
  KfsDevItem* di = reinterpret_cast<KfsDevItem*>(st->dv_dup + sizeof(KfsDevHead));
  std::memset(hh, 0, sizeof(*hh));
  hh->flag = kKfsDevNoFlag;
  for (int k = 0; k < n; k++) {
    const dvm_kfs_device_keyframe& f = kfs[k];
    KfsDevItem& it = hi[k];
    std::memset(&it, 0, sizeof(it));
    it.kps = reinterpret_cast<const dvm_keypoint_pod*>(f.d_kps); it.desc = f.d_desc; it.d_n = f.d_n;
    it.slot = st->slot_base(slots[k]);
    it.cap = f.n; it.n_levels = f.n_levels;
    it.minX = f.min_x; it.minY = f.min_y;
    it.wInv = static_cast<float>(64) / static_cast<float>(f.max_x - f.min_x);   // Frame.cc:443-444, as dvm_frame_build
    it.hInv = static_cast<float>(48) / static_cast<float>(f.max_y - f.min_y);
    std::memcpy(it.sf, f.scale_factors, (size_t)f.n_levels * 4);
    std::memcpy(it.sigma2, f.level_sigma2, (size_t)f.n_levels * 4);
    std::memcpy(it.inv_sigma2, f.inv_level_sigma2, (size_t)f.n_levels * 4);
  }
  const size_t up = sizeof(KfsDevHead) + (size_t)n * sizeof(KfsDevItem), os = st->dv_out_stride;
  hipStream_t s = st->s;
  if (st->read_pending) {                                          // behind the chain kernels that read the slots
    DVM_HIP(hipStreamWaitEvent(s, st->read_ev, 0));
    st->read_pending = false;
  }
  DVM_HIP(hipEventRecord(st->src_ev, src));                        // behind what produced the arrays
  DVM_HIP(hipStreamWaitEvent(s, st->src_ev, 0));
  DVM_HIP(hipMemcpyAsync(st->dv_dup, st->dv_hup, up, hipMemcpyHostToDevice, s));
  st->last_h2d = (int64_t)up;
  const bool tm = st->timing;
  const KfsDevOut out_dev = carve_dev_out(st->dv_dout, (size_t)K, nullptr);
  if (tm) DVM_HIP(hipEventRecord(st->tev[0], s));
  launch_kfs_dev_check(s, dh, di, n, K, out_dev.res, os);
  if (tm) DVM_HIP(hipEventRecord(st->tev[1], s));
  const KfsDevScratch W = carve_dev_scratch(st->dv_scratch, (size_t)st->dv_round, (size_t)K, nullptr);
  for (int first = 0; first < n; first += st->dv_round) {
    const int m = std::min(st->dv_round, n - first);
    for (int r = 0; r < m; r++) {
      const dvm_kfs_device_keyframe& f = kfs[first + r];
      vocab_launch_transform(voc, s, f.d_desc, std::min(f.n, K), &di[first + r].count, levelsup, W.word + (size_t)r * K, W.node + (size_t)r * K,
                             W.w + (size_t)r * K, nullptr, 1, 0);
    }
    if (tm && first == 0) DVM_HIP(hipEventRecord(st->tev[2], s));
    KfsDevOut o = out_dev;
    const size_t ob = (size_t)first * os;
    auto mv = [ob](auto*& p) { p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(reinterpret_cast<uint8_t*>(p) + ob); };
    mv(o.res); mv(o.bow_ids); mv(o.bow_vals); mv(o.fv_node); mv(o.fv_off); mv(o.fv_feat);
    if (!launch_kfs_dev_bow(s, dh, di, first, m, K, W, st->L, o, os)) {
      (void)hipStreamSynchronize(s);
      return fail(fn, DVM_ERR_CAPACITY, "the LDS of the FeatureVector sort (16 B per keypoint of the slot size rounded up to a power of two)");
    }
    if (tm && first == 0) DVM_HIP(hipEventRecord(st->tev[3], s));
    launch_kfs_dev_put(s, dh, di, first, m, st->L, o.res, os);
    if (tm && first == 0) DVM_HIP(hipEventRecord(st->tev[4], s));
  }
  { const int rc = hip_check(hipGetLastError(), "the device put's launches"); if (rc != DVM_OK) return rc; }
  DVM_HIP(hipEventRecord(st->write_ev, s));
  st->write_pending = true;
  // the ONE synchronisation: the flag, the counts, the BowVector and the FeatureVector lie in mapped memory behind it
  DVM_HIP(hipStreamSynchronize(s));
  st->write_pending = false;
  if (tm)
    for (int i = 0; i < 4; i++) DVM_HIP(hipEventElapsedTime(&st->last_ms[i], st->tev[i], st->tev[i + 1]));
  const KfsDevOut out_host = carve_dev_out(st->dv_hout, (size_t)K, nullptr);
  auto host_at = [&](auto* p, int k) { return reinterpret_cast<decltype(p)>(reinterpret_cast<uint8_t*>(p) + (size_t)k * os); };
  const int32_t flag = host_at(out_host.res, 0)->flag;
  if (flag != kKfsDevNoFlag) {
    const int k = flag >> 1;
    const std::string w = "keyframe " + std::to_string(k) + " (slot " + std::to_string(k < n ? slots[k] : -1) + ")";
    if (flag & 1) return fail(fn, DVM_ERR_INVALID, w + ": a keypoint's octave outside the level tables; no slot of the call written");
    return fail(fn, DVM_ERR_CAPACITY, w + ": " + std::to_string(k < n ? host_at(out_host.res, k)->n : 0) + " keypoints beyond slot_keypoints " +
                                          std::to_string(K) + "; no slot of the call written");
  }
  {                                                                // a new keyframe holds nothing until it is told: the slots' rows are unset
    bool any = false;
    for (int k = 0; k < n; k++) any |= st->rows_forget(slots[k]);
    if (any) {
      { const int rc = st->rows_unset_device(slots, n); if (rc != DVM_OK) return rc; }
      DVM_HIP(hipEventRecord(st->write_ev, s));
      st->write_pending = true;
    }
  }
  for (int k = 0; k < n; k++) {
    const dvm_kfs_device_keyframe& f = kfs[k];
    const KfsDevRes& R = *host_at(out_host.res, k);
    SlotMeta& M = st->meta[slots[k]];
    M.written = 1; M.gen++;
    M.n = R.n; M.fv_n = R.n_fv; M.n_feat = R.n_feat; M.n_levels = f.n_levels;
    M.fv_once = 1;                                                 // a feature lies in one node: the transform gives each feature one
    M.fx = f.fx; M.fy = f.fy; M.cx = f.cx; M.cy = f.cy;
    M.min_x = f.min_x; M.max_x = f.max_x; M.min_y = f.min_y; M.max_y = f.max_y; M.log_scale_factor = f.log_scale_factor;
    if (!outs) continue;
    dvm_kfs_bow_out& o = outs[k];
    o.n = R.n; o.n_bow = R.n_bow; o.n_fv = R.n_fv; o.n_feat = R.n_feat;
    if (o.bow_ids) std::memcpy(o.bow_ids, host_at(out_host.bow_ids, k), (size_t)R.n_bow * 4);
    if (o.bow_vals) std::memcpy(o.bow_vals, host_at(out_host.bow_vals, k), (size_t)R.n_bow * 8);
    if (o.fv_node) std::memcpy(o.fv_node, host_at(out_host.fv_node, k), (size_t)R.n_fv * 4);
    if (o.fv_off) std::memcpy(o.fv_off, host_at(out_host.fv_off, k), ((size_t)R.n_fv + 1) * 4);
    if (o.fv_feat) std::memcpy(o.fv_feat, host_at(out_host.fv_feat, k), (size_t)R.n_feat * 4);
  }
  return DVM_OK;
}
}  // namespace dvm

extern "C" {

int dvm_keyframe_store_create(int device, int capacity, int slot_keypoints, dvm_keyframe_store** out) {
  static_assert(sizeof(dvm_keypoint) == kKfsKeypointBytes && sizeof(dvm_keypoint_pod) == kKfsKeypointBytes, "layout");
  static_assert(kCellStartStride == (int)kKfsCellStart, "layout");
  const char* fn = "dvm_keyframe_store_create";
  if (!out) return DVM_ERR_INVALID;
  *out = nullptr;
  if (capacity < 1 || slot_keypoints < 1 || slot_keypoints > kFrameCap) return fail(fn, DVM_ERR_INVALID, "capacity < 1 or slot_keypoints outside [1, 8192]");
  { const int rc = need_device(device); if (rc != DVM_OK) return rc; }
  dvm_keyframe_store* st = new (std::nothrow) dvm_keyframe_store();
  if (!st) return DVM_ERR_INVALID;
  st->device = device; st->capacity = capacity; st->K = slot_keypoints;
  st->L = kf_slot_layout((size_t)slot_keypoints);
  st->row_words = pad<16>((size_t)slot_keypoints);
  const size_t C = (size_t)capacity, block = C * st->L.stride;
  st->item_bytes = pad<256>(C * sizeof(KfsPutItem));
  st->stage_bytes = st->item_bytes + (size_t)std::min(capacity, kStageKeyframes) * kf_stage_bytes_max((size_t)slot_keypoints);
  const char* what = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&st->d), block) != hipSuccess) { st->d = nullptr; what = "hipMalloc"; }
  else if (hipMalloc(reinterpret_cast<void**>(&st->ds), st->stage_bytes) != hipSuccess) { st->ds = nullptr; what = "hipMalloc of the staging twin"; }
  else if (hipHostMalloc(reinterpret_cast<void**>(&st->hs), st->stage_bytes, hipHostMallocDefault) != hipSuccess) { st->hs = nullptr; what = "page-locked staging"; }
  if (what) {
    (void)hipGetLastError();
    dvm_keyframe_store_destroy(st);
    return fail(fn, DVM_ERR_CAPACITY, std::string(what) + " (capacity " + std::to_string(capacity) + ", slot_keypoints " + std::to_string(slot_keypoints) + ")");
  }
  if (hipStreamCreateWithFlags(&st->s, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&st->write_ev, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&st->read_ev, hipEventDisableTiming) != hipSuccess || hipMemsetAsync(st->d, 0, block, st->s) != hipSuccess ||
      hipStreamSynchronize(st->s) != hipSuccess) {
    dvm_keyframe_store_destroy(st);
    return fail(fn, DVM_ERR_HIP, "stream, events or clearing the slots");
  }
  st->meta.assign(C, SlotMeta()); st->stamp.assign(C, 0); st->seen.assign((size_t)slot_keypoints, 0);
  *out = st;
  return DVM_OK;
}

void dvm_keyframe_store_destroy(dvm_keyframe_store* st) {
  if (!st) return;
  (void)hipSetDevice(st->device);
  if (st->s) (void)hipStreamSynchronize(st->s);
  if (st->read_pending && st->read_ev) (void)hipEventSynchronize(st->read_ev);   // a chain still reading the slots
  if (st->s) (void)hipStreamDestroy(st->s);
  if (st->write_ev) (void)hipEventDestroy(st->write_ev);
  if (st->read_ev) (void)hipEventDestroy(st->read_ev);
  if (st->d) (void)hipFree(st->d);
  if (st->ds) (void)hipFree(st->ds);
  if (st->hs) (void)hipHostFree(st->hs);
  if (st->dv_dup) (void)hipFree(st->dv_dup);
  if (st->dv_scratch) (void)hipFree(st->dv_scratch);
  if (st->dv_hup) (void)hipHostFree(st->dv_hup);
  if (st->dv_hout) (void)hipHostFree(st->dv_hout);
  if (st->src_ev) (void)hipEventDestroy(st->src_ev);
  for (int w = 0; w < 2; w++) {
    if (st->rows_d[w]) (void)hipFree(st->rows_d[w]);
    if (st->rowlen_d[w]) (void)hipFree(st->rowlen_d[w]);
  }
  for (hipEvent_t e : st->tev) if (e) (void)hipEventDestroy(e);
  delete st;
}

int dvm_keyframe_store_capacity(const dvm_keyframe_store* st) { return st ? st->capacity : DVM_ERR_INVALID; }
int dvm_keyframe_store_slot_keypoints(const dvm_keyframe_store* st) { return st ? st->K : DVM_ERR_INVALID; }

int dvm_keyframe_store_put(dvm_keyframe_store* st, int n, const int32_t* slots, const dvm_kfs_keyframe* kfs) {
  const char* fn = "dvm_keyframe_store_put";
  if (!st || n < 0 || (n && (!slots || !kfs))) return fail(fn, DVM_ERR_INVALID, "missing argument");
  if (n == 0) return DVM_OK;
  // the whole batch is decided before anything is staged or queued
  if (++st->call == 0) { std::fill(st->stamp.begin(), st->stamp.end(), 0u); st->call = 1; }
  for (int k = 0; k < n; k++) {
    const int32_t sl = slots[k];
    const std::string w = "keyframe " + std::to_string(k) + " (slot " + std::to_string(sl) + ")";
    if (sl < 0 || sl >= st->capacity) return fail(fn, DVM_ERR_INVALID, w + ": slot outside [0, capacity)");
    if (st->stamp[sl] == st->call) return fail(fn, DVM_ERR_INVALID, w + ": slot named twice in one call");
    st->stamp[sl] = st->call;
    const int rc = check_keyframe(fn, kfs[k], w, st->K);
    if (rc != DVM_OK) return rc;
  }
  DVM_HIP(hipSetDevice(st->device));
  KfsPutItem* items = reinterpret_cast<KfsPutItem*>(st->hs);
  st->last_h2d = 0;
  for (int done = 0; done < n;) {
    { const int rc = st->staging_free(); if (rc != DVM_OK) return rc; }
    Cursor<kKfsAlign> c{st->hs, st->ds, st->item_bytes};
    int m = 0;
    for (; done + m < n; m++) {
      const dvm_kfs_keyframe& k = kfs[done + m];
      const size_t nf = k.fv_n > 0 ? (size_t)k.fv_off[k.fv_n] : 0, nl = (size_t)k.n_levels;
      if (c.used() + kf_stage_bytes((size_t)k.n, (size_t)k.fv_n, nf, nl) > st->stage_bytes) break;   // (the first of a round always fits)
      KfsPutItem& it = items[m];
      it.src = c.put(k.kps, (size_t)k.n * kKfsKeypointBytes);
      c.put(k.desc, (size_t)k.n * 32);
      c.put(k.fv_node, (size_t)k.fv_n * 4);
      c.put(k.fv_off, k.fv_n > 0 ? ((size_t)k.fv_n + 1) * 4 : 0);
      c.put(k.fv_feat, nf * 4);
      c.put(k.scale_factors, nl * 4);
      c.put(k.level_sigma2, nl * 4);
      c.put(k.inv_level_sigma2, nl * 4);
      it.slot = st->slot_base(slots[done + m]);
      it.n = k.n; it.fv_n = k.fv_n; it.n_feat = (int32_t)nf; it.n_levels = k.n_levels;
      it.minX = k.min_x; it.minY = k.min_y;
      it.wInv = static_cast<float>(64) / static_cast<float>(k.max_x - k.min_x);   // Frame.cc:443-444, as dvm_frame_build
      it.hInv = static_cast<float>(48) / static_cast<float>(k.max_y - k.min_y);
    }
    if (m == 0) return fail(fn, DVM_ERR_STATE, "a keyframe exceeds the staging block");   // (an internal error: kf_stage_bytes_max bounds every keyframe)
    if (st->read_pending) {                                        // behind the chain kernels that read the slots
      DVM_HIP(hipStreamWaitEvent(st->s, st->read_ev, 0));
      st->read_pending = false;
    }
    // the items and the arrays in one copy (the gap between them, when the batch is smaller than the capacity, travels too: at most 48 B per slot)
    DVM_HIP(hipMemcpyAsync(st->ds, st->hs, c.used(), hipMemcpyHostToDevice, st->s));
    st->last_h2d += (int64_t)c.used();
    launch_kfs_put(st->s, reinterpret_cast<const KfsPutItem*>(st->ds), m, st->L);
    { const int rc = hip_check(hipGetLastError(), "k_kfs_put"); if (rc != DVM_OK) return rc; }
    {                                                              // a new keyframe holds nothing until it is told: the slots' rows are unset
      bool any = false;
      for (int k = done; k < done + m; k++) any |= st->rows_forget(slots[k]);
      if (any) { const int rc = st->rows_unset_device(slots + done, m); if (rc != DVM_OK) return rc; }
    }
    DVM_HIP(hipEventRecord(st->write_ev, st->s));
    st->write_pending = true;
    for (int k = done; k < done + m; k++) {
      const dvm_kfs_keyframe& f = kfs[k];
      SlotMeta& M = st->meta[slots[k]];
      M.written = 1; M.gen++;
      M.n = f.n; M.fv_n = f.fv_n; M.n_feat = f.fv_n > 0 ? f.fv_off[f.fv_n] : 0; M.n_levels = f.n_levels;
      // put accepts a feature listed in two nodes (Fuse and CreateNewMapPoints do not mind); the slot remembers it for the chain that does
      M.fv_once = fv_first_repeat(f.fv_feat, M.n_feat, f.n, st->seen.data()) < 0;
      M.fx = f.fx; M.fy = f.fy; M.cx = f.cx; M.cy = f.cy;
      M.min_x = f.min_x; M.max_x = f.max_x; M.min_y = f.min_y; M.max_y = f.max_y; M.log_scale_factor = f.log_scale_factor;
    }
    done += m;
  }
  return DVM_OK;
}

int dvm_keyframe_store_put_device(dvm_keyframe_store* st, const dvm_vocab* voc, int levelsup, void* stream, int n, const int32_t* slots,
                                  const dvm_kfs_device_keyframe* kfs, dvm_kfs_bow_out* outs) {
  return kfs_put_device_run("dvm_keyframe_store_put_device", st, voc, levelsup, (hipStream_t)stream, n, slots, kfs, outs);
}

int dvm_keyframe_store_last_put_bytes(const dvm_keyframe_store* st, int64_t* host_to_device) {
  if (!st || !host_to_device) return DVM_ERR_INVALID;
  *host_to_device = st->last_h2d;
  return DVM_OK;
}

int dvm_keyframe_store_profile(dvm_keyframe_store* st, int enable) {
  if (!st) return DVM_ERR_INVALID;
  DVM_HIP(hipSetDevice(st->device));
  if (enable)
    for (hipEvent_t& e : st->tev) if (!e) DVM_HIP(hipEventCreate(&e));
  st->timing = enable != 0;
  return DVM_OK;
}

int dvm_keyframe_store_last_put_ms(const dvm_keyframe_store* st, float ms[4]) {
  if (!st || !ms) return DVM_ERR_INVALID;
  for (int i = 0; i < 4; i++) ms[i] = st->last_ms[i];
  return DVM_OK;
}

int dvm_keyframe_store_remove(dvm_keyframe_store* st, int n, const int32_t* slots) {
  const char* fn = "dvm_keyframe_store_remove";
  if (!st || n < 0 || (n && !slots)) return fail(fn, DVM_ERR_INVALID, "missing argument");
  for (int k = 0; k < n; k++)
    if ((uint32_t)slots[k] >= (uint32_t)st->capacity || !st->meta[slots[k]].written)
      return fail(fn, DVM_ERR_INVALID, "slot " + std::to_string(slots[k]) + " outside [0, capacity) or not written");
  bool any = false;
  for (int k = 0; k < n; k++) {
    SlotMeta& M = st->meta[slots[k]];
    if (M.written) { M.written = 0; M.gen++; }
    any |= st->rows_forget(slots[k]);
  }
  if (any) {                                                       // the slots' row lengths on the device, queued as a put
    DVM_HIP(hipSetDevice(st->device));
    if (st->read_pending) {
      DVM_HIP(hipStreamWaitEvent(st->s, st->read_ev, 0));
      st->read_pending = false;
    }
    { const int rc = st->rows_unset_device(slots, n); if (rc != DVM_OK) return rc; }
    DVM_HIP(hipEventRecord(st->write_ev, st->s));
    st->write_pending = true;
  }
  return DVM_OK;
}

int dvm_keyframe_store_debug_read(dvm_keyframe_store* st, int slot, dvm_kfs_readback* out) {
  const char* fn = "dvm_keyframe_store_debug_read";
  if (!st || !out) return fail(fn, DVM_ERR_INVALID, "missing argument");
  if ((uint32_t)slot >= (uint32_t)st->capacity || !st->meta[slot].written)
    return fail(fn, DVM_ERR_INVALID, "slot " + std::to_string(slot) + " outside [0, capacity) or not written");
  DVM_HIP(hipSetDevice(st->device));
  DVM_HIP(hipStreamSynchronize(st->s));
  st->write_pending = false;
  std::vector<uint8_t> h(st->L.stride);
  DVM_HIP(hipMemcpy(h.data(), st->slot_base(slot), st->L.stride, hipMemcpyDeviceToHost));
  const SlotMeta& M = st->meta[slot];
  const KfSlotLayout& L = st->L;
  const int32_t* cnt = reinterpret_cast<const int32_t*>(h.data() + L.counters);
  out->n = M.n; out->fv_n = M.fv_n; out->n_feat = M.n_feat; out->n_levels = M.n_levels;
  out->n_sorted = cnt[0]; out->n_total = cnt[1];
  out->fx = M.fx; out->fy = M.fy; out->cx = M.cx; out->cy = M.cy;
  out->min_x = M.min_x; out->max_x = M.max_x; out->min_y = M.min_y; out->max_y = M.max_y; out->log_scale_factor = M.log_scale_factor;
  out->generation = M.gen;
  if (cnt[0] < 0 || cnt[0] > M.n) return fail(fn, DVM_ERR_STATE, "the slot's grid counter lies outside [0, n]");
  const size_t n = (size_t)M.n, ns = (size_t)cnt[0];
  auto give = [&](void* dst, size_t at, size_t bytes) { if (dst && bytes) std::memcpy(dst, h.data() + at, bytes); };
  give(out->kps, L.kps, n * kKfsKeypointBytes);
  give(out->desc, L.desc, n * 32);
  give(out->fv_node, L.fv_node, (size_t)M.fv_n * 4);
  give(out->fv_off, L.fv_off, M.fv_n > 0 ? ((size_t)M.fv_n + 1) * 4 : 0);
  give(out->fv_feat, L.fv_feat, (size_t)M.n_feat * 4);
  give(out->scale_factors, L.sf, (size_t)M.n_levels * 4);
  give(out->level_sigma2, L.sigma2, (size_t)M.n_levels * 4);
  give(out->inv_level_sigma2, L.inv_sigma2, (size_t)M.n_levels * 4);
  give(out->skp, L.skp, ns * 16);
  give(out->sidx, L.sidx, ns * 4);
  give(out->sdesc, L.sdesc, ns * 32);
  give(out->cell_start, L.cell_start, kKfsCellStart * 4);
  return DVM_OK;
}

}  // extern "C"

// ---- the rows beside the keyframes
namespace {
const char* row_name(int which) { return which == DVM_KFS_ROW_MATCHES ? "MATCHES" : "OBSERVED"; }
// what both row calls check of their arguments before they look at a slot
int rows_args(const char* fn, const dvm_keyframe_store* st, int which, const dvm_map_store* points) {
  if (which != DVM_KFS_ROW_MATCHES && which != DVM_KFS_ROW_OBSERVED) return fail(fn, DVM_ERR_INVALID, "which = " + std::to_string(which) + ": not DVM_KFS_ROW_MATCHES or DVM_KFS_ROW_OBSERVED");
  if (!points) return fail(fn, DVM_ERR_INVALID, "missing map store");
  if (store_device(points) != st->device) return fail(fn, DVM_ERR_INVALID, "the map store lives on another device");
  return DVM_OK;
}
// the first row call of a kind makes the kind's block: every word -1, every length 0
int rows_reserve(const char* fn, dvm_keyframe_store* st, int which) {
  if (st->rows_d[which]) return DVM_OK;
  const size_t C = (size_t)st->capacity, bytes = C * st->row_words * 4;
  int32_t *r = nullptr, *l = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&r), bytes) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&l), C * 4) != hipSuccess) {
    (void)hipGetLastError();
    if (r) (void)hipFree(r);
    return fail(fn, DVM_ERR_CAPACITY, std::string("the block of the ") + row_name(which) + " rows (" + std::to_string(bytes) + " bytes)");
  }
  if (hipMemsetAsync(r, 0xff, bytes, st->s) != hipSuccess || hipMemsetAsync(l, 0, C * 4, st->s) != hipSuccess || hipStreamSynchronize(st->s) != hipSuccess) {
    (void)hipFree(r); (void)hipFree(l);
    return fail(fn, DVM_ERR_HIP, "clearing the rows");
  }
  st->rows_d[which] = r; st->rowlen_d[which] = l;
  st->rowmeta[which].assign(C, dvm_keyframe_store::RowMeta());
  return DVM_OK;
}
// slot's row of the kind is set and names `points` from now on (host state)
void row_mark_set(dvm_keyframe_store* st, int which, int32_t sl, const dvm_map_store* points) {
  dvm_keyframe_store::RowMeta& R = st->rowmeta[which][sl];
  if (R.set) st->row_count(which, R.points, -1);
  R.set = 1; R.points = points;
  st->row_count(which, points, +1);
}
}  // namespace

extern "C" {

int dvm_keyframe_store_set_rows(dvm_keyframe_store* st, int which, const dvm_map_store* points, int n, const int32_t* slots, const int32_t* const* rows) {
  const char* fn = "dvm_keyframe_store_set_rows";
  if (!st || n < 0 || (n && (!slots || !rows))) return fail(fn, DVM_ERR_INVALID, "missing argument");
  { const int rc = rows_args(fn, st, which, points); if (rc != DVM_OK) return rc; }
  if (n == 0) return DVM_OK;
  // the whole batch is decided before anything is staged or queued
  if (++st->call == 0) { std::fill(st->stamp.begin(), st->stamp.end(), 0u); st->call = 1; }
  const FplStore ps{dvm_map_store_capacity(points), store_written(points)};
  for (int k = 0; k < n; k++) {
    const int32_t sl = slots[k];
    const std::string w = "row " + std::to_string(k) + " (slot " + std::to_string(sl) + ")";
    if ((uint32_t)sl >= (uint32_t)st->capacity || !st->meta[sl].written) return fail(fn, DVM_ERR_INVALID, w + ": slot outside [0, capacity), never put or removed");
    if (st->stamp[sl] == st->call) return fail(fn, DVM_ERR_INVALID, w + ": slot named twice in one call");
    st->stamp[sl] = st->call;
    const int32_t len = st->meta[sl].n;
    if (len > 0 && !rows[k]) return fail(fn, DVM_ERR_INVALID, w + ": NULL row where the slot holds " + std::to_string(len) + " keypoints");
    int at = -1;
    if (fpl_slots_check(ps, rows[k], len, nullptr, &at))
      return fail(fn, DVM_ERR_INVALID, w + ": entry " + std::to_string(at) + " = " + std::to_string(rows[k][at]) + " is below -1, outside the map store or never written");
  }
  DVM_HIP(hipSetDevice(st->device));
  { const int rc = rows_reserve(fn, st, which); if (rc != DVM_OK) return rc; }
  KfsRowItem* items = reinterpret_cast<KfsRowItem*>(st->hs);
  st->last_h2d = 0;
  for (int done = 0; done < n;) {
    { const int rc = st->staging_free(); if (rc != DVM_OK) return rc; }
    Cursor<kKfsAlign> c{st->hs, st->ds, st->item_bytes};
    int m = 0;
    for (; done + m < n; m++) {
      const int32_t len = st->meta[slots[done + m]].n;
      if (c.used() + pad<kKfsAlign>((size_t)len * 4) > st->stage_bytes) break;   // (the first of a round always fits: a row is smaller than a keyframe)
      items[m] = KfsRowItem{slots[done + m], len, (int32_t)c.used(), 0};
      c.put(rows[done + m], (size_t)len * 4);
    }
    if (m == 0) return fail(fn, DVM_ERR_STATE, "a row exceeds the staging block");
    if (st->read_pending) {                                        // behind the chain kernels that read the rows
      DVM_HIP(hipStreamWaitEvent(st->s, st->read_ev, 0));
      st->read_pending = false;
    }
    DVM_HIP(hipMemcpyAsync(st->ds, st->hs, c.used(), hipMemcpyHostToDevice, st->s));
    st->last_h2d += (int64_t)c.used();
    launch_kfs_rows_set(st->s, reinterpret_cast<const KfsRowItem*>(st->ds), m, st->ds, st->rows_d[which], st->rowlen_d[which], st->row_words);
    { const int rc = hip_check(hipGetLastError(), "k_kfs_rows_set"); if (rc != DVM_OK) return rc; }
    DVM_HIP(hipEventRecord(st->write_ev, st->s));
    st->write_pending = true;
    for (int k = done; k < done + m; k++) row_mark_set(st, which, slots[k], points);
    done += m;
  }
  return DVM_OK;
}

int dvm_keyframe_store_patch_rows(dvm_keyframe_store* st, int which, const dvm_map_store* points, int n_edits, const dvm_kfs_row_edit* edits) {
  static_assert(sizeof(dvm_kfs_row_edit) == sizeof(KfsRowEdit) && sizeof(KfsRowEdit) == 12, "layout");
  const char* fn = "dvm_keyframe_store_patch_rows";
  if (!st || n_edits < 0 || (n_edits && !edits)) return fail(fn, DVM_ERR_INVALID, "missing argument");
  { const int rc = rows_args(fn, st, which, points); if (rc != DVM_OK) return rc; }
  if (n_edits == 0) return DVM_OK;
  const int32_t pcap = dvm_map_store_capacity(points);
  const uint8_t* pw = store_written(points);
  const bool have = st->rows_d[which] != nullptr;
  for (int i = 0; i < n_edits; i++) {
    const dvm_kfs_row_edit& e = edits[i];
    const std::string w = "edit " + std::to_string(i) + " (slot " + std::to_string(e.slot) + ", kp " + std::to_string(e.kp) + ")";
    if ((uint32_t)e.slot >= (uint32_t)st->capacity || !st->meta[e.slot].written) return fail(fn, DVM_ERR_INVALID, w + ": slot outside [0, capacity), never put or removed");
    if ((uint32_t)e.kp >= (uint32_t)st->meta[e.slot].n) return fail(fn, DVM_ERR_INVALID, w + ": kp outside [0, " + std::to_string(st->meta[e.slot].n) + ")");
    if (e.value != -1 && ((uint32_t)e.value >= (uint32_t)pcap || !pw[e.value]))
      return fail(fn, DVM_ERR_INVALID, w + ": value " + std::to_string(e.value) + " is below -1, outside the map store or never written");
    if (have && st->rowmeta[which][e.slot].set && st->rowmeta[which][e.slot].points != points)
      return fail(fn, DVM_ERR_INVALID, w + ": the slot's row names another map store");
  }
  // the last edit of a cell wins: one edit per cell is queued, so no two threads write one word
  std::vector<int32_t>& ord = st->edit_order;
  ord.resize((size_t)n_edits);
  for (int i = 0; i < n_edits; i++) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) {
    return edits[a].slot != edits[b].slot ? edits[a].slot < edits[b].slot : edits[a].kp < edits[b].kp;
  });
  std::vector<KfsRowEdit>& keep = st->edit_keep;
  keep.clear();
  for (int i = 0; i < n_edits; i++) {
    const dvm_kfs_row_edit& e = edits[ord[i]];
    if (i + 1 < n_edits && edits[ord[i + 1]].slot == e.slot && edits[ord[i + 1]].kp == e.kp) continue;
    keep.push_back(KfsRowEdit{e.slot, e.kp, e.value});
  }
  DVM_HIP(hipSetDevice(st->device));
  { const int rc = rows_reserve(fn, st, which); if (rc != DVM_OK) return rc; }
  { const int rc = st->staging_free(); if (rc != DVM_OK) return rc; }
  // a row not yet set opens as n entries of -1 (a new keyframe holds nothing): its items lead the first round
  KfsRowItem* items = reinterpret_cast<KfsRowItem*>(st->hs);
  int n_open = 0;
  for (size_t i = 0; i < keep.size(); i++) {
    const int32_t sl = keep[i].slot;
    if (st->rowmeta[which][sl].set || (i > 0 && keep[i - 1].slot == sl)) continue;   // (keep is sorted by slot)
    items[n_open++] = KfsRowItem{sl, st->meta[sl].n, -1, 0};
  }
  const size_t per_round = (st->stage_bytes - st->item_bytes) / sizeof(KfsRowEdit);
  st->last_h2d = 0;
  for (size_t done = 0; done < keep.size();) {
    if (done) { const int rc = st->staging_free(); if (rc != DVM_OK) return rc; }
    const size_t m = std::min(per_round, keep.size() - done), bytes = m * sizeof(KfsRowEdit);
    std::memcpy(st->hs + st->item_bytes, keep.data() + done, bytes);
    if (st->read_pending) {                                        // behind the chain kernels that read the rows
      DVM_HIP(hipStreamWaitEvent(st->s, st->read_ev, 0));
      st->read_pending = false;
    }
    const bool open = done == 0 && n_open > 0;
    const size_t from = open ? 0 : st->item_bytes;                 // (the items travel only when a row opens)
    DVM_HIP(hipMemcpyAsync(st->ds + from, st->hs + from, st->item_bytes - from + bytes, hipMemcpyHostToDevice, st->s));
    st->last_h2d += (int64_t)(st->item_bytes - from + bytes);
    if (open) launch_kfs_rows_set(st->s, reinterpret_cast<const KfsRowItem*>(st->ds), n_open, st->ds, st->rows_d[which], st->rowlen_d[which], st->row_words);
    launch_kfs_rows_patch(st->s, reinterpret_cast<const KfsRowEdit*>(st->ds + st->item_bytes), (int)m, st->rows_d[which], st->row_words);
    { const int rc = hip_check(hipGetLastError(), "k_kfs_rows_patch"); if (rc != DVM_OK) return rc; }
    DVM_HIP(hipEventRecord(st->write_ev, st->s));
    st->write_pending = true;
    if (open)
      for (int k = 0; k < n_open; k++) row_mark_set(st, which, items[k].slot, points);
    done += m;
  }
  return DVM_OK;
}

int dvm_keyframe_store_debug_read_rows(dvm_keyframe_store* st, int which, int slot, int32_t* out, int cap, int32_t* n_out) {
  const char* fn = "dvm_keyframe_store_debug_read_rows";
  if (!st || !n_out || cap < 0 || (cap && !out)) return fail(fn, DVM_ERR_INVALID, "missing argument");
  if (which != DVM_KFS_ROW_MATCHES && which != DVM_KFS_ROW_OBSERVED) return fail(fn, DVM_ERR_INVALID, "which = " + std::to_string(which));
  if ((uint32_t)slot >= (uint32_t)st->capacity || !st->meta[slot].written)
    return fail(fn, DVM_ERR_INVALID, "slot " + std::to_string(slot) + " outside [0, capacity) or not written");
  *n_out = 0;
  if (!st->rows_d[which]) return DVM_OK;                           // no row of the kind was ever set
  DVM_HIP(hipSetDevice(st->device));
  DVM_HIP(hipStreamSynchronize(st->s));
  st->write_pending = false;
  int32_t len = 0;
  DVM_HIP(hipMemcpy(&len, st->rowlen_d[which] + slot, 4, hipMemcpyDeviceToHost));
  const int32_t want = st->rowmeta[which][slot].set ? st->meta[slot].n : 0;
  if (len != want) return fail(fn, DVM_ERR_STATE, "the slot's device row length " + std::to_string(len) + " is not the host's " + std::to_string(want));
  *n_out = len;
  if (len > cap) return fail(fn, DVM_ERR_CAPACITY, "the row holds " + std::to_string(len) + " entries, the buffer " + std::to_string(cap));
  if (len > 0) DVM_HIP(hipMemcpy(out, st->rows_d[which] + (size_t)slot * st->row_words, (size_t)len * 4, hipMemcpyDeviceToHost));
  return DVM_OK;
}

}  // extern "C"
