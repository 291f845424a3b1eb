// dvm_slam_amd/csrc/keyframe_store.h -- dvm_keyframe_store as the chains see it (keyframe_store.cpp), and the launcher of
// keyframe_store_kernels.hip.
//
// A chain that reads slots asks for each slot's view on the host (kfs_slot_view: false for a slot outside the store, never written or
// removed), fills its own device structs (FtTargetDev, NpKfDev) with the view's pointers, then brackets the kernels that read them:
//   kfs_read_begin(st, s)   s waits for the store's last queued put
//   ... the reading kernels on s ...
//   kfs_read_end(st, s)     the store's next put waits for what s holds so far
// A view's pointers stay valid for the store's life (the block never moves); its CONTENT is the keyframe of generation `gen`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dvmslam_hip.h"
#include "kf_store_layout.h"
#include "match_kernels.h"   // FrameView, dvm_keypoint_pod

namespace dvm {

struct KfSlotView {
  const dvm_keypoint_pod* kps;   // [n] as put
  const uint8_t* desc;           // [n][32]
  const int32_t *fv_node, *fv_off, *fv_feat;
  const float *sf, *sigma2, *inv_sigma2;
  FrameView F;                   // the slot's grid (cap = n, the bounds' minX, minY, wInv, hInv)
  int32_t n, fv_n, n_feat, n_levels;
  float fx, fy, cx, cy, min_x, max_x, min_y, max_y, log_scale_factor;
  uint32_t gen;
  bool fv_once;                  // every feature lies in at most one node of the FeatureVector (fv_once.h)
};
int kfs_device(const dvm_keyframe_store* st);
bool kfs_slot_view(const dvm_keyframe_store* st, int32_t slot, KfSlotView* v);
// the slot's generation now (put and remove bump it); 0 for a slot outside the store
uint32_t kfs_generation(const dvm_keyframe_store* st, int32_t slot);
// the store's block for a kernel that forms slot addresses itself: slot sl's arrays begin at base + sl * stride + kps / desc / sf
struct KfsBlockView { const uint8_t* base; size_t stride, kps, desc, sf; };
KfsBlockView kfs_block_view(const dvm_keyframe_store* st);
int kfs_read_begin(const dvm_keyframe_store* st, hipStream_t s);
int kfs_read_end(const dvm_keyframe_store* st, hipStream_t s);

// ---- the rows beside the keyframes (dvm_keyframe_store_set_rows / _patch_rows; keyframe_rows_kernels.hip): per kind one device block of
// [capacity] rows of row_words int32 each (slot_keypoints rounded up to 16: a row starts on 64 bytes) and one length per slot -- the
// slot's n while the row is set, 0 otherwise -- which a kernel that walks the whole store reads instead of a host-made list.
// rows == nullptr: no row of the kind was ever set (every length counts as 0).
struct KfsRowsView { const int32_t* rows; const int32_t* len; size_t row_words; };
KfsRowsView kfs_rows_view(const dvm_keyframe_store* st, int which);
// slot's row of the kind as the host knows it: false for a slot outside the store, never put, removed, or whose row is not set;
// *n: its length, *points: the map store its values were checked against
bool kfs_row_info(const dvm_keyframe_store* st, int which, int32_t slot, int32_t* n, const dvm_map_store** points);
// every row of the kind that is set names `points` (true for none set): what lets a kernel walk ALL rows against one map store's tables
bool kfs_rows_all_name(const dvm_keyframe_store* st, int which, const dvm_map_store* points);
int kfs_capacity(const dvm_keyframe_store* st);

// one row of a set round: staged at src_off bytes of the staging block's device twin (src_off < 0: no staged row -- the row becomes n
// entries of -1, what patch_rows does to a row not yet set)
struct KfsRowItem { int32_t slot, n, src_off, pad; };
struct KfsRowEdit { int32_t slot, kp, value; };   // == dvm_kfs_row_edit
// one 256-thread workgroup per item: the staged row into rows + slot * row_words, len[slot] = n
void launch_kfs_rows_set(hipStream_t s, const KfsRowItem* items, int n_items, const uint8_t* stage, int32_t* rows, int32_t* len, size_t row_words);
// one thread per edit (the host left one edit per cell): rows[slot * row_words + kp] = value
void launch_kfs_rows_patch(hipStream_t s, const KfsRowEdit* edits, int n_edits, int32_t* rows, size_t row_words);

// one keyframe of a put round: its staged arrays (the device copy of the staging block: kps, desc, fv_node, fv_off, fv_feat, sf, sigma2,
// inv_sigma2 back to back, each rounded up to 64 bytes) and its slot
struct KfsPutItem {
  const uint8_t* src;
  uint8_t* slot;
  int32_t n, fv_n, n_feat, n_levels;
  float minX, minY, wInv, hInv;
};
// one workgroup per item: the staged arrays to the slot's (layout L), and the slot's grid by frame_build_block
void launch_kfs_put(hipStream_t s, const KfsPutItem* items, int n_items, const KfSlotLayout& L);

// ---- dvm_keyframe_store_put_device: the keyframe's arrays are in device memory already (keyframe_put_kernels.hip)
// The one upload of a call: this head, then one KfsDevItem per keyframe.
constexpr int32_t kKfsDevNoFlag = 0x7FFFFFFF;
struct KfsDevHead {
  int32_t flag;          // kKfsDevNoFlag, or (keyframe << 1 | what): the first keyframe of the call the device refuses; what = 0: its
  int32_t pad[15];       // count exceeds slot_keypoints, 1: an octave outside [0, n_levels).  Raised by k_kfs_dev_check (atomicMin)
};
struct KfsDevItem {
  const dvm_keypoint_pod* kps;     // the caller's arrays (4-byte aligned at least)
  const uint8_t* desc;
  const int32_t* d_n;              // the device count, or null: cap is the count
  uint8_t* slot;
  int32_t cap, n_levels;
  float minX, minY, wInv, hInv;
  int32_t count;                   // written by k_kfs_dev_check: the keyframe's keypoints (0 for a keyframe it refuses); the transform's d_n
  int32_t pad;
  float sf[kKfsLevels], sigma2[kKfsLevels], inv_sigma2[kKfsLevels];
};                                 // 832 bytes: everything that travels up per keyframe
// what the host reads of one keyframe after the call's one wait (mapped memory): the counts, then the BowVector and a copy of the
// FeatureVector, each array sized for slot_keypoints
struct KfsDevRes { int32_t n, n_bow, n_fv, n_feat, flag, pad[3]; };
struct KfsDevOut {
  KfsDevRes* res;                  // [1]
  int32_t* bow_ids; double* bow_vals; int32_t *fv_node, *fv_off, *fv_feat;   // [K], [K], [K], [K + 1], [K]
};
// the scratch of a round of keyframes: k_vocab_transform's per-feature results, keyframe r of the round at r * K
struct KfsDevScratch { int32_t* word; int32_t* node; double* w; };
// one workgroup per keyframe of the call: items[k].count, res[k].n, the call's flag
void launch_kfs_dev_check(hipStream_t s, KfsDevHead* head, KfsDevItem* items, int n_items, int K, KfsDevRes* res, size_t res_stride);
// one 1 024-thread workgroup per keyframe of a round (items first .. first + m): ComputeBoW's bookkeeping, the FeatureVector into the
// slot, the BowVector and a copy of the FeatureVector to out0 + r * out_stride bytes; false: the sort's LDS cannot be had
bool launch_kfs_dev_bow(hipStream_t s, const KfsDevHead* head, const KfsDevItem* items, int first, int m, int K, const KfsDevScratch& W,
                        const KfSlotLayout& L, const KfsDevOut& out0, size_t out_stride);
// one 1 024-thread workgroup per keyframe of a round: keypoints, descriptors and tables into the slot, the slot's grid, res[k].flag
void launch_kfs_dev_put(hipStream_t s, const KfsDevHead* head, const KfsDevItem* items, int first, int m, const KfSlotLayout& L,
                        KfsDevRes* res0, size_t res_stride);

// dvm_keyframe_store_put_device behind its name (track.cpp: dvm_keyframe_store_put_tracked calls it on the tracker's frames)
int kfs_put_device_run(const char* fn, dvm_keyframe_store* st, const dvm_vocab* voc, int levelsup, hipStream_t src, int n, const int32_t* slots,
                       const dvm_kfs_device_keyframe* kfs, dvm_kfs_bow_out* outs);

}  // namespace dvm
