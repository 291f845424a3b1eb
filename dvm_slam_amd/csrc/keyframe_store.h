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
int kfs_read_begin(const dvm_keyframe_store* st, hipStream_t s);
int kfs_read_end(const dvm_keyframe_store* st, hipStream_t s);

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

}  // namespace dvm
