// dvm_slam_amd/csrc/keyframe_store_kernels.hip -- the kernel of dvm_keyframe_store_put (include/dvmslam_hip.h, "keyframes resident on the
// device"): k_kfs_put, one 1 024-thread workgroup per keyframe of a put round.  It moves the keyframe's staged arrays into its slot -- 16
// bytes per thread and step, consecutive lanes on consecutive addresses, both sides at multiples of 64 bytes -- and builds the slot's
// feature grid with frame_build_block (proj_device.h), the function k_frame_build and k_ft_build call: a resident grid has the order a
// per-call dvm_fuse_targets_set produces.  The grid is built FROM THE STAGED keypoints and descriptors, which nothing writes during the
// launch, so the build needs no ordering against the workgroup's own copy.  The kernel checks no count: the host has (keyframe_store.cpp),
// before anything was queued -- n, fv_n and the features at most slot_keypoints, the tables at most 64 entries.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keyframe_store.h"
#include "proj_device.h"

namespace dvm {

namespace {
// bytes: a multiple of 4; dst and src: multiples of 16
__device__ __forceinline__ void kfs_move(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, size_t bytes) {
  const size_t n16 = bytes >> 4, n4 = bytes >> 2;
  uint4* d = reinterpret_cast<uint4*>(dst);
  const uint4* s = reinterpret_cast<const uint4*>(src);
  for (size_t i = threadIdx.x; i < n16; i += 1024) d[i] = s[i];
  uint32_t* dw = reinterpret_cast<uint32_t*>(dst);
  const uint32_t* sw = reinterpret_cast<const uint32_t*>(src);
  for (size_t i = n16 * 4 + threadIdx.x; i < n4; i += 1024) dw[i] = sw[i];
}
}  // namespace

__global__ void __launch_bounds__(1024) k_kfs_put(const KfsPutItem* __restrict__ items, KfSlotLayout L) {
  const KfsPutItem it = items[blockIdx.x];
  const size_t n = (size_t)it.n, fv_n = (size_t)it.fv_n, nf = (size_t)it.n_feat, nl = (size_t)it.n_levels;
  const uint8_t* src = it.src;
  const uint8_t* s_kps = src;
  const uint8_t* s_desc = s_kps + kfs_pad(n * kKfsKeypointBytes);
  const uint8_t* s_node = s_desc + kfs_pad(n * 32);
  const uint8_t* s_off = s_node + kfs_pad(fv_n * 4);
  const size_t off_bytes = fv_n ? (fv_n + 1) * 4 : 0;
  const uint8_t* s_feat = s_off + kfs_pad(off_bytes);
  const uint8_t* s_sf = s_feat + kfs_pad(nf * 4);
  const uint8_t* s_sigma2 = s_sf + kfs_pad(nl * 4);
  const uint8_t* s_inv = s_sigma2 + kfs_pad(nl * 4);
  uint8_t* slot = it.slot;
  kfs_move(slot + L.kps, s_kps, n * kKfsKeypointBytes);
  kfs_move(slot + L.desc, s_desc, n * 32);
  kfs_move(slot + L.fv_node, s_node, fv_n * 4);
  kfs_move(slot + L.fv_off, s_off, off_bytes);
  kfs_move(slot + L.fv_feat, s_feat, nf * 4);
  kfs_move(slot + L.sf, s_sf, nl * 4);
  kfs_move(slot + L.sigma2, s_sigma2, nl * 4);
  kfs_move(slot + L.inv_sigma2, s_inv, nl * 4);

  FrameView F;
  F.skp = reinterpret_cast<float4*>(slot + L.skp);
  F.sidx = reinterpret_cast<int32_t*>(slot + L.sidx);
  F.sdesc = slot + L.sdesc;
  F.cell_start = reinterpret_cast<int32_t*>(slot + L.cell_start);
  F.n_sorted = reinterpret_cast<int32_t*>(slot + L.counters);
  F.n_total = F.n_sorted + 1;
  F.n_overflow = F.n_sorted + 2;
  F.cap = it.n;
  F.minX = it.minX; F.minY = it.minY; F.wInv = it.wInv; F.hInv = it.hInv;
  frame_build_block(reinterpret_cast<const dvm_keypoint_pod*>(s_kps), s_desc, it.n, F);
}

void launch_kfs_put(hipStream_t s, const KfsPutItem* items, int n_items, const KfSlotLayout& L) {
  static_assert(sizeof(dvm_keypoint_pod) == kKfsKeypointBytes && kCellStartStride == (int)kKfsCellStart, "kf_store_layout.h restates these");
  if (n_items > 0) hipLaunchKernelGGL(k_kfs_put, dim3(n_items), dim3(1024), 0, s, items, L);
}

}  // namespace dvm
