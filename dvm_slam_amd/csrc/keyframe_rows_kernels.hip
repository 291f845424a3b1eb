// dvm_slam_amd/csrc/keyframe_rows_kernels.hip -- the kernels of dvm_keyframe_store_set_rows / _patch_rows (include/dvmslam_hip.h, "rows
// beside the keyframes"): a keyframe's GetMapPointMatches() and the inverse of its points' GetObservations() as map-store slots, one int32
// row per slot and kind in a block of their own (keyframe_store.h: KfsRowsView).
//   k_kfs_rows_set    one workgroup per row of a round: the staged row into its place -- 16 bytes per thread and step, both sides at
//                     multiples of 64 bytes --, or n entries of -1 for a row that a patch opens; then the slot's length
//   k_kfs_rows_patch  one thread per edit.  The host has collapsed the call's edits to one per cell, so no two threads write one word.
// No kernel checks a slot, a kp or a length: the host has (keyframe_store.cpp), before anything was queued -- slot < capacity,
// kp < n <= slot_keypoints <= row_words.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keyframe_store.h"

namespace dvm {

__global__ void __launch_bounds__(256) k_kfs_rows_set(const KfsRowItem* __restrict__ items, const uint8_t* __restrict__ stage, int32_t* __restrict__ rows,
                                                      int32_t* __restrict__ len, size_t row_words) {
  const KfsRowItem it = items[blockIdx.x];
  int32_t* dst = rows + (size_t)it.slot * row_words;
  const int n = it.n, n4 = n >> 2;
  if (it.src_off >= 0) {
    const int32_t* src = reinterpret_cast<const int32_t*>(stage + it.src_off);
    int4* d4 = reinterpret_cast<int4*>(dst);
    const int4* s4 = reinterpret_cast<const int4*>(src);
    for (int i = threadIdx.x; i < n4; i += 256) d4[i] = s4[i];
    for (int i = n4 * 4 + threadIdx.x; i < n; i += 256) dst[i] = src[i];
  } else {
    for (int i = threadIdx.x; i < n; i += 256) dst[i] = -1;
  }
  if (threadIdx.x == 0) len[it.slot] = n;
}

__global__ void __launch_bounds__(256) k_kfs_rows_patch(const KfsRowEdit* __restrict__ edits, int n_edits, int32_t* __restrict__ rows, size_t row_words) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_edits) return;
  const KfsRowEdit e = edits[i];
  rows[(size_t)e.slot * row_words + e.kp] = e.value;
}

void launch_kfs_rows_set(hipStream_t s, const KfsRowItem* items, int n_items, const uint8_t* stage, int32_t* rows, int32_t* len, size_t row_words) {
  if (n_items > 0) hipLaunchKernelGGL(k_kfs_rows_set, dim3(n_items), dim3(256), 0, s, items, stage, rows, len, row_words);
}
void launch_kfs_rows_patch(hipStream_t s, const KfsRowEdit* edits, int n_edits, int32_t* rows, size_t row_words) {
  if (n_edits > 0) hipLaunchKernelGGL(k_kfs_rows_patch, dim3((unsigned)((n_edits + 255) / 256)), dim3(256), 0, s, edits, n_edits, rows, row_words);
}

}  // namespace dvm
