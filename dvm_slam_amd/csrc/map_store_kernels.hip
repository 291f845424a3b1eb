// dvm_slam_amd/csrc/map_store_kernels.hip -- the kernels of dvm_map_store (include/dvmslam_hip.h, "map points resident on the device"): a record
// is 18 dwords, and every kernel moves one dword per thread -- consecutive lanes read and write consecutive dwords of a record, 18 lanes
// to a record.  No kernel checks a slot: the host has (map_store.cpp, track.cpp), before anything was queued.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "map_store.h"

namespace dvm {

namespace {
constexpr int kRecWords = sizeof(LocalPointPod) / 4;
static_assert(sizeof(LocalPointPod) == 72 && sizeof(LocalPointPod) == sizeof(dvm_local_point), "a store record is dvm_local_point");
}  // namespace

// dvm_map_store_update: staged records (page-locked, read in place) to their slots
__global__ void __launch_bounds__(256) k_store_scatter(uint32_t* __restrict__ dst, const int32_t* __restrict__ slots, const uint32_t* __restrict__ src, int n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)n * kRecWords) return;
  const int k = (int)(i / kRecWords), w = (int)(i % kRecWords);
  dst[(size_t)slots[k] * kRecWords + w] = src[i];
}

// dvm_map_store_read: slots back, in the order asked
__global__ void __launch_bounds__(256) k_store_read(const uint32_t* __restrict__ src, const int32_t* __restrict__ slots, uint32_t* __restrict__ dst, int n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)n * kRecWords) return;
  const int k = (int)(i / kRecWords), w = (int)(i % kRecWords);
  dst[i] = src[(size_t)slots[k] * kRecWords + w];
}

// dvm_track_local_map_batch_resident: the device table of the second half from the frames' stores.  blockIdx.y = frame, blockIdx.x walks
// its table; a skipped frame has n = 0 and reads nothing (its store pointer is not touched).
__global__ void __launch_bounds__(256) k_store_gather(StoreGather G, uint32_t* __restrict__ dst) {
  const int b = blockIdx.y;
  const int n = G.per_frame[b].n;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)n * kRecWords) return;
  const int k = (int)(i / kRecWords), w = (int)(i % kRecWords);
  const size_t o = (size_t)G.qoff[b];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(G.stores[b]);
  dst[(o + k) * kRecWords + w] = src[(size_t)G.slots[o + k] * kRecWords + w];
}

// dvm_ba_resident_commit: blockIdx.y = range, a lane per word of the eight geometry words; the other ten words of a record (desc, n_obs,
// bad) and the records of points whose state is not 0 are never written
__global__ void __launch_bounds__(256) k_store_commit(uint32_t* __restrict__ dst, StoreCommit C) {
  const StoreCommitRange& R = C.r[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= R.n * 8) return;
  const int k = i >> 3, w = i & 7;
  if (R.state[k] != 0) return;
  dst[(size_t)R.slot[k] * kRecWords + w] = reinterpret_cast<const uint32_t*>(R.geom)[i];
}

void launch_store_commit(hipStream_t s, LocalPointPod* dst, const StoreCommit& C, int n_ranges, int span_max) {
  if (n_ranges < 1 || span_max < 1) return;
  hipLaunchKernelGGL(k_store_commit, dim3((unsigned)(((int64_t)span_max * 8 + 255) / 256), (unsigned)n_ranges), dim3(256), 0, s, reinterpret_cast<uint32_t*>(dst), C);
}
void launch_store_scatter(hipStream_t s, LocalPointPod* dst, const int32_t* slots, const LocalPointPod* src, int n) {
  if (n < 1) return;
  const unsigned blocks = (unsigned)(((int64_t)n * kRecWords + 255) / 256);
  hipLaunchKernelGGL(k_store_scatter, dim3(blocks), dim3(256), 0, s, reinterpret_cast<uint32_t*>(dst), slots, reinterpret_cast<const uint32_t*>(src), n);
}
void launch_store_read(hipStream_t s, const LocalPointPod* src, const int32_t* slots, LocalPointPod* dst, int n) {
  if (n < 1) return;
  const unsigned blocks = (unsigned)(((int64_t)n * kRecWords + 255) / 256);
  hipLaunchKernelGGL(k_store_read, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(src), slots, reinterpret_cast<uint32_t*>(dst), n);
}
void launch_store_gather(hipStream_t s, const StoreGather& G, LocalPointPod* dst, int count, int span_max) {
  if (count < 1 || span_max < 1) return;
  const unsigned bx = (unsigned)(((int64_t)span_max * kRecWords + 255) / 256);
  hipLaunchKernelGGL(k_store_gather, dim3(bx, (unsigned)count), dim3(256), 0, s, G, reinterpret_cast<uint32_t*>(dst));
}

}  // namespace dvm
