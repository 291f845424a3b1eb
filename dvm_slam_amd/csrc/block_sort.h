// dvm_slam_amd/csrc/block_sort.h -- what the two ComputeBoW bookkeeping kernels share (k_refkf_bow of track_kernels.hip, k_kfs_dev_bow of
// keyframe_put_kernels.hip): a 1 024-thread workgroup's exclusive scan, its bitonic sort of 64-bit keys in LDS and the walk over the
// runs of equal high words of the sorted keys.  Internal linkage, one copy per translation unit, as when they lived in track_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dvm {
namespace {
// exclusive prefix sum of v over the 1024 threads of a workgroup; *total = the sum.  s_wave: 16 ints of LDS (free again on return)
__device__ int block_scan_1024(int v, int* s_wave, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) s_wave[wv] = x;
  __syncthreads();
  int base = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 16; w++) {
    const int c = s_wave[w];
    if (w < wv) base += c;
    all += c;
  }
  __syncthreads();
  *total = all;
  return base + x - v;
}
// ascending bitonic sort of keys[0 .. P) (P a power of two) by the whole workgroup
__device__ void bitonic_sort(uint64_t* keys, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint64_t a = keys[i], b = keys[ixj];
          if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[ixj] = a; }
        }
      }
      __syncthreads();
    }
  }
}
// the runs of equal (key >> 32) among the first M sorted keys: run r starts at sorted position start and is run number r (ascending).
// Each thread owns a contiguous chunk of positions and calls f(r, start) for the runs that start in it.  Returns the number of runs.
template <class Fn>
__device__ int for_each_run(const uint64_t* keys, int M, int* s_wave, Fn f) {
  const int chunk = (M + 1023) / 1024;
  const int b = min((int)threadIdx.x * chunk, M), e = min(b + chunk, M);
  int heads = 0;
  for (int i = b; i < e; i++) heads += (i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32)) ? 1 : 0;
  int total = 0;
  int r = block_scan_1024(heads, s_wave, &total);
  for (int i = b; i < e; i++)
    if (i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32)) f(r++, i);
  return total;
}
}  // namespace
}  // namespace dvm
