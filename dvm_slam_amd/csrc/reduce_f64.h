// dvm_slam_amd/csrc/reduce_f64.h -- fixed-order sums of doubles over a 256-thread workgroup, for the one-workgroup optimisers
// (k_pose_optimize, pose_kernels.hip; k_optimize_sim3, sim3_kernels.hip): the result does not depend on the run.
#pragma once
#include <hip/hip_runtime.h>

namespace dvm {

// Sums of N per-thread doubles over a 256-thread workgroup, THROUGH LDS: every thread parks its values (pitch N + 1), thread
// (q, i) adds the 64 threads of wave q for value i in thread order, then the four wave sums are added -- a fixed order.  The
// alternative, xor-butterflies of __shfl_xor, is ds_bpermute_b32 twice per double and step: 24 cycles of the CU's LDS unit
// each (tools/valu_issue2.hip), 336 of them for 28 values -- 13 us per reduction with four waves sharing the unit.
// park: 256 * (N + 1) doubles, part: 4 * N doubles, out: N doubles (all in LDS; out is valid for every thread on return).
template <int N>
__device__ __forceinline__ void block_sum_lds(const double* v, double* park, double* part, double* out) {
  const int tid = threadIdx.x;
  double* mine = park + (size_t)tid * (N + 1);
#pragma unroll
  for (int i = 0; i < N; i++) mine[i] = v[i];
  __syncthreads();
  if (tid < 4 * N) {
    const int q = tid / N, i = tid - q * N;
    const double* col = park + (size_t)(64 * q) * (N + 1) + i;
    double s = 0;
#pragma unroll 16
    for (int l = 0; l < 64; l++) s += col[(size_t)l * (N + 1)];
    part[q * N + i] = s;
  }
  __syncthreads();
  if (tid < N) out[tid] = (part[tid] + part[N + tid]) + (part[2 * N + tid] + part[3 * N + tid]);
  __syncthreads();
}
// One value over the workgroup in a fixed order: xor-butterfly inside each wave, then the four wave sums in wave order.
// (What the chi2-only evaluation of a trial needs: running the 28-value reduction for it cost 2 us per LM trial.)
__device__ __forceinline__ double block_sum_one(double v, double* part4) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) part4[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = (part4[0] + part4[1]) + (part4[2] + part4[3]);
  __syncthreads();
  return r;
}

}  // namespace dvm
