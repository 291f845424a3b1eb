// dvm_slam_amd/csrc/fuse_points_kernels.hip -- the point table of a Fuse run from the records of a dvm_map_store (dvm_fuse_targets_run[_hits]_resident,
// dvm_fuse_targets_run_hits_candidates; include/dvmslam_hip.h, launchers in fuse_targets_kernels.h):
//   k_ft_gather       records[slot[k]] into the separate arrays k_ft_search reads, plus the row's valid flag (isBad() read here)
//   k_ft_cand_*       vpFuseCandidates of LocalMapping::SearchInNeighbors (reference src/LocalMapping.cc:826-846): the union of the target
//                     keyframes' map points, not bad, each once, in order of first occurrence -- mark (an integer atomicMin of the flat
//                     index per slot), count per block, scan (k_ft_hit_scan), stable write, reset
// A record is 18 dwords, and like the kernels of map_store_kernels.hip the gather moves one dword per thread: consecutive lanes read
// consecutive dwords of a record and write consecutive dwords of an array.  No kernel checks a slot: the host has (fuse_points_lists.h),
// before anything was queued.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fuse_targets_kernels.h"

namespace dvm {

namespace {
constexpr int kRecWords = 18;    // dvm_local_point: pos 0-2, normal 3-5, min_dist 6, max_dist 7, desc 8-15, n_obs 16, bad 17
constexpr int kBadWord = 17;
}  // namespace

__global__ void __launch_bounds__(256) k_ft_gather(FtGather G) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)G.n * kRecWords) return;
  const int k = (int)(i / kRecWords), w = (int)(i % kRecWords);
  if (w == 16) return;                                       // (Observations(): no array of the search)
  const int32_t sl = !G.n_live || k < *G.n_live ? G.slot[k] : -1;
  if (sl < 0) {
    if (w == kBadWord) G.valid[k] = 0;
    return;
  }
  const uint32_t v = G.records[(size_t)sl * kRecWords + w];
  if (w < 3) G.pos[3 * (size_t)k + w] = v;
  else if (w < 6) G.normal[3 * (size_t)k + (w - 3)] = v;
  else if (w == 6) G.min_dist[k] = v;
  else if (w == 7) G.max_dist[k] = v;
  else if (w < 16) G.desc[8 * (size_t)k + (w - 8)] = v;
  else G.valid[k] = v == 0u && (!G.valid_in || G.valid_in[k] != 0) && (!G.mark || G.mark[sl] == 0) ? 1 : 0;
}

// first[s] = the lowest flat index among the non-bad entries naming slot s; the threads behind the entries mark the exclude list's slots
__global__ void __launch_bounds__(256) k_ft_cand_mark(FtCand C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < C.n_entries) {
    const int32_t sl = C.entry[i];
    if (sl >= 0 && C.records[(size_t)sl * kRecWords + kBadWord] == 0u) atomicMin(&C.first[sl], i);
  } else if (i - C.n_entries < C.n_exclude) {
    const int32_t sl = C.exclude[i - C.n_entries];
    if (sl >= 0) C.mark[sl] = 1;
  }
}
// entry i is a candidate: it names a slot and is the first entry to name it (only a non-bad entry ever reaches first[])
__device__ __forceinline__ bool ft_is_cand(const FtCand& C, int i, int32_t* sl) {
  *sl = i < C.n_entries ? C.entry[i] : -1;
  return *sl >= 0 && C.first[*sl] == i;
}
// ---- the stable compaction in the form of k_ft_hit_*: a block per 256 entries counts, k_ft_hit_scan scans the blocks, a block writes
__global__ void __launch_bounds__(256) k_ft_cand_count(FtCand C, int32_t* __restrict__ cnt) {
  __shared__ int s_wave[4];
  const int tid = threadIdx.x;
  int32_t sl;
  const int c = __popcll(__ballot(ft_is_cand(C, blockIdx.x * 256 + tid, &sl)));
  if ((tid & 63) == 0) s_wave[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) cnt[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}
// cand[off[block] ..): the block's candidates in flat order; cand_out (may be mapped host memory) takes the positions below cap
__global__ void __launch_bounds__(256) k_ft_cand_write(FtCand C, const int32_t* __restrict__ off, int32_t* __restrict__ cand, int32_t* __restrict__ cand_out, int cap) {
  __shared__ int s_wave[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int32_t sl;
  const bool is = ft_is_cand(C, blockIdx.x * 256 + tid, &sl);
  const unsigned long long m = __ballot(is);
  if (lane == 0) s_wave[wv] = __popcll(m);
  __syncthreads();
  int pos = off[blockIdx.x] + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
#pragma unroll
  for (int w = 0; w < 4; w++)
    if (w < wv) pos += s_wave[w];
  if (!is) return;
  cand[pos] = sl;
  if (pos < cap) cand_out[pos] = sl;
}
__global__ void __launch_bounds__(256) k_ft_cand_reset(FtCand C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < C.n_entries) {
    const int32_t sl = C.entry[i];
    if (sl >= 0) C.first[sl] = kFtFirstIdle;
  } else if (i - C.n_entries < C.n_exclude) {
    const int32_t sl = C.exclude[i - C.n_entries];
    if (sl >= 0) C.mark[sl] = 0;
  }
}

void launch_ft_gather(hipStream_t s, const FtGather& G) {
  if (G.n < 1) return;
  hipLaunchKernelGGL(k_ft_gather, dim3((unsigned)(((int64_t)G.n * kRecWords + 255) / 256)), dim3(256), 0, s, G);
}
void launch_ft_candidates(hipStream_t s, const FtCand& C, int32_t* cnt, int32_t* off, int32_t* off_out, int32_t* cand, int32_t* cand_out, int cap) {
  if (C.n_entries < 1) return;
  const unsigned blocks = (unsigned)((C.n_entries + 255) / 256), all = (unsigned)(((int64_t)C.n_entries + C.n_exclude + 255) / 256);
  hipLaunchKernelGGL(k_ft_cand_mark, dim3(all), dim3(256), 0, s, C);
  hipLaunchKernelGGL(k_ft_cand_count, dim3(blocks), dim3(256), 0, s, C, cnt);
  launch_ft_scan(s, cnt, (int)blocks, off, off_out);
  hipLaunchKernelGGL(k_ft_cand_write, dim3(blocks), dim3(256), 0, s, C, off, cand, cand_out, cap);
}
void launch_ft_cand_reset(hipStream_t s, const FtCand& C) {
  if (C.n_entries < 1) return;
  hipLaunchKernelGGL(k_ft_cand_reset, dim3((unsigned)(((int64_t)C.n_entries + C.n_exclude + 255) / 256)), dim3(256), 0, s, C);
}

}  // namespace dvm
