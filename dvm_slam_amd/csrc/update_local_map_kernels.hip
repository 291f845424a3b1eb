// dvm_slam_amd/csrc/update_local_map_kernels.hip -- Tracking::UpdateLocalMap's two graph walks (reference src/Tracking.cc:3117-3181) as list
// intersections over the rows a dvm_keyframe_store keeps beside its keyframes (dvm_update_local_map_keyframes / _points,
// include/dvmslam_hip.h).  Every launch is batched over the frames of a tick: blockIdx.y is the frame, and a frame reads its own stores
// through its parameter block (UlmFrameDev).
//   the votes (UpdateLocalKeyFrames, :3145-3181)
//     k_ulm_mult        mult[s] += 1 per frame keypoint that holds the non-bad point s (integer atomicAdd: the sum does not depend on the
//                       order of arrival); frame_bad
//     k_ulm_votes       one wavefront per (frame, keyframe slot): the slot's OBSERVED row in 16-byte loads (a row starts on 64 bytes),
//                       mult gathered per entry, the sum reduced across the wave, one word written
//     k_ulm_mult_reset  the frame's entries put mult back to 0
//   the local points (UpdateLocalPoints, :3117-3141), in the form of k_ft_cand_* (fuse_points_kernels.hip)
//     k_ulm_mark        first[s] = the lowest key k * (padded row length) + kp among the non-bad entries of the named MATCHES rows that
//                       name s (integer atomicMin)
//     k_ulm_count / k_ulm_scan / k_ulm_write   the entries that are the first of their slot, counted per workgroup, scanned, written in
//                       key order; the write records pos[s]
//     k_ulm_frame_mp    frame_mp[i] = pos of the point keypoint i holds; n_outside
//     k_ulm_points_reset  the rows' entries put first and pos back to idle
// No workgroup waits on another.  No kernel checks a slot, a row length or a list entry: the host has (update_local_map_lists.h; the rows'
// values at set_rows / patch_rows time), before anything was queued.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "update_local_map_kernels.h"
#include "update_local_map_lists.h"

namespace dvm {

namespace {
constexpr int kRecWords = 18;    // dvm_local_point in words; bad is word 17
constexpr int kBadWord = 17;
__device__ __forceinline__ bool ulm_bad(const UlmFrameDev& F, int32_t sl) { return F.records[(size_t)sl * kRecWords + kBadWord] != 0u; }
}  // namespace

// ---- the votes
__global__ void __launch_bounds__(256) k_ulm_mult(UlmArgs A) {
  const int b = blockIdx.y;
  const UlmFrameDev F = A.frames[b];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= F.n) return;
  const int32_t sl = A.lists[F.mp_off + i];
  const bool bad = sl >= 0 && ulm_bad(F, sl);
  A.frame_bad[(size_t)b * A.n_pad + i] = bad ? 1 : 0;
  if (sl >= 0 && !bad) atomicAdd(&A.mult[(size_t)b * A.map_capacity + sl], 1);
}

__global__ void __launch_bounds__(256) k_ulm_votes(UlmArgs A) {
  const int b = blockIdx.y;
  const UlmFrameDev F = A.frames[b];
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);   // j: wave-uniform
  if (j >= F.kf_capacity) return;
  const int len = F.rows ? F.len[j] : 0;
  const int4* row = reinterpret_cast<const int4*>(F.rows + (size_t)j * F.row_words);
  const int32_t* mult = A.mult + (size_t)b * A.map_capacity;
  int sum = 0;
  for (int i = lane * 4; i < len; i += 256) {        // (i + 3 < row_words: a row's words are a multiple of 16)
    const int4 v = row[i >> 2];
    if (v.x >= 0) sum += mult[v.x];
    if (i + 1 < len && v.y >= 0) sum += mult[v.y];
    if (i + 2 < len && v.z >= 0) sum += mult[v.z];
    if (i + 3 < len && v.w >= 0) sum += mult[v.w];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
  if (lane == 0) A.votes[(size_t)b * A.kf_capacity_res + j] = sum;
}

__global__ void __launch_bounds__(256) k_ulm_mult_reset(UlmArgs A) {
  const int b = blockIdx.y;
  const UlmFrameDev F = A.frames[b];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= F.n) return;
  const int32_t sl = A.lists[F.mp_off + i];
  if (sl >= 0) A.mult[(size_t)b * A.map_capacity + sl] = 0;
}

// ---- the local points.  Workgroup x of frame b takes entries [blk * 256, blk * 256 + 256) of named keyframe k's row, x = k * row_blocks + blk;
// the entry's key is x * 256 + lane: ascending in (keyframe, keypoint) order
namespace {
// the slot entry (x, tid) names, or -1: beyond the frame's keyframes, beyond the row, or no point
__device__ __forceinline__ int32_t ulm_entry(const UlmArgs& A, const UlmFrameDev& F, int x, int tid) {
  const int k = x / A.row_blocks;
  if (k >= F.n_kfs) return -1;
  const int kp = (x - k * A.row_blocks) * kUlmBlock + tid;
  const int32_t j = A.lists[F.kf_off + k];
  return kp < F.len[j] ? F.rows[(size_t)j * F.row_words + kp] : -1;
}
// the entry is taken: the first to name its slot (only a non-bad entry ever reaches first[])
__device__ __forceinline__ bool ulm_taken(const UlmArgs& A, int b, int x, int tid, int32_t sl) {
  return sl >= 0 && A.first[(size_t)b * A.map_capacity + sl] == x * kUlmBlock + tid;
}
}  // namespace

__global__ void __launch_bounds__(256) k_ulm_mark(UlmArgs A) {
  const int b = blockIdx.y;
  const UlmFrameDev F = A.frames[b];
  const int32_t sl = ulm_entry(A, F, blockIdx.x, threadIdx.x);
  if (sl >= 0 && !ulm_bad(F, sl)) atomicMin(&A.first[(size_t)b * A.map_capacity + sl], (int32_t)(blockIdx.x * kUlmBlock + threadIdx.x));
}

__global__ void __launch_bounds__(256) k_ulm_count(UlmArgs A) {
  __shared__ int s_wave[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const UlmFrameDev F = A.frames[b];
  if ((int)blockIdx.x >= F.n_kfs * A.row_blocks) return;         // (uniform: the scan reads the frame's own workgroups only)
  const int32_t sl = ulm_entry(A, F, blockIdx.x, tid);
  const int c = __popcll(__ballot(ulm_taken(A, b, blockIdx.x, tid, sl)));
  if ((tid & 63) == 0) s_wave[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) A.cnt[(size_t)b * (A.blocks_max + 1) + blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// off[x] = cnt[0] + .. + cnt[x - 1], off[T] = n_local: one workgroup per frame, rounds of 256 workgroups (the form of k_ft_hit_scan)
__global__ void __launch_bounds__(256) k_ulm_scan(UlmArgs A) {
  __shared__ int s_wave[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int T = A.frames[b].n_kfs * A.row_blocks;
  const int32_t* cnt = A.cnt + (size_t)b * (A.blocks_max + 1);
  int32_t* off = A.off + (size_t)b * (A.blocks_max + 1);
  int base = 0;
  for (int c0 = 0; c0 < T; c0 += 256) {
    const int i = c0 + tid;
    const int v = i < T ? cnt[i] : 0;
    int x = v;                                // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    if (lane == 63) s_wave[wv] = x;
    __syncthreads();
    int pre = base + x - v, total = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const int cw = s_wave[w];
      if (w < wv) pre += cw;
      total += cw;
    }
    if (i < T) off[i] = pre;
    base += total;
    __syncthreads();
  }
  if (tid == 0) { off[T] = base; A.counts[2 * b] = base; }
}

__global__ void __launch_bounds__(256) k_ulm_write(UlmArgs A) {
  __shared__ int s_wave[4];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const UlmFrameDev F = A.frames[b];
  if ((int)blockIdx.x >= F.n_kfs * A.row_blocks) return;
  const int32_t sl = ulm_entry(A, F, blockIdx.x, tid);
  const bool is = ulm_taken(A, b, blockIdx.x, tid, sl);
  const unsigned long long m = __ballot(is);
  if (lane == 0) s_wave[wv] = __popcll(m);
  __syncthreads();
  int pos = A.off[(size_t)b * (A.blocks_max + 1) + blockIdx.x] + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
#pragma unroll
  for (int w = 0; w < 4; w++)
    if (w < wv) pos += s_wave[w];
  if (!is) return;
  A.pos[(size_t)b * A.map_capacity + sl] = pos;                  // (pos < map_capacity: every taken entry names another slot)
  if (pos < F.local_cap) A.local[(size_t)b * A.map_capacity + pos] = sl;
}

// one workgroup per frame walks the frame's list: no atomic on the count
__global__ void __launch_bounds__(256) k_ulm_frame_mp(UlmArgs A) {
  __shared__ int s_wave[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const UlmFrameDev F = A.frames[b];
  const int32_t* pos = A.pos + (size_t)b * A.map_capacity;
  int outside = 0;                              // wave-uniform
  for (int c0 = 0; c0 < F.n; c0 += 256) {
    const int i = c0 + tid;
    bool out = false;
    if (i < F.n) {
      const int32_t sl = A.lists[F.mp_off + i];
      int32_t p = -1;
      if (sl >= 0 && !ulm_bad(F, sl)) {
        p = pos[sl];
        out = p < 0;
      }
      A.frame_mp[(size_t)b * A.n_pad + i] = p;
    }
    outside += __popcll(__ballot(out));
  }
  if ((tid & 63) == 0) s_wave[tid >> 6] = outside;
  __syncthreads();
  if (tid == 0) A.counts[2 * b + 1] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

__global__ void __launch_bounds__(256) k_ulm_points_reset(UlmArgs A) {
  const int b = blockIdx.y;
  const UlmFrameDev F = A.frames[b];
  const int32_t sl = ulm_entry(A, F, blockIdx.x, threadIdx.x);
  if (sl < 0) return;
  A.first[(size_t)b * A.map_capacity + sl] = kUlmFirstIdle;
  A.pos[(size_t)b * A.map_capacity + sl] = -1;
}

void launch_ulm_keyframes(hipStream_t s, const UlmArgs& A, int count, int n_max, int c_max) {
  if (count < 1) return;
  const dim3 per_entry((unsigned)((n_max + 255) / 256), (unsigned)count);
  if (n_max > 0) hipLaunchKernelGGL(k_ulm_mult, per_entry, dim3(256), 0, s, A);
  hipLaunchKernelGGL(k_ulm_votes, dim3((unsigned)((c_max + 3) / 4), (unsigned)count), dim3(256), 0, s, A);
  if (n_max > 0) hipLaunchKernelGGL(k_ulm_mult_reset, per_entry, dim3(256), 0, s, A);
}

void launch_ulm_points(hipStream_t s, const UlmArgs& A, int count, int kfs_max) {
  if (count < 1) return;
  const dim3 per_block((unsigned)(kfs_max * A.row_blocks), (unsigned)count);
  if (kfs_max > 0) {
    hipLaunchKernelGGL(k_ulm_mark, per_block, dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_ulm_count, per_block, dim3(256), 0, s, A);
  }
  hipLaunchKernelGGL(k_ulm_scan, dim3((unsigned)count), dim3(256), 0, s, A);
  if (kfs_max > 0) hipLaunchKernelGGL(k_ulm_write, per_block, dim3(256), 0, s, A);
  hipLaunchKernelGGL(k_ulm_frame_mp, dim3((unsigned)count), dim3(256), 0, s, A);
  if (kfs_max > 0) hipLaunchKernelGGL(k_ulm_points_reset, per_block, dim3(256), 0, s, A);
}

}  // namespace dvm
