// dvm_slam_amd/csrc/fuse_targets_kernels.hip -- the search part of ORBmatcher::Fuse(pKF, vpMapPoints, th) (reference src/ORBmatcher.cc:
// 1089-1210) for ALL target keyframes of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:812-821) at once (dvm_fuse_targets,
// include/dvmslam_hip.h):
//   k_ft_build    the feature grids of all targets in one launch, one workgroup per target, into back-to-back spans
//   k_ft_search   one DPP row (16 lanes) per (target, map point): the projection gates and the window search of k_project_search[_kb8] with
//                 the 5.99 gate -- or without it: Fuse(pKF, Scw, ...) of LoopClosing::SearchAndFuse (:1256-1327) --, then Fuse's acceptance
//                 (best distance <= TH_LOW); one instantiation per camera model, one launch per model present among the targets
//   k_ft_hit_*    the hits of the dense rows, target by target (dvm_fuse_targets_run_hits)
// Both kernels call the device functions the single calls run (proj_device.h), so entry (t, i) is dvm_project_search[_cam] on target t alone.
// What the sequential loop of the reference changes between two targets -- isBad(), IsInKeyFrame(), a survivor's descriptor -- never
// reaches these kernels: the caller masks or repeats rows (the skip array of a run).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fuse_targets_kernels.h"
#include "proj_device.h"

namespace dvm {

__global__ void __launch_bounds__(1024) k_ft_build(const FtTargetDev* __restrict__ targets) {
  const FtTargetDev& T = targets[blockIdx.x];
  frame_build_block(T.kps, T.desc, T.n, T.F);
}

// target = order[blockIdx.y]: the launch's part of the target list, all of camera MODEL (project_row<MODEL>; T.kb8 = mvParameters for
// KannalaBrandt8, unused for the pinhole camera).  T.inv_sigma2 == null is the ungated form: project_row skips the gate on a null table.
// A row whose point is masked (valid[i] == 0 or skip[t * n + i] != 0) writes "none" and leaves before anything is read.
template <int MODEL>
__global__ void __launch_bounds__(256) k_ft_search(const FtTargetDev* __restrict__ targets, const int32_t* __restrict__ order, FtPoints P, float th,
                                                   int32_t* __restrict__ best_idx, int32_t* __restrict__ best_dist) {
  const int lane = threadIdx.x & 15;
  const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
  if (i >= P.n) return;
  const int t = order[blockIdx.y];
  const size_t e = (size_t)t * P.n + i;
  if ((P.valid && P.valid[i] == 0) || (P.skip && P.skip[e] != 0)) {   // uniform inside the row
    if (lane == 0) { best_idx[e] = -1; best_dist[e] = 256; }
    return;
  }
  const FtTargetDev& T = targets[t];
  const ProjectRow R = project_row<MODEL>(T.F, nullptr, T.C, th, P.pos, P.normal, P.min_dist, P.max_dist, P.desc, true, i, T.sf, T.inv_sigma2, 5.99, lane,
                                          MODEL == dvm_cam::kKannalaBrandt8 ? T.kb8 : nullptr);
  if (lane == 0) {
    const int d = (int)(R.k1 >> 16);
    best_dist[e] = d;
    best_idx[e] = d <= 50 ? T.F.sidx[R.k1 & 0xFFFFu] : -1;   // ORBmatcher::TH_LOW (:1213); d = 256: no candidate
  }
}

// ---- the hits of the dense rows: entries with best_idx >= 0, target by target, in ascending point.  Three launches -- count, scan, write
// -- so that no workgroup waits on another.  One workgroup of four waves per target walks its row in rounds of 256; the compaction is the
// form of k_track_queries: a ballot and mbcnt give the lane's offset inside its wave, the four waves' counts go through LDS, a running
// base carries over the rounds.
__global__ void __launch_bounds__(256) k_ft_hit_count(const int32_t* __restrict__ best_idx, int n, int32_t* __restrict__ cnt) {
  __shared__ int s_wave[4];
  const int tid = threadIdx.x;
  const int32_t* row = best_idx + (size_t)blockIdx.x * n;
  int c = 0;                                  // wave-uniform
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int i = c0 + tid;
    c += __popcll(__ballot(i < n && row[i] >= 0));
  }
  if ((tid & 63) == 0) s_wave[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) cnt[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}
// off[t] = cnt[0] + .. + cnt[t - 1], off[T] = the total: one workgroup, rounds of 256 targets
__global__ void __launch_bounds__(256) k_ft_hit_scan(const int32_t* __restrict__ cnt, int T, int32_t* __restrict__ off, int32_t* __restrict__ off_out) {
  __shared__ int s_wave[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
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
    if (i < T) { off[i] = pre; off_out[i] = pre; }
    base += total;
    __syncthreads();
  }
  if (tid == 0) { off[T] = base; off_out[T] = base; }
}
// hits_out[off[t] ..): target t's hits; a position at or beyond cap is counted (off holds the full counts) and not written
__global__ void __launch_bounds__(256) k_ft_hit_write(const int32_t* __restrict__ best_idx, const int32_t* __restrict__ best_dist, int n,
                                                      const int32_t* __restrict__ off, FtHit* __restrict__ hits_out, int cap) {
  __shared__ int s_wave[4];
  __shared__ int32_t s_hit[256 * 3];          // the round's hits, packed: the block then stores them as one run of consecutive dwords
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int32_t* row = best_idx + (size_t)blockIdx.x * n;
  const int32_t* drow = best_dist + (size_t)blockIdx.x * n;
  int32_t* out = reinterpret_cast<int32_t*>(hits_out);
  int base = off[blockIdx.x];
  for (int c0 = 0; c0 < n; c0 += 256) {
    if (base >= cap) return;                  // uniform: positions only grow
    const int i = c0 + tid;
    const int idx = i < n ? row[i] : -1;
    const bool hit = idx >= 0;
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int pos = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));   // inside the round
    int total = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const int cw = s_wave[w];
      if (w < wv) pos += cw;
      total += cw;
    }
    if (hit) { s_hit[3 * pos] = i; s_hit[3 * pos + 1] = idx; s_hit[3 * pos + 2] = drow[i]; }
    __syncthreads();
    const int nd = 3 * min(total, cap - base);   // (base < cap here)
    for (int k = tid; k < nd; k += 256) out[3 * (size_t)base + k] = s_hit[k];
    base += total;
    __syncthreads();
  }
}

void launch_ft_build(hipStream_t s, const FtTargetDev* targets, int n_targets) {
  if (n_targets > 0) hipLaunchKernelGGL(k_ft_build, dim3(n_targets), dim3(1024), 0, s, targets);
}
void launch_ft_search(hipStream_t s, const FtTargetDev* targets, const int32_t* order, int n_pinhole, int n_kb8, const FtPoints& P, float th,
                      int32_t* best_idx, int32_t* best_dist) {
  if (P.n <= 0) return;
  const int bx = (P.n + 15) / 16;
  if (n_pinhole > 0)
    hipLaunchKernelGGL(k_ft_search<dvm_cam::kPinhole>, dim3(bx, n_pinhole), dim3(256), 0, s, targets, order, P, th, best_idx, best_dist);
  if (n_kb8 > 0)
    hipLaunchKernelGGL(k_ft_search<dvm_cam::kKannalaBrandt8>, dim3(bx, n_kb8), dim3(256), 0, s, targets, order + n_pinhole, P, th, best_idx, best_dist);
}
void launch_ft_hits(hipStream_t s, const int32_t* best_idx, const int32_t* best_dist, int n_targets, int n, int32_t* cnt, int32_t* off,
                    int32_t* off_out, FtHit* hits_out, int cap) {
  if (n_targets <= 0) return;
  hipLaunchKernelGGL(k_ft_hit_count, dim3(n_targets), dim3(256), 0, s, best_idx, n, cnt);
  hipLaunchKernelGGL(k_ft_hit_scan, dim3(1), dim3(256), 0, s, cnt, n_targets, off, off_out);
  hipLaunchKernelGGL(k_ft_hit_write, dim3(n_targets), dim3(256), 0, s, best_idx, best_dist, n, off, hits_out, cap);
}
void launch_ft_scan(hipStream_t s, const int32_t* cnt, int n, int32_t* off, int32_t* off_out) {
  hipLaunchKernelGGL(k_ft_hit_scan, dim3(1), dim3(256), 0, s, cnt, n, off, off_out);
}

}  // namespace dvm
