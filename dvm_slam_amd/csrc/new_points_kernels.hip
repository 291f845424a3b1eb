// dvm_slam_amd/csrc/new_points_kernels.hip -- LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:446-760, monocular) for all
// neighbour keyframes of the current keyframe as three launches behind one upload (dvm_create_new_map_points, include/dvmslam_hip.h):
//   k_np_search     ORBmatcher::SearchForTriangulation's search (src/ORBmatcher.cc:890-960) for every (neighbour, KF1 keypoint without a
//                   point AT ENTRY), speculatively: the reference never sets vbMatched2, so a keypoint's best candidate in a neighbour
//                   depends on nothing the loop over the neighbours changes
//   k_np_geometry   the per-match body of CreateNewMapPoints (:598-741) for every best candidate found
//   k_np_settle     ONE workgroup walks the neighbours in order: the matches of keypoints that still have no point vote in the rotation
//                   histogram (:961-1031), the survivors are compacted in ascending idx1 with their precomputed status and point, and the
//                   keypoints of accepted pairs are marked (what pKF->AddMapPoint does to the table, :744)
// The launches' order carries the dependency; no workgroup waits for another inside a kernel.  The per-candidate test and the per-pair
// geometry are the functions the single calls run (tri_device.h); the FeatureVector lookups are match_device.h's.  The pinhole and the
// KannalaBrandt8 kernels of a pair are one template body each.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "new_points_kernels.h"
#include "rot_bin.h"
#include "tri_device.h"

namespace dvm {

// What the row of KF1 feature position k asks of neighbour N: idx1 = the keypoint, [fb, fe) = the positions of k's vocabulary node in N's
// FeatureVector (node ids ascend as unsigned, node -1 last).  false: nothing to search -- k past the list, a keypoint with a MapPoint at entry (never
// asked), or a node the neighbour lacks.
__device__ __forceinline__ bool np_node_range(const NpArgs& A, const NpNbDev& N, int k, int& idx1, int& fb, int& fe) {
  const NpKfDev& C = A.cur;
  if (k >= A.nfeat1) return false;
  idx1 = C.fv_feat[k];
  if (C.mp[idx1] >= 0) return false;
  const int at = fv_find(N.kf.fv_node, N.kf.fv_n, C.fv_node[fv_node_of(C.fv_off, C.fv_n, k)]);
  if (at < 0) return false;
  fb = N.kf.fv_off[at]; fe = N.kf.fv_off[at + 1];
  return true;
}

// One DPP row (16 lanes) per (KF1 feature position k, neighbour blockIdx.y).  The row scans the KF2 features of k's node (np_node_range)
// across its lanes, those with a map point skipped; a tie goes to the last candidate in the node's order, as in k_match_triangulation.
__global__ void __launch_bounds__(256) k_np_search(NpArgs A) {
  const int lane = threadIdx.x & 15;
  const int k = blockIdx.x * 16 + (threadIdx.x >> 4);
  const NpKfDev& C = A.cur;
  const NpNbDev& N = A.nb[blockIdx.y];
  int idx1 = 0, fb = 0, fe = 0;
  if (!np_node_range(A, N, k, idx1, fb, fe)) return;
  const TriQuery Q = tri_query(C.desc, C.kps, idx1, N.G.F12);
  uint32_t key = 0xFFFFFFFFu;
  for (int p = fb + lane; p < fe; p += 16) {
    const int idx2 = N.kf.fv_feat[p];
    if (N.kf.mp[idx2] >= 0) continue;
    if ((unsigned)N.kf.kps[idx2].octave >= (unsigned)A.n_levels) continue;   // outside the tables: no candidate, nothing read
    const int d = tri_candidate(Q, N.kf.desc, N.kf.kps, idx2, N.G, N.kf.sf, N.kf.sigma2);
    if (d < 0) continue;
    key = min(key, tri_key(d, p - fb));
  }
  key = row_min(key);
  if (lane == 0 && key != 0xFFFFFFFFu) A.best[(size_t)blockIdx.y * A.n1p + idx1] = N.kf.fv_feat[fb + tri_key_pos(key)];
}

// thread per (KF1 keypoint, neighbour blockIdx.y) with a best candidate: tri_pair_geometry<MODEL>, for KannalaBrandt8 on the pair's
// cameras G[blockIdx.y].cam1 / cam2 (G is not read for the pinhole camera)
template <int MODEL>
__device__ __forceinline__ void np_geometry_thread(const NpArgs& A, const TriGeomKB8* G) {
  const int i = blockIdx.x * 128 + threadIdx.x;
  if (i >= A.n1) return;
  const size_t o = (size_t)blockIdx.y * A.n1p + i;
  const int m = A.best[o];
  if (m < 0) return;
  const NpNbDev& N = A.nb[blockIdx.y];
  const float *cam1 = nullptr, *cam2 = nullptr;
  if constexpr (MODEL == dvm_cam::kKannalaBrandt8) { cam1 = G[blockIdx.y].cam1; cam2 = G[blockIdx.y].cam2; }
  float x[3];
  A.st[o] = tri_pair_geometry<MODEL>(N.P, A.cur.kps[i], N.kf.kps[m], A.cur.sigma2, N.kf.sigma2, A.cur.sf, N.kf.sf, x, cam1, cam2);
  A.X[3 * o] = x[0]; A.X[3 * o + 1] = x[1]; A.X[3 * o + 2] = x[2];
}
__global__ void __launch_bounds__(128) k_np_geometry(NpArgs A) { np_geometry_thread<dvm_cam::kPinhole>(A, nullptr); }

// One workgroup; thread t owns the keypoints [t * chunk, (t + 1) * chunk) (chunk <= 8: 8192 keypoints), so the table in LDS is only ever
// touched by its owner and the records of a neighbour come out in ascending idx1 from an exclusive scan of the per-thread counts.
__global__ void __launch_bounds__(1024) k_np_settle(NpArgs A) {
  __shared__ uint8_t s_has[kFrameCap];
  __shared__ int s_hist[kRotHisto];
  __shared__ int s_ind[3];
  __shared__ int s_wave[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const NpKfDev& C = A.cur;
  const int chunk = (A.n1 + 1023) / 1024;
  const int b = min(tid * chunk, A.n1), e = min(b + chunk, A.n1);
  for (int i = b; i < e; i++) { s_has[i] = C.mp[i] >= 0 ? 1 : 0; A.h_new_point[i] = -1; }
  if (tid == 0) A.h_pair_off[0] = 0;
  int base = 0;
  for (int r = 0; r < A.nrun; r++) {
    const NpNbDev& N = A.nb[r];
    const int32_t* best = A.best + (size_t)r * A.n1p;
    if (tid < kRotHisto) s_hist[tid] = 0;
    __syncthreads();
    int bins[8];
    unsigned live = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int i = b + j;
      bins[j] = -1;
      if (i >= e) continue;
      const int m = best[i];
      if (m < 0 || s_has[i]) continue;               // no match, or a point from an earlier neighbour: the reference does not ask (:897-902)
      live |= 1u << j;
      const int bin = rot_bin(C.kps[i].angle, N.kf.kps[m].angle);
      if (bin >= 0 && bin < kRotHisto) { bins[j] = bin; if (A.check_ori) atomicAdd(&s_hist[bin], 1); }
    }
    __syncthreads();
    if (tid == 0) three_maxima(s_hist, s_ind);
    __syncthreads();
    unsigned keep = live;
    if (A.check_ori) {
#pragma unroll
      for (int j = 0; j < 8; j++)
        if (bins[j] < 0 || rot_dropped(bins[j], s_ind)) keep &= ~(1u << j);
    }
    const int cnt = __popc(keep);
    int incl = cnt;                                   // inclusive scan inside the wave, then over the 16 waves
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) { const int v = s_wave[w]; if (w < wave) before += v; total += v; }
    int rec = base + before + incl - cnt;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (!(keep >> j & 1u)) continue;
      const int i = b + j;
      const size_t o = (size_t)r * A.n1p + i;
      const int st = A.st[o];
      A.h_pairs[2 * (size_t)rec] = i; A.h_pairs[2 * (size_t)rec + 1] = best[i];
      A.h_status[rec] = st;
      A.h_x3D[3 * (size_t)rec] = A.X[3 * o]; A.h_x3D[3 * (size_t)rec + 1] = A.X[3 * o + 1]; A.h_x3D[3 * (size_t)rec + 2] = A.X[3 * o + 2];
      if (st == 0) { s_has[i] = 1; A.h_new_point[i] = rec; }
      rec++;
    }
    base += total;
    if (tid == 0) { A.h_matches[r] = total; A.h_pair_off[r + 1] = base; }
    __syncthreads();                                  // s_wave and s_hist are rewritten by the next neighbour
  }
}

// ---- KannalaBrandt8 keyframes.  k_np_settle reads no camera and serves both models.

// k_np_search with KannalaBrandt8::epipolarConstrain as the candidate test, run over the workgroup's survivors of the two cheap tests
// (tri_rows_kb8, tri_device.h): no row leaves before the workgroup's barriers
__global__ void __launch_bounds__(256) k_np_search_kb8(NpArgsKB8 K) {
  __shared__ TriBlockKB8 S;
  const NpArgs& A = K.A;
  const int lane = threadIdx.x & 15;
  const int k = blockIdx.x * 16 + (threadIdx.x >> 4);
  const NpKfDev& C = A.cur;
  const NpNbDev& N = A.nb[blockIdx.y];
  const TriGeomKB8& G = K.G[blockIdx.y];
  int idx1 = 0, fb = 0, fe = 0;
  const bool active = np_node_range(A, N, k, idx1, fb, fe);
  const uint32_t key = tri_rows_kb8(S, active, C.desc, C.kps, idx1, fb, fe,
                                    [&](int p) { const int idx2 = N.kf.fv_feat[p]; return N.kf.mp[idx2] >= 0 ? -1 : idx2; }, N.kf.desc, N.kf.kps, G,
                                    C.sigma2, N.kf.sf, N.kf.sigma2, A.n_levels);
  if (lane == 0 && active && key != 0xFFFFFFFFu) A.best[(size_t)blockIdx.y * A.n1p + idx1] = N.kf.fv_feat[fb + tri_key_pos(key)];
}

__global__ void __launch_bounds__(128) k_np_geometry_kb8(NpArgsKB8 K) { np_geometry_thread<dvm_cam::kKannalaBrandt8>(K.A, K.G); }

void launch_np_search_kb8(hipStream_t s, const NpArgsKB8& K) {
  if (K.A.nrun < 1 || K.A.nfeat1 < 1) return;
  hipLaunchKernelGGL(k_np_search_kb8, dim3((K.A.nfeat1 + 15) / 16, K.A.nrun), dim3(256), 0, s, K);
}
void launch_np_geometry_kb8(hipStream_t s, const NpArgsKB8& K) {
  if (K.A.nrun < 1 || K.A.n1 < 1) return;
  hipLaunchKernelGGL(k_np_geometry_kb8, dim3((K.A.n1 + 127) / 128, K.A.nrun), dim3(128), 0, s, K);
}
void launch_np_search(hipStream_t s, const NpArgs& A) {
  if (A.nrun < 1 || A.nfeat1 < 1) return;
  hipLaunchKernelGGL(k_np_search, dim3((A.nfeat1 + 15) / 16, A.nrun), dim3(256), 0, s, A);
}
void launch_np_geometry(hipStream_t s, const NpArgs& A) {
  if (A.nrun < 1 || A.n1 < 1) return;
  hipLaunchKernelGGL(k_np_geometry, dim3((A.n1 + 127) / 128, A.nrun), dim3(128), 0, s, A);
}
void launch_np_settle(hipStream_t s, const NpArgs& A) { hipLaunchKernelGGL(k_np_settle, dim3(1), dim3(1024), 0, s, A); }

}  // namespace dvm
