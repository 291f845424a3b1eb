// dvm_slam_amd/csrc/map_refresh_kernels.hip -- k_mp_refresh, the one launch of dvm_map_store_refresh (map_store.cpp): a map point's
// record made where it lies.  MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:384-453) over the descriptor rows the
// keyframe slots hold, MapPoint::UpdateNormalAndDepth (:473-540) from the record's own position (a given one for a new point) and the
// call's camera centres.  One wavefront per point; a record is read and written by its own wave only, so there is no atomic.
//   descriptor, N <= 64   lane j keeps observation j's row in eight registers, row i is broadcast from lane i (v_readlane), the distance
//                         row is one value per lane, its median the nine-step ballot search (kth_distance, match_device.h) with ONE
//                         ballot per step.  Observations on bad keyframes stay in their lanes and are masked out of every ballot, so the
//                         winner's lane IS its index in the point's full list.  No LDS, no barrier.
//   descriptor, N > 64    the candidates' rows packed into LDS in list order, then k_distinctive's own routine (distinctive_lds); the
//                         winner's index in the full list is found by counting the candidates again.  (By N, not by the candidate
//                         count: a point beyond 64 observations with so many bad keyframes that 64 remain takes this form too.)
//   geometry              the terms (pos - ow) / |pos - ow| across the lanes, 64 at a time; the SUM one term after another in list
//                         order (point_geometry.h: the bits k_ba_res_points leaves).
// No index is checked here: the entry has checked every one before anything was queued (map_refresh_lists.h).
#include <hip/hip_runtime.h>

#include "map_store.h"
#include "match_device.h"
#include "point_geometry.h"

namespace dvm {

static_assert(sizeof(LocalPointPod) == 72 && sizeof(MprKfDev) == 20 && sizeof(dvm_mp_obs) == 8 && sizeof(dvm_keypoint_pod) == 28, "the record, what travels up");

namespace {
__device__ __forceinline__ const uint8_t* mpr_slot(const MprArgs& A, const MprKfDev& kf) { return A.kf_base + (size_t)kf.slot * A.kf_stride; }
// observation j of the point whose list begins at o0: is it a candidate (its keyframe is not bad), and if so its descriptor row
__device__ __forceinline__ bool mpr_candidate(const MprArgs& A, int o0, int j, uint32_t (&w)[8]) {
  const dvm_mp_obs ob = A.obs[o0 + j];
  const MprKfDev kf = A.kfs[ob.kf];
  if (kf.fl & DVM_MPR_KF_BAD) return false;
  desc_load(mpr_slot(A, kf) + A.kf_desc, ob.kp, w);
  return true;
}
__device__ __forceinline__ float lane_value(float v, int i) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i)); }
}  // namespace

// the record as 18 words: pos 0-2, normal 3-5, min_dist 6, max_dist 7, desc 8-15, n_obs 16, bad 17
template <bool BIG>
__global__ void __launch_bounds__(64) k_mp_refresh(const MprArgs A) {
  const int p = blockIdx.x, lane = threadIdx.x;
  if (p >= A.n_points) return;
  const int o0 = A.obs_off[p], N = A.obs_off[p + 1] - o0;
  uint32_t* rec = reinterpret_cast<uint32_t*>(A.records + A.mp_slot[p]);
  const bool fresh = A.is_new && A.is_new[p];
  const bool want_d = (A.what & DVM_MPR_DESCRIPTOR) && N > 0, want_g = (A.what & DVM_MPR_GEOMETRY) && N > 0;
  // what the record holds now, a word per lane (a new point's slot holds nothing of it)
  const float old = lane < 8 && !fresh ? __uint_as_float(rec[lane]) : 0.f;

  int best_obs = -1, best_median = -1;
  if (want_d) {
    bool have = false;                             // the candidate set is not empty
    if (!BIG || N <= 64) {
      uint32_t mine[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
      const bool cand = lane < N && mpr_candidate(A, o0, lane, mine);
      unsigned long long m = __ballot(cand);
      have = m != 0;
      if (have) {
        const int k = (__popcll(m) - 1) >> 1;
        uint32_t best = 0xFFFFFFFFu;               // median << 16 | i
        while (m) {
          const int i = __ffsll(m) - 1;
          m &= m - 1;
          int d = 0;
#pragma unroll
          for (int w = 0; w < 8; w++) d += __popc((uint32_t)__builtin_amdgcn_readlane((int)mine[w], i) ^ mine[w]);
          const int med = kth_distance(k, [&](int mid) { return __popcll(__ballot(cand && d <= mid)); });
          best = min(best, ((uint32_t)med << 16) | (uint32_t)i);
        }
        best_obs = (int)(best & 0xFFFFu); best_median = (int)(best >> 16);
        if (lane == best_obs) {
#pragma unroll
          for (int w = 0; w < 8; w++) rec[8 + w] = mine[w];
        }
      }
    } else if constexpr (BIG) {
      __shared__ uint32_t s_desc[kDistinctMaxN * 8];
      __shared__ uint16_t s_row[kDistinctMaxN];
      const unsigned long long below = (1ull << lane) - 1ull;
      int cnt = 0;
      for (int base = 0; base < N; base += 64) {
        uint32_t w[8];
        const bool cand = base + lane < N && mpr_candidate(A, o0, base + lane, w);
        const unsigned long long m = __ballot(cand);
        if (cand) {
          const int r = cnt + __popcll(m & below);
#pragma unroll
          for (int q = 0; q < 8; q++) s_desc[r * 8 + q] = w[q];
        }
        cnt += __popcll(m);
      }
      __syncthreads();
      have = cnt > 0;
      if (have) {
        const uint32_t best = distinctive_lds(s_desc, s_row, cnt, lane);
        const int c = (int)(best & 0xFFFFu);       // the winner among the candidates
        best_median = (int)(best >> 16);
        int seen = 0;
        for (int base = 0; base < N; base += 64) {
          const bool cand = base + lane < N && !(A.kfs[A.obs[o0 + base + lane].kf].fl & DVM_MPR_KF_BAD);
          const unsigned long long m = __ballot(cand);
          const unsigned long long hit = __ballot(cand && seen + __popcll(m & below) == c);
          if (hit) best_obs = base + __ffsll(hit) - 1;
          seen += __popcll(m);
        }
        if (lane < 8) rec[8 + lane] = s_desc[c * 8 + lane];
      }
    }
    if (!have && fresh && lane < 8) rec[8 + lane] = 0u;   // a new point seen by bad keyframes only: its record is whole all the same
  }

  float pos[3];
  if (fresh) { pos[0] = A.new_pos[3 * (size_t)p]; pos[1] = A.new_pos[3 * (size_t)p + 1]; pos[2] = A.new_pos[3 * (size_t)p + 2]; }
  else { pos[0] = __uint_as_float(rec[0]); pos[1] = __uint_as_float(rec[1]); pos[2] = __uint_as_float(rec[2]); }
  float g[8] = {pos[0], pos[1], pos[2], 0.f, 0.f, 0.f, 0.f, 0.f};
  if (want_g) {
    float normal[3] = {0.f, 0.f, 0.f};
    for (int base = 0; base < N; base += 64) {
      float t[3] = {0.f, 0.f, 0.f};
      if (base + lane < N) geo_term(pos, A.kfs[A.obs[o0 + base + lane].kf].ow, t);
      const int m = min(64, N - base);
      for (int i = 0; i < m; i++) geo_add(normal, lane_value(t[0], i), lane_value(t[1], i), lane_value(t[2], i));
    }
    geo_mean(pos, normal, N, g);
    const dvm_mp_obs ro = A.obs[o0 + A.ref_obs[p]];
    const MprKfDev rk = A.kfs[ro.kf];
    const uint8_t* slot = mpr_slot(A, rk);
    const int octave = reinterpret_cast<const dvm_keypoint_pod*>(slot + A.kf_kps)[ro.kp].octave;
    geo_distances(pos, rk.ow, reinterpret_cast<const float*>(slot + A.kf_sf), octave, (int)(rk.fl >> 8), g);
  }
  if (lane < 8) {
    float v = old;
    if (lane < 3) v = lane == 0 ? g[0] : lane == 1 ? g[1] : g[2];
    else if (want_g) v = lane == 3 ? g[3] : lane == 4 ? g[4] : lane == 5 ? g[5] : lane == 6 ? g[6] : g[7];
    if (fresh || (want_g && lane >= 3)) rec[lane] = __float_as_uint(v);
    if (A.geometry_out) A.geometry_out[8 * (size_t)p + lane] = v;
  }
  if (lane == 0) {
    rec[16] = (uint32_t)N;
    if (fresh) rec[17] = 0u;
    A.best_obs_out[p] = best_obs;
    if (A.best_median_out) A.best_median_out[p] = best_median;
  }
}

void launch_mp_refresh(hipStream_t s, const MprArgs& A, bool big) {
  if (A.n_points <= 0) return;
  if (big) hipLaunchKernelGGL(k_mp_refresh<true>, dim3((unsigned)A.n_points), dim3(64), 0, s, A);
  else hipLaunchKernelGGL(k_mp_refresh<false>, dim3((unsigned)A.n_points), dim3(64), 0, s, A);
}

}  // namespace dvm
