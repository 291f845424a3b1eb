// dvm_slam_amd/csrc/match_device.h -- the inner steps every matcher kernel shares, one definition each (match_kernels.hip, track_kernels.hip,
// bow_targets_kernels.hip, new_points_kernels.hip, proj_device.h, tri_device.h):
//   desc_load / desc_distance        ORBmatcher::DescriptorDistance (reference src/ORBmatcher.cc:1900-1914): popcount over 8 dwords
//   window_scan<LANES>               Frame::GetFeaturesInArea (src/Frame.cc:712-770) over a frame's sorted keypoints
//   row_min / row_top2               reductions over a DPP row (16 lanes);  wave_min / wave_top2 / wave_sum: over the wave
//   block_sum4_put / block_sum4      a count summed over a workgroup of four waves
//   fv_find / fv_node_of             lookups in a DBoW2 FeatureVector stored as (fv_node[], fv_off[], fv_feat[])
//   bow_node_scan                    the per-feature step of ORBmatcher::SearchByBoW inside one vocabulary node
// The tie rules live in the callers' key encodings (window keys dist << 16 | sorted position, tri_key, BoW keys dist << 20 | scan
// position): everything here only takes minima of keys.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.h"

namespace dvm {

// ---- descriptors: 32 bytes at base + 32 * idx, read as two 16-byte loads
__device__ __forceinline__ void desc_load(const uint8_t* __restrict__ base, int idx, uint32_t (&w)[8]) {
  const uint4* q = reinterpret_cast<const uint4*>(base + (size_t)idx * 32);
  const uint4 a = q[0], b = q[1];
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
__device__ __forceinline__ int desc_distance(const uint32_t (&w)[8], const uint8_t* __restrict__ base, int idx) {
  const uint4* td = reinterpret_cast<const uint4*>(base + (size_t)idx * 32);
  const uint4 a = td[0], b = td[1];
  return __popc(a.x ^ w[0]) + __popc(a.y ^ w[1]) + __popc(a.z ^ w[2]) + __popc(a.w ^ w[3]) +
         __popc(b.x ^ w[4]) + __popc(b.y ^ w[5]) + __popc(b.z ^ w[6]) + __popc(b.w ^ w[7]);
}

// the two smallest keys seen so far, k1 <= k2 (an equal key counts again: it becomes the second).  Written with min / max: the form
// "if (k < k1) { k2 = k1; k1 = k; } else if (k < k2) k2 = k;" on references compiles to a store through a selected address, which
// keeps k1 and k2 in scratch memory.
template <class T>
__device__ __forceinline__ void top2_insert(T& k1, T& k2, T k) {
  k2 = min(k2, max(k1, k));
  k1 = min(k1, k);
}

// ---- sums across the lanes that share a window (window_scan).  lanes_prefix: the inclusive prefix sum of v over a DPP row (LANES = 16:
// four row_shr steps, a lane without a source adds 0) or over the wave (LANES = 64: the row prefixes plus the totals of the rows in front,
// read with v_readlane -- the caller is in wave-uniform control flow with all 64 lanes active); lanes_total: the last lane's prefix in
// every lane.
#define DVM_ROW_SHR(v, N) __builtin_amdgcn_update_dpp(0, v, 0x110 + N, 0xF, 0xF, false)
template <int LANES>
__device__ __forceinline__ int lanes_prefix(int v, int lane) {
  static_assert(LANES == 16 || LANES == 64, "a DPP row or the wave");
  v += DVM_ROW_SHR(v, 1);
  v += DVM_ROW_SHR(v, 2);
  v += DVM_ROW_SHR(v, 4);
  v += DVM_ROW_SHR(v, 8);
  if constexpr (LANES == 64) {
    const int t0 = __builtin_amdgcn_readlane(v, 15), t1 = __builtin_amdgcn_readlane(v, 31), t2 = __builtin_amdgcn_readlane(v, 47);
    v += (lane >= 16 ? t0 : 0) + (lane >= 32 ? t1 : 0) + (lane >= 48 ? t2 : 0);
  }
  return v;
}
#undef DVM_ROW_SHR
template <int LANES>
__device__ __forceinline__ int lanes_total(int incl) {
  if constexpr (LANES == 64) return __builtin_amdgcn_readlane(incl, 63);
  else return __builtin_amdgcn_update_dpp(0, incl, 0x15F, 0xF, 0xF, false);   // row_newbcast:15
}

// ---- GetFeaturesInArea(x, y, r, minLevel, maxLevel) of frame F: the cell rectangle with the reference's early-outs, then the keypoints
// of the rectangle's cells alone across LANES lanes (16: one DPP row per query; 64: the whole wave); visit(p, oct, dx, dy) for every
// sorted position p that passes the level and radius tests (oct = its octave, dx / dy = its offset from the window's centre), in no
// particular order: the callers take minima of keys.
// Rows nMinCellY .. nMaxCellY of grid column c are one span of sorted positions, cell_start[c * 48 + nMinCellY] .. cell_start[c * 48 +
// nMaxCellY + 1).  The columns go LANES at a time: a lane owns one column's span, a prefix sum over the span lengths gives every span its
// place in one flat range, and each owner writes its span's positions (uint16: < kFrameCap) to the window's LDS queue at that place.  The
// lanes then walk the queue side by side, so a round of the loop tests LANES keypoints of the rectangle whatever the columns hold.  The
// queue holds kWindowQueue * LANES positions and is filled again, pass by pass, where a group of columns holds more.  It is the window's
// own (128 B per DPP row, 512 B per wave, workgroups of at most 256 threads) and one wave's LDS operations execute in order: between the
// writes and the reads the compiler only has to keep that order (a wavefront-scope fence).
constexpr int kWindowQueue = 4;
template <int LANES, class Visit>
__device__ __forceinline__ void window_scan(const FrameView& F, float x, float y, float r, int minLevel, int maxLevel, int lane, Visit visit) {
  const int nMinCellX = max(0, (int)floorf((x - F.minX - r) * F.wInv));
  const int nMaxCellX = min(kGridCols - 1, (int)ceilf((x - F.minX + r) * F.wInv));
  const int nMinCellY = max(0, (int)floorf((y - F.minY - r) * F.hInv));
  const int nMaxCellY = min(kGridRows - 1, (int)ceilf((y - F.minY + r) * F.hInv));
  const bool empty = nMinCellX >= kGridCols || nMaxCellX < 0 || nMinCellY >= kGridRows || nMaxCellY < 0;
  if (empty || nMinCellX > nMaxCellX || nMinCellY > nMaxCellY) return;
  const bool checkLevels = (minLevel > 0) || (maxLevel >= 0);
  constexpr int kQueue = kWindowQueue * LANES;
  __shared__ uint16_t s_queue[(256 / LANES) * kQueue];
  uint16_t* queue = s_queue + (threadIdx.x / LANES) * kQueue;
  for (int g = nMinCellX; g <= nMaxCellX; g += LANES) {
    const int c = g + lane;
    int beg = 0, len = 0;
    if (c <= nMaxCellX) {
      beg = F.cell_start[c * kGridRows + nMinCellY];
      len = F.cell_start[c * kGridRows + nMaxCellY + 1] - beg;
    }
    const int incl = lanes_prefix<LANES>(len, lane), excl = incl - len;
    const int total = lanes_total<LANES>(incl);
    for (int base = 0; base < total; base += kQueue) {
      const int hi = min(incl, base + kQueue);
#pragma clang loop vectorize(disable) unroll(disable)
      for (int f = max(excl, base); f < hi; f++) queue[f - base] = (uint16_t)(beg + (f - excl));
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const int n = min(total - base, kQueue);
      for (int j = lane; j < n; j += LANES) {
        const int p = queue[j];
        const float4 kp = F.skp[p];
        const int oct = __float_as_int(kp.z);
        if (checkLevels) {
          if (oct < minLevel) continue;
          if (maxLevel >= 0 && oct > maxLevel) continue;
        }
        const float dx = kp.x - x, dy = kp.y - y;
        if (!(fabsf(dx) < r && fabsf(dy) < r)) continue;
        visit(p, oct, dx, dy);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ---- reductions.  A DPP row: xor-1, xor-2 inside quads, then half-row and row mirrors; every lane of the row ends with the result.
#define DVM_ROW_DPP(v, CTRL, OLD) (uint32_t)__builtin_amdgcn_update_dpp(OLD, (int)(v), CTRL, 0xF, 0xF, false)
__device__ __forceinline__ uint32_t row_min(uint32_t k) {
  k = min(k, DVM_ROW_DPP(k, 0xB1, -1));    // quad_perm [1,0,3,2]
  k = min(k, DVM_ROW_DPP(k, 0x4E, -1));    // quad_perm [2,3,0,1]
  k = min(k, DVM_ROW_DPP(k, 0x141, -1));   // row_half_mirror
  k = min(k, DVM_ROW_DPP(k, 0x140, -1));   // row_mirror
  return k;
}
// the two smallest of two ascending pairs (disjoint sets): min(a1, b1), min(max(a1, b1), min(a2, b2))
template <class T>
__device__ __forceinline__ void top2_merge(T& k1, T& k2, T o1, T o2) {
  const T n1 = min(k1, o1), n2 = min(max(k1, o1), min(k2, o2));
  k1 = n1; k2 = n2;
}
__device__ __forceinline__ void row_top2(uint32_t& k1, uint32_t& k2) {
  top2_merge(k1, k2, DVM_ROW_DPP(k1, 0xB1, 0), DVM_ROW_DPP(k2, 0xB1, 0));
  top2_merge(k1, k2, DVM_ROW_DPP(k1, 0x4E, 0), DVM_ROW_DPP(k2, 0x4E, 0));
  top2_merge(k1, k2, DVM_ROW_DPP(k1, 0x141, 0), DVM_ROW_DPP(k2, 0x141, 0));
  top2_merge(k1, k2, DVM_ROW_DPP(k1, 0x140, 0), DVM_ROW_DPP(k2, 0x140, 0));
}
#undef DVM_ROW_DPP
__device__ __forceinline__ uint32_t wave_min(uint32_t k) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) k = min(k, (uint32_t)__shfl_xor((int)k, o));
  return k;
}
template <class T>
__device__ __forceinline__ void wave_top2(T& k1, T& k2) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const T o1 = __shfl_xor(k1, o), o2 = __shfl_xor(k2, o);
    top2_merge(k1, k2, o1, o2);
  }
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// The sum of v over a workgroup of four waves in two halves: every thread calls block_sum4_put(v, s4) (s4: four ints of LDS), and
// behind the caller's next barrier block_sum4(s4) is the sum.
__device__ __forceinline__ void block_sum4_put(int v, int* s4) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
}
__device__ __forceinline__ int block_sum4(const int* s4) { return s4[0] + s4[1] + s4[2] + s4[3]; }

// ---- FeatureVector lookups.  fv_find: the index of `node` in the ascending list fv_node[0 .. fv_n) or -1.  DBoW2's NodeId is
// unsigned, so every list ascends as uint32_t: node -1 (a walk that ended above level L - levelsup) is last.
__device__ __forceinline__ int fv_find(const int32_t* __restrict__ fv_node, int fv_n, int32_t node) {
  int lo = 0, hi = fv_n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((uint32_t)fv_node[mid] < (uint32_t)node) lo = mid + 1; else hi = mid;
  }
  return lo < fv_n && fv_node[lo] == node ? lo : -1;
}
// the list index of the node that holds feature position k: the last node whose offset is <= k
__device__ __forceinline__ int fv_node_of(const int32_t* __restrict__ fv_off, int fv_n, int k) {
  int lo = 0, hi = fv_n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (fv_off[mid] <= k) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- SearchByBoW inside one node, for one query feature, by one wave: the query qdesc[r] against the features fv_feat[fb .. fe) of
// `desc`, scan position p across the 64 lanes, those skipped for which taken(p, j) holds (j = fv_feat[p]).  Returns, in every lane, the
// smallest (distance << 20 | scan position - fb) -- first in scan order wins -- or 0xFFFFFFFF without a candidate; second = the second
// smallest distance (duplicates counted), 256 without one.
template <class Taken>
__device__ __forceinline__ uint32_t bow_node_scan(const uint8_t* __restrict__ qdesc, int r, const int32_t* __restrict__ fv_feat, int fb, int fe,
                                                  const uint8_t* __restrict__ desc, int lane, Taken taken, int& second) {
  uint32_t w[8];
  desc_load(qdesc, r, w);
  uint32_t best = 0xFFFFFFFFu;
  int d1 = 256, d2 = 256;
  for (int p = fb + lane; p < fe; p += 64) {
    const int j = fv_feat[p];
    if (taken(p, j)) continue;
    const int d = desc_distance(w, desc, j);
    best = min(best, ((uint32_t)d << 20) | (uint32_t)(p - fb));
    top2_insert(d1, d2, d);
  }
  wave_top2(d1, d2);
  second = d2;
  return wave_min(best);
}

// ---- MapPoint::ComputeDistinctiveDescriptors' order statistic (reference src/MapPoint.cc:384-453), shared by k_distinctive
// (match_kernels.hip) and k_mp_refresh (map_refresh_kernels.hip).  kth_distance: the smallest v in [0, 256] with count_le(v) > k -- the
// k-th value of a sorted row of Hamming distances -- by a binary search over the value range, nine steps, no sort; count_le(v) counts the
// row's entries <= v (ballots) and is wave-uniform.
constexpr int kDistinctMaxN = 512;
template <class CountLE>
__device__ __forceinline__ int kth_distance(int k, CountLE count_le) {
  int lo = 0, hi = 256;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (count_le(mid) > k) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// The LDS form, for ONE wavefront that is its whole workgroup: s_desc [N][8] holds the N <= kDistinctMaxN descriptors (written and
// made visible by the caller: a barrier behind its stores), s_row [N] is scratch.  Row i = one distance per lane in chunks of 64, its
// median = sorted_row[(N - 1) >> 1] with the self distance included.  Returns median << 16 | i of the first row with the strictly
// smallest median, in every lane; s_desc is as it was and no lane is still reading s_row.
__device__ __forceinline__ uint32_t distinctive_lds(const uint32_t* s_desc, uint16_t* s_row, int N, int lane) {
  const int k = (N - 1) >> 1;                     // (size_t)(0.5 * (N - 1))
  uint32_t best = 0xFFFFFFFFu;
  for (int i = 0; i < N; i++) {
    uint32_t di[8];
#pragma unroll
    for (int w = 0; w < 8; w++) di[w] = s_desc[i * 8 + w];
    for (int j = lane; j < N; j += 64) {
      int d = 0;
#pragma unroll
      for (int w = 0; w < 8; w++) d += __popc(di[w] ^ s_desc[j * 8 + w]);
      s_row[j] = (uint16_t)d;
    }
    __syncthreads();
    const int med = kth_distance(k, [&](int mid) {
      int cnt = 0;
      for (int base = 0; base < N; base += 64) {
        const int j = base + lane;
        cnt += __popcll(__ballot(j < N && (int)s_row[j] <= mid));
      }
      return cnt;
    });
    best = min(best, ((uint32_t)med << 16) | (uint32_t)i);
    __syncthreads();
  }
  return best;
}

}  // namespace dvm
