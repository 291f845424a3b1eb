// dvm_slam_amd/csrc/match_kernels.hip -- gfx950 kernels of the matching path.
//
//   ORBmatcher::DescriptorDistance (reference src/ORBmatcher.cc:1900-1914) -> desc_distance (match_device.h)
//   Frame::AssignFeaturesToGrid / PosInGrid (src/Frame.cc:481-506,773-782)  -> k_frame_build
//   Frame::GetFeaturesInArea (src/Frame.cc:712-770) + the best / second-best loops of
//   ORBmatcher::SearchByProjection (src/ORBmatcher.cc:70-115,1604-1639)      -> k_match_window
// (the grid build, the best two of a window and the projection row are device functions of proj_device.h: fuse_targets_kernels.hip calls
// them too; the window scan itself, the descriptor distance and the row / wave reductions are match_device.h's, shared with the chains)
//
// Layout: a frame's keypoints are stored SORTED by (grid column ix, grid row iy, keypoint index) --
// exactly the order in which GetFeaturesInArea enumerates candidates -- so "first candidate wins a
// tie" becomes "smallest sorted position wins", an associative rule a wavefront can reduce.
#include <hip/hip_runtime.h>

#include "frustum_point.h"
#include "match_device.h"
#include "match_kernels.h"
#include "pose_f32.h"
#include "proj_device.h"
#include "undistort_f64.h"
#include "jacobi4.h"
#include "tri_device.h"

namespace dvm {

// One workgroup (1024 threads) per frame slot (frame_build_block, proj_device.h: bitonic sort of (cell << 13 | idx) keys in LDS, then
// gather).  Slot s = first_slot + blockIdx.x reads keypoints kps + blockIdx.x*kps_stride.
__global__ void __launch_bounds__(1024) k_frame_build(const dvm_keypoint_pod* __restrict__ kps_base, int64_t kps_stride,
                                                      const uint8_t* __restrict__ desc_base, int64_t desc_stride,
                                                      int n_host, const int32_t* __restrict__ d_n, FrameView FB,
                                                      int first_slot) {
  const int tid = threadIdx.x;
  const FrameView F = FB.slot(first_slot + blockIdx.x);
  const dvm_keypoint_pod* kps = kps_base + (int64_t)blockIdx.x * kps_stride;
  const uint8_t* desc = desc_base + (int64_t)blockIdx.x * desc_stride;
  int n = d_n ? d_n[blockIdx.x] : n_host;
  if (tid == 0 && n > F.cap) atomicAdd(F.n_overflow, 1);   // a truncated frame is reported, not hidden (dvm_frame_overflows)
  n = min(max(n, 0), F.cap);
  frame_build_block(kps, desc, n, F);
}


// Sixteen lanes (one DPP row) per query, four queries per wave: a window's cell rectangle holds ~25 keypoints (window_scan walks those
// alone), so a full wave per query left most lanes idle and paid a 6-step cross-lane reduction; a row reduces its top-2 with four DPP
// steps.  QUERIES_FROM_KPS: queries are keypoints of another frame (frame-to-frame
// search, window th*scale[octave], octaves [o-1,o+1]); otherwise explicit query arrays.
template <bool QUERIES_FROM_KPS>
__global__ void __launch_bounds__(256) k_match_window(FrameView FB, int first_slot, const uint8_t* __restrict__ skip,
                                                      const uint8_t* __restrict__ qdesc, const float* __restrict__ qx,
                                                      const float* __restrict__ qy, const float* __restrict__ qr,
                                                      const int32_t* __restrict__ qmin, const int32_t* __restrict__ qmax,
                                                      int nq_host, const int32_t* __restrict__ d_nq, PairQueries PQ,
                                                      float th, const float* __restrict__ scale_factors, int nlevels,
                                                      dvm_match_pod* __restrict__ out, int64_t out_stride,
                                                      int32_t* __restrict__ second_idx) {
  const int lane = threadIdx.x & 15;               // lane within the query's row
  const int q = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int pair = blockIdx.y;
  const FrameView F = FB.slot(first_slot + pair);
  const dvm_keypoint_pod* qkps = nullptr;
  int nq;
  if (QUERIES_FROM_KPS) {
    // pair 0 takes its queries from the carry frame (previous batch), pair i>0 from frame i-1
    if (pair == 0) {
      if (!PQ.carry_kps) { if (q == 0 && lane == 0 && PQ.n_out) PQ.n_out[0] = 0; return; }
      qkps = PQ.carry_kps; qdesc = PQ.carry_desc; nq = *PQ.carry_n;
    } else {
      qkps = PQ.kps + (int64_t)(pair - 1) * PQ.kps_stride;
      qdesc = PQ.desc + (int64_t)(pair - 1) * PQ.desc_stride;
      nq = PQ.n[pair - 1];
    }
    if (q == 0 && lane == 0 && nq > PQ.cap) atomicAdd(F.n_overflow, 1);
    nq = min(nq, PQ.cap);
    if (q == 0 && lane == 0 && PQ.n_out) PQ.n_out[pair] = nq;
    out += (int64_t)pair * out_stride;
  } else {
    nq = d_nq ? *d_nq : nq_host;
  }
  if (q >= nq) return;
  float x, y, r;
  int minLevel, maxLevel;
  if (QUERIES_FROM_KPS) {
    const dvm_keypoint_pod kp = qkps[q];
    x = kp.x; y = kp.y;
    const int o = min(max(kp.octave, 0), nlevels - 1);
    r = th * scale_factors[o];
    minLevel = kp.octave - 1;
    maxLevel = kp.octave + 1;
  } else {
    x = qx[q]; y = qy[q]; r = qr[q];
    minLevel = qmin[q]; maxLevel = qmax[q];
  }
  uint32_t k1, k2;
  window_top2(F, x, y, r, minLevel, maxLevel, qdesc + (size_t)q * 32, skip, nullptr, 0.0, lane, k1, k2);
  if (lane == 0) {
    dvm_match_pod m;
    const int p1 = (int)(k1 & 0xFFFFu), p2 = (int)(k2 & 0xFFFFu);
    m.best_dist = (int)(k1 >> 16);
    m.second_dist = (int)(k2 >> 16);
    m.best_idx = (m.best_dist < 256) ? F.sidx[p1] : -1;
    m.best_level = (m.best_dist < 256) ? (int16_t)__float_as_int(F.skp[p1].z) : (int16_t)-1;
    m.second_level = (m.second_dist < 256) ? (int16_t)__float_as_int(F.skp[p2].z) : (int16_t)-1;
    out[q] = m;
    // the runner-up's index: what the reference's scan finds when the best candidate is excluded (a caller replaying claims)
    if (!QUERIES_FROM_KPS && second_idx) second_idx[q] = (m.second_dist < 256) ? F.sidx[p2] : -1;
  }
}

// The same scan returning the FOUR best candidates in the reference's order of preference (distance, then scan position: strict '<',
// first wins).  A caller that replays ORBmatcher.cc:1613-1664's claims in query order walks the list to the first keypoint no earlier
// query of the call has taken -- with the best two only (k_match_window), 15 % of a frame's queries had to be searched again on the host.
// ranked[q][c] = dist << 16 | train index, dist = 256 from the end of the list on (fewer than four candidates: the list is complete).
__device__ __forceinline__ void sort4(uint32_t (&k)[4]) {
  uint32_t t;
#define DVM_CE(a, b) t = min(k[a], k[b]); k[b] = max(k[a], k[b]); k[a] = t;
  DVM_CE(0, 1) DVM_CE(2, 3) DVM_CE(0, 2) DVM_CE(1, 3) DVM_CE(1, 2)
#undef DVM_CE
}
// blockIdx.y = frame of a batch (the shared search service, dvm_match_pool_*): frame b searches grid slot `slot + b` with its own query
// arrays at b * qstride elements, nq_arr[b] queries and -- where skip_on[b] is set -- the skip flags at b * skip_stride bytes.
// A single search is the batch of one (qstride = 0, nq_arr = skip_on = NULL).  qoff (may be NULL): frame b's query arrays at qoff[b]
// elements instead of b * qstride (tables of different sizes back to back; qstride then only sizes the grid: the largest frame's queries).
__global__ void __launch_bounds__(256) k_match_window_ranked(FrameView FB, int slot, const uint8_t* __restrict__ skip,
                                                             const uint8_t* __restrict__ qdesc, const float* __restrict__ qx,
                                                             const float* __restrict__ qy, const float* __restrict__ qr,
                                                             const int32_t* __restrict__ qmin, const int32_t* __restrict__ qmax, int nq,
                                                             uint32_t* __restrict__ ranked, int qstride, const int32_t* __restrict__ nq_arr,
                                                             const int32_t* __restrict__ skip_on, int skip_stride,
                                                             const int32_t* __restrict__ qoff) {
  const int lane = threadIdx.x & 15;               // lane within the query's DPP row
  const int q = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int b = blockIdx.y;
  if (nq_arr) nq = nq_arr[b];
  if (q >= nq) return;
  const FrameView F = FB.slot(slot + b);
  {
    const size_t o = qoff ? (size_t)qoff[b] : (size_t)b * qstride;
    qdesc += o * 32; qx += o; qy += o; qr += o; qmin += o; qmax += o; ranked += o * 4;
    if (skip_on) skip = skip_on[b] ? skip + (size_t)b * skip_stride : nullptr;
  }
  const float x = qx[q], y = qy[q], r = qr[q];
  const int minLevel = qmin[q], maxLevel = qmax[q];
  const uint32_t none = (256u << 16) | 0xFFFFu;
  uint32_t k[4] = {none, none, none, none};
  uint32_t w[8];
  desc_load(qdesc, q, w);
  window_scan<16>(F, x, y, r, minLevel, maxLevel, lane, [&](int p, int, float, float) {
    if (skip && skip[F.sidx[p]]) return;
    const uint32_t key = ((uint32_t)desc_distance(w, F.sdesc, p) << 16) | (uint32_t)p;
    if (key < k[3]) { k[3] = key; sort4(k); }
  });
  // the four smallest of two ascending 4-lists: min(a[i], b[3 - i]) (a bitonic half-cleaner), sorted again; the sets are disjoint
#define DVM_TOP4_STEP(CTRL)                                                                                     \
  {                                                                                                             \
    uint32_t o[4];                                                                                              \
    _Pragma("unroll") for (int i = 0; i < 4; i++) o[i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)k[i], CTRL, 0xF, 0xF, false); \
    _Pragma("unroll") for (int i = 0; i < 4; i++) k[i] = min(k[i], o[3 - i]);                                   \
    sort4(k);                                                                                                   \
  }
  DVM_TOP4_STEP(0xB1)    // quad_perm [1,0,3,2]
  DVM_TOP4_STEP(0x4E)    // quad_perm [2,3,0,1]
  DVM_TOP4_STEP(0x141)   // row_half_mirror
  DVM_TOP4_STEP(0x140)   // row_mirror
#undef DVM_TOP4_STEP
  if (lane < 4) {
    uint32_t mine = k[0];
#pragma unroll
    for (int i = 1; i < 4; i++) mine = lane == i ? k[i] : mine;
    const uint32_t d = mine >> 16;
    ranked[(size_t)q * 4 + lane] = d < 256 ? ((d << 16) | (uint32_t)F.sidx[mine & 0xFFFFu]) : (256u << 16);
  }
}

// Best / second-best over an EXPLICIT candidate list per query (CSR: cand[off[q] .. off[q+1]) in the
// reference's scan order).  This is the inner loop of the vocabulary-node restricted searches --
// ORBmatcher::SearchByBoW (reference src/ORBmatcher.cc:262-300,:760-800), SearchForTriangulation
// (:905-960), SearchBySim3, Fuse -- whose candidate enumeration (DBoW2 FeatureVector walk, epipolar /
// chi2 gates) stays with the caller.  Strict '<' first-wins ties == min over (dist << 20 | position).
__global__ void __launch_bounds__(256) k_match_lists(const uint8_t* __restrict__ tdesc, const uint8_t* __restrict__ qdesc,
                                                     const int32_t* __restrict__ off, const int32_t* __restrict__ cand,
                                                     int nq, dvm_match_pod* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  uint32_t w[8];
  desc_load(qdesc, q, w);
  const int beg = off[q], end = off[q + 1];
  unsigned long long k1 = (256ull << 32) | 0xFFFFFFFFull, k2 = k1;
  for (int p = beg + lane; p < end; p += 64) {
    const int idx = cand[p];
    if (idx < 0) continue;  // caller-masked candidate
    const unsigned long long k = ((unsigned long long)desc_distance(w, tdesc, idx) << 32) | (unsigned)(p - beg);
    if (k < k1) { k2 = k1; k1 = k; } else if (k < k2) k2 = k;     // (64-bit keys: the branch is cheaper than top2_insert's min / max)
  }
  wave_top2(k1, k2);
  if (lane == 0) {
    dvm_match_pod m;
    m.best_dist = (int)(k1 >> 32);
    m.second_dist = (int)(k2 >> 32);
    m.best_idx = m.best_dist < 256 ? cand[beg + (int)(k1 & 0xFFFFFFFFu)] : -1;
    m.best_level = -1;
    m.second_level = -1;
    out[q] = m;
  }
}

// Projection of map points into a keyframe + windowed best-descriptor search: the common body of ORBmatcher::Fuse(KF, MPs)
// (reference src/ORBmatcher.cc:1060-1234), Fuse(KF, Scw, ...) (:1236-1345), SearchByProjection(KF, Scw, ...) x2 (:395-603)
// -- depth > 0, KeyFrame::IsInImage, distance inside the scale-invariance range, viewing angle < 60 deg
// (PO.Pn >= 0.5 dist), MapPoint::PredictScale, radius = th * scaleFactor[level], candidates of octave [level-1, level],
// optional per-candidate chi2 gate (Fuse).  One DPP row (16 lanes) per map point; every lane repeats the projection.
// MODEL: the camera behind pCamera->project (project_row<MODEL>); kb8 = mvParameters for KannalaBrandt8, unused for the pinhole camera.
template <int MODEL>
__device__ __forceinline__ void project_search_row(const FrameView& FB, int slot, const uint8_t* __restrict__ skip, const ProjectCam& C,
                                                   const float* kb8, const float* __restrict__ P, const float* __restrict__ normal,
                                                   const float* __restrict__ min_dist, const float* __restrict__ max_dist,
                                                   const uint8_t* __restrict__ desc, const uint8_t* __restrict__ valid, int n,
                                                   const float* __restrict__ scale_factors, const float* __restrict__ gate_inv_sigma2,
                                                   double gate, dvm_match_pod* __restrict__ out, Projection* __restrict__ proj) {
  const int lane = threadIdx.x & 15;
  const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
  if (i >= n) return;
  const FrameView F = FB.slot(slot);
  const ProjectRow R = project_row<MODEL>(F, skip, C, C.th, P, normal, min_dist, max_dist, desc, valid == nullptr || valid[i] != 0, i, scale_factors,
                                          gate_inv_sigma2, gate, lane, kb8);
  const uint32_t k1 = R.k1, k2 = R.k2;
  if (lane == 0) {
    dvm_match_pod m;
    const int p1i = (int)(k1 & 0xFFFFu), p2i = (int)(k2 & 0xFFFFu);
    m.best_dist = (int)(k1 >> 16);
    m.second_dist = (int)(k2 >> 16);
    m.best_idx = (m.best_dist < 256) ? F.sidx[p1i] : -1;
    m.best_level = (m.best_dist < 256) ? (int16_t)__float_as_int(F.skp[p1i].z) : (int16_t)-1;
    m.second_level = (m.second_dist < 256) ? (int16_t)__float_as_int(F.skp[p2i].z) : (int16_t)-1;
    out[i] = m;
    if (proj) {
      Projection pr;
      pr.u = R.u; pr.v = R.v; pr.radius = R.r; pr.level = R.level;
      proj[i] = pr;
    }
  }
}
__global__ void __launch_bounds__(256) k_project_search(FrameView FB, int slot, const uint8_t* __restrict__ skip, ProjectCam C,
                                                        const float* __restrict__ P, const float* __restrict__ normal,
                                                        const float* __restrict__ min_dist, const float* __restrict__ max_dist,
                                                        const uint8_t* __restrict__ desc, const uint8_t* __restrict__ valid, int n,
                                                        const float* __restrict__ scale_factors,
                                                        const float* __restrict__ gate_inv_sigma2, double gate,
                                                        dvm_match_pod* __restrict__ out, Projection* __restrict__ proj) {
  project_search_row<dvm_cam::kPinhole>(FB, slot, skip, C, nullptr, P, normal, min_dist, max_dist, desc, valid, n, scale_factors, gate_inv_sigma2, gate, out, proj);
}
// the same with pCamera->project of a KannalaBrandt8 camera (dvm_project_search_cam, model 1)
__global__ void __launch_bounds__(256) k_project_search_kb8(FrameView FB, int slot, const uint8_t* __restrict__ skip, ProjectCam C, CamParams K,
                                                            const float* __restrict__ P, const float* __restrict__ normal,
                                                            const float* __restrict__ min_dist, const float* __restrict__ max_dist,
                                                            const uint8_t* __restrict__ desc, const uint8_t* __restrict__ valid, int n,
                                                            const float* __restrict__ scale_factors,
                                                            const float* __restrict__ gate_inv_sigma2, double gate,
                                                            dvm_match_pod* __restrict__ out, Projection* __restrict__ proj) {
  project_search_row<dvm_cam::kKannalaBrandt8>(FB, slot, skip, C, K.p, P, normal, min_dist, max_dist, desc, valid, n, scale_factors, gate_inv_sigma2, gate, out,
                                               proj);
}

// ORBmatcher::SearchForTriangulation inner loop (reference src/ORBmatcher.cc:905-998, monocular): query q = keypoint
// qidx[q] of KF1 scans KF2 keypoints cand[off[q] .. off[q+1]) (its vocabulary node's features that are neither matched
// nor carry a map point); a candidate is taken if dist <= TH_LOW, dist <= the best so far, it is not within
// 100*scaleFactor[octave] (squared px) of the epipole, and (bCoarse or) Pinhole::epipolarConstrain holds
// (CameraModels/Pinhole.cpp:104-127).  The reference never sets vbMatched2, so queries are independent; within a query the
// sequential rule "<= replaces" is "minimum distance, LAST position wins a tie" = min over (dist << 16 | 0xFFFF - pos).
__global__ void __launch_bounds__(256) k_match_triangulation(const uint8_t* __restrict__ desc1, const dvm_keypoint_pod* __restrict__ kps1,
                                                             const int32_t* __restrict__ qidx, int nq,
                                                             const uint8_t* __restrict__ desc2, const dvm_keypoint_pod* __restrict__ kps2,
                                                             const int32_t* __restrict__ off, const int32_t* __restrict__ cand, TriGeom G,
                                                             const float* __restrict__ scale_factors2,
                                                             const float* __restrict__ level_sigma2_2, int32_t* __restrict__ best_idx,
                                                             int32_t* __restrict__ best_dist) {
  const int lane = threadIdx.x & 15;
  const int q = blockIdx.x * 16 + (threadIdx.x >> 4);
  if (q >= nq) return;
  const TriQuery Q = tri_query(desc1, kps1, qidx[q], G.F12);
  const int beg = off[q], end = off[q + 1];
  uint32_t k = 0xFFFFFFFFu;
  for (int p = beg + lane; p < end; p += 16) {
    const int idx2 = cand[p];
    if (idx2 < 0) continue;
    const int d = tri_candidate(Q, desc2, kps2, idx2, G, scale_factors2, level_sigma2_2);
    if (d < 0) continue;
    k = min(k, tri_key(d, p - beg));
  }
  k = row_min(k);
  if (lane == 0) {
    const bool hit = k != 0xFFFFFFFFu;
    best_idx[q] = hit ? cand[beg + tri_key_pos(k)] : -1;
    best_dist[q] = hit ? (int)(k >> 16) : 256;
  }
}

// k_match_triangulation on a KannalaBrandt8 pair (dvm_match_triangulation_cam, model 1): the candidate test is
// KannalaBrandt8::epipolarConstrain, run over the workgroup's survivors of the two cheap tests (tri_rows_kb8, tri_device.h).  A candidate
// whose octave lies outside the tables is no candidate.
__global__ void __launch_bounds__(256) k_match_triangulation_kb8(const uint8_t* __restrict__ desc1, const dvm_keypoint_pod* __restrict__ kps1,
                                                                 const int32_t* __restrict__ qidx, int nq,
                                                                 const uint8_t* __restrict__ desc2, const dvm_keypoint_pod* __restrict__ kps2,
                                                                 const int32_t* __restrict__ off, const int32_t* __restrict__ cand, TriGeomKB8 G,
                                                                 const float* __restrict__ level_sigma2_1, const float* __restrict__ scale_factors2,
                                                                 const float* __restrict__ level_sigma2_2, int n_levels,
                                                                 int32_t* __restrict__ best_idx, int32_t* __restrict__ best_dist) {
  __shared__ TriBlockKB8 S;
  const int lane = threadIdx.x & 15;
  const int q = blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool active = q < nq;
  const int beg = active ? off[q] : 0, end = active ? off[q + 1] : 0;
  const uint32_t k = tri_rows_kb8(S, active, desc1, kps1, active ? qidx[q] : 0, beg, end, [&](int p) { return cand[p]; }, desc2, kps2, G, level_sigma2_1,
                                  scale_factors2, level_sigma2_2, n_levels);
  if (lane == 0 && active) {
    const bool hit = k != 0xFFFFFFFFu;
    best_idx[q] = hit ? cand[beg + tri_key_pos(k)] : -1;
    best_dist[q] = hit ? (int)(k >> 16) : 256;
  }
}

// KeyFrameDatabase place-recognition queries (reference src/KeyFrameDatabase.cc:224-808: DetectCandidates,
// DetectNBestCandidates, CalculateMergeScore) walk an inverted file word -> keyframes to count, per keyframe, the words it
// shares with the query BowVector, then score the survivors with L1Scoring::score (DBoW2/ScoringObject.cpp:23-63).
// A keyframe is in the inverted list of a word iff its BowVector holds the word, so the count is |ids(query) n ids(kf)| and
// the position of a keyframe in lKFsSharingWords is ordered by (first shared word, insertion order): one wave per stored
// keyframe intersects its sorted word list with the query's (binary search per word) and produces count, first shared
// word and the score for ALL keyframes at once -- no inverted file on the device.  The double sum of the score is taken
// in ascending word order (the reference's merge walk) by walking the hit mask of each 64-word chunk.
__global__ void __launch_bounds__(256) k_bowdb_query(const int64_t* __restrict__ kf_off, const int32_t* __restrict__ kf_len,
                                                     const int32_t* __restrict__ live, int n_live,
                                                     const int32_t* __restrict__ ids_base, const double* __restrict__ vals_base,
                                                     const int32_t* __restrict__ qids, const double* __restrict__ qvals, int nq,
                                                     int32_t* __restrict__ common, int32_t* __restrict__ first_word,
                                                     float* __restrict__ score) {
  const int lane = threadIdx.x & 63;
  const int li = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (li >= n_live) return;
  const int kf = live[li];                         // erased slots are not launched (their results are preset by the host)
  const int len = kf_len[kf];
  const int32_t* __restrict__ ids = ids_base + kf_off[kf];
  const double* __restrict__ vals = vals_base + kf_off[kf];
  constexpr int off = 0;
  int n_common = 0, first = -1;
  double acc = 0.0;
  for (int base = 0; base < len; base += 64) {
    const int p = base + lane;
    bool hit = false;
    double term = 0.0;
    if (p < len) {
      const int id = ids[off + p];
      int lo = 0, hi = nq;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (qids[mid] < id) lo = mid + 1; else hi = mid;
      }
      if (lo < nq && qids[lo] == id) {
        hit = true;
        const double vi = qvals[lo], wi = vals[off + p];   // score(v1 = query, v2 = keyframe)
        term = fabs(vi - wi) - fabs(vi) - fabs(wi);
      }
    }
    unsigned long long mask = __ballot(hit);
    if (mask != 0ull && first < 0) first = ids[off + base + (int)__builtin_ctzll(mask)];
    n_common += __builtin_popcountll(mask);
    while (mask) {
      const int l = (int)__builtin_ctzll(mask);
      const int lo32 = __builtin_amdgcn_readlane(__double2loint(term), l), hi32 = __builtin_amdgcn_readlane(__double2hiint(term), l);
      acc += __hiloint2double(hi32, lo32);
      mask &= mask - 1;
    }
  }
  if (lane == 0) {
    common[kf] = len < 0 ? -1 : n_common;
    first_word[kf] = first;
    score[kf] = (float)(-acc / 2.0);
  }
}

// Frame::isInFrustum, mono branch (reference src/Frame.cc:575-636) + MapPoint::PredictScale
// (src/MapPoint.cc:573-587): thread per map point, float arithmetic in the reference's order (frustum_point.h).
// MODEL: the camera behind mpCamera->project; kb8 = mvParameters for KannalaBrandt8, unused for the pinhole camera.
template <int MODEL>
__device__ __forceinline__ void is_in_frustum_thread(const FrustumFrame& F, const float* kb8, const float* __restrict__ P, const float* __restrict__ normal,
                                                     const float* __restrict__ min_dist, const float* __restrict__ max_dist, int n, float cos_limit,
                                                     TrackPoint* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = frustum_point<MODEL>(F, P[3 * i], P[3 * i + 1], P[3 * i + 2], normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], min_dist[i], max_dist[i],
                                cos_limit, kb8);
}
__global__ void __launch_bounds__(256) k_is_in_frustum(FrustumFrame F, const float* __restrict__ P, const float* __restrict__ normal,
                                                       const float* __restrict__ min_dist, const float* __restrict__ max_dist,
                                                       int n, float cos_limit, TrackPoint* __restrict__ out) {
  is_in_frustum_thread<dvm_cam::kPinhole>(F, nullptr, P, normal, min_dist, max_dist, n, cos_limit, out);
}
// the same with mpCamera->project of a KannalaBrandt8 camera (dvm_is_in_frustum_cam, model 1)
__global__ void __launch_bounds__(256) k_is_in_frustum_kb8(FrustumFrame F, CamParams K, const float* __restrict__ P, const float* __restrict__ normal,
                                                           const float* __restrict__ min_dist, const float* __restrict__ max_dist,
                                                           int n, float cos_limit, TrackPoint* __restrict__ out) {
  is_in_frustum_thread<dvm_cam::kKannalaBrandt8>(F, K.p, P, normal, min_dist, max_dist, n, cos_limit, out);
}

// LocalMapping::CreateNewMapPoints, the geometry of one neighbour keyframe's matches (reference src/LocalMapping.cc:598-741, monocular
// pinhole branch; GeometricTools::Triangulate src/GeometricTools.cc:48-67): thread per match.  Parallax of the two rays, the
// homogeneous point (null vector of the 4x4 system: eigenvector of the smallest eigenvalue of A^T A by cyclic Jacobi in double --
// the reference runs Eigen::JacobiSVD<Matrix4f>, tolerance parity), depth, reprojection error and scale-consistency tests in float
// in Eigen's evaluation order, comparisons with double literals in double.  status: include/dvmslam_hip.h.
// MODEL: tri_pair_geometry<MODEL>; for KannalaBrandt8 (dvm_triangulate_matches_cam, model 1) the rays come from kb8_unproject and both
// reprojections go through kb8_project on cam1 / cam2, and P.K1 / P.K2 are not read.
template <int MODEL>
__device__ __forceinline__ void triangulate_match_thread(const TriPair& P, const float* cam1, const float* cam2, const dvm_keypoint_pod* __restrict__ kps1,
                                                         int n1, const dvm_keypoint_pod* __restrict__ kps2, int n2, const int32_t* __restrict__ pairs,
                                                         int n, const float* __restrict__ sigma2_1, const float* __restrict__ sigma2_2,
                                                         const float* __restrict__ sf1, const float* __restrict__ sf2, float* __restrict__ x3D_out,
                                                         int32_t* __restrict__ status) {
  const int m = blockIdx.x * 128 + threadIdx.x;
  if (m >= n) return;
  float* X = x3D_out + 3 * (int64_t)m;
  const int i1 = pairs[2 * m], i2 = pairs[2 * m + 1];
  if (i1 < 0 || i1 >= n1 || i2 < 0 || i2 >= n2) { X[0] = X[1] = X[2] = 0.0f; status[m] = -1; return; }
  float x[3];
  status[m] = tri_pair_geometry<MODEL>(P, kps1[i1], kps2[i2], sigma2_1, sigma2_2, sf1, sf2, x, cam1, cam2);
  X[0] = x[0]; X[1] = x[1]; X[2] = x[2];
}
__global__ void __launch_bounds__(128) k_triangulate_matches(TriPair P, const dvm_keypoint_pod* __restrict__ kps1, int n1,
                                                             const dvm_keypoint_pod* __restrict__ kps2, int n2,
                                                             const int32_t* __restrict__ pairs, int n, const float* __restrict__ sigma2_1,
                                                             const float* __restrict__ sigma2_2, const float* __restrict__ sf1,
                                                             const float* __restrict__ sf2, float* __restrict__ x3D_out,
                                                             int32_t* __restrict__ status) {
  triangulate_match_thread<dvm_cam::kPinhole>(P, nullptr, nullptr, kps1, n1, kps2, n2, pairs, n, sigma2_1, sigma2_2, sf1, sf2, x3D_out, status);
}
__global__ void __launch_bounds__(128) k_triangulate_matches_kb8(TriPair P, CamParams C1, CamParams C2, const dvm_keypoint_pod* __restrict__ kps1, int n1,
                                                                 const dvm_keypoint_pod* __restrict__ kps2, int n2,
                                                                 const int32_t* __restrict__ pairs, int n, const float* __restrict__ sigma2_1,
                                                                 const float* __restrict__ sigma2_2, const float* __restrict__ sf1,
                                                                 const float* __restrict__ sf2, float* __restrict__ x3D_out,
                                                                 int32_t* __restrict__ status) {
  triangulate_match_thread<dvm_cam::kKannalaBrandt8>(P, C1.p, C2.p, kps1, n1, kps2, n2, pairs, n, sigma2_1, sigma2_2, sf1, sf2, x3D_out, status);
}
void launch_triangulate_matches(hipStream_t s, const TriPair& P, const dvm_keypoint_pod* kps1, int n1, const dvm_keypoint_pod* kps2, int n2,
                                const int32_t* pairs, int n, const float* sigma2_1, const float* sigma2_2, const float* sf1,
                                const float* sf2, float* x3D, int32_t* status) {
  hipLaunchKernelGGL(k_triangulate_matches, dim3((n + 127) / 128), dim3(128), 0, s, P, kps1, n1, kps2, n2, pairs, n, sigma2_1, sigma2_2, sf1, sf2,
                     x3D, status);
}

void launch_triangulate_matches_kb8(hipStream_t s, const TriPair& P, const CamParams& C1, const CamParams& C2, const dvm_keypoint_pod* kps1, int n1,
                                    const dvm_keypoint_pod* kps2, int n2, const int32_t* pairs, int n, const float* sigma2_1, const float* sigma2_2,
                                    const float* sf1, const float* sf2, float* x3D, int32_t* status) {
  hipLaunchKernelGGL(k_triangulate_matches_kb8, dim3((n + 127) / 128), dim3(128), 0, s, P, C1, C2, kps1, n1, kps2, n2, pairs, n, sigma2_1, sigma2_2, sf1,
                     sf2, x3D, status);
}

// D[i][j] = Hamming(A[i], B[j]); one thread per pair, 64 columns x 4 rows per workgroup.
__global__ void __launch_bounds__(256) k_hamming_matrix(const uint8_t* __restrict__ A, int nA,
                                                        const uint8_t* __restrict__ B, int nB, uint16_t* __restrict__ D) {
  const int j = blockIdx.x * 64 + (threadIdx.x & 63);
  const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i >= nA || j >= nB) return;
  uint32_t w[8];
  desc_load(A, i, w);
  D[(size_t)i * nB + j] = (uint16_t)desc_distance(w, B, j);
}

void launch_frame_build(hipStream_t s, const dvm_keypoint_pod* kps, int64_t kps_stride, const uint8_t* desc,
                        int64_t desc_stride, int n, const int32_t* d_n, const FrameView& F, int first_slot, int count) {
  hipLaunchKernelGGL(k_frame_build, dim3(count), dim3(1024), 0, s, kps, kps_stride, desc, desc_stride, n, d_n, F, first_slot);
}
void launch_match_window(hipStream_t s, const FrameView& F, int slot, const uint8_t* skip, const uint8_t* qdesc,
                         const float* qx, const float* qy, const float* qr, const int32_t* qmin, const int32_t* qmax,
                         int nq, const int32_t* d_nq, int grid_q, dvm_match_pod* out, int32_t* second_idx) {
  PairQueries pq{};
  hipLaunchKernelGGL(k_match_window<false>, dim3((grid_q + 15) / 16, 1), dim3(256), 0, s, F, slot, skip, qdesc, qx, qy, qr,
                     qmin, qmax, nq, d_nq, pq, 0.f, nullptr, 0, out, 0, second_idx);
}
void launch_match_window_ranked(hipStream_t s, const FrameView& F, int slot, const uint8_t* skip, const uint8_t* qdesc, const float* qx,
                                const float* qy, const float* qr, const int32_t* qmin, const int32_t* qmax, int nq, uint32_t* ranked) {
  hipLaunchKernelGGL(k_match_window_ranked, dim3((nq + 15) / 16), dim3(256), 0, s, F, slot, skip, qdesc, qx, qy, qr, qmin, qmax, nq, ranked, 0,
                     nullptr, nullptr, 0, nullptr);
}
void launch_match_window_ranked_batch(hipStream_t s, const FrameView& F, int first_slot, int count, const uint8_t* skip, const int32_t* skip_on,
                                      int skip_stride, const uint8_t* qdesc, const float* qx, const float* qy, const float* qr, const int32_t* qmin,
                                      const int32_t* qmax, const int32_t* nq_arr, int qstride, uint32_t* ranked, const int32_t* qoff) {
  hipLaunchKernelGGL(k_match_window_ranked, dim3((qstride + 15) / 16, count), dim3(256), 0, s, F, first_slot, skip, qdesc, qx, qy, qr, qmin, qmax, 0,
                     ranked, qstride, nq_arr, skip_on, skip_stride, qoff);
}
void launch_match_frames(hipStream_t s, const FrameView& F, int first_slot, int count, const PairQueries& pq, float th,
                         const float* scale_factors, int nlevels, dvm_match_pod* out, int64_t out_stride) {
  hipLaunchKernelGGL(k_match_window<true>, dim3((pq.cap + 15) / 16, count), dim3(256), 0, s, F, first_slot, nullptr, nullptr,
                     nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, pq, th, scale_factors, nlevels, out, out_stride, nullptr);
}
// Frame::UndistortKeyPoints (Frame.cc:791-818): thread per keypoint, cv::undistortPoints in double (undistort_f64.h)
__global__ void __launch_bounds__(256) k_undistort_keypoints(dvm_undistort::Camera cam, const float* __restrict__ in, float* __restrict__ out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float kp[7];
#pragma unroll
  for (int k = 0; k < 7; k++) kp[k] = in[7 * (int64_t)i + k];
  if (cam.k1 != 0.0f) dvm_undistort::undistort_point(cam, kp[0], kp[1], &kp[0], &kp[1]);
#pragma unroll
  for (int k = 0; k < 7; k++) out[7 * (int64_t)i + k] = kp[k];
}
void launch_undistort_keypoints(hipStream_t s, const dvm_undistort::Camera& cam, const float* in, float* out, int n) {
  hipLaunchKernelGGL(k_undistort_keypoints, dim3((n + 255) / 256), dim3(256), 0, s, cam, in, out, n);
}

void launch_is_in_frustum(hipStream_t s, const FrustumFrame& F, const float* P, const float* normal, const float* min_dist,
                          const float* max_dist, int n, float cos_limit, TrackPoint* out) {
  hipLaunchKernelGGL(k_is_in_frustum, dim3((n + 255) / 256), dim3(256), 0, s, F, P, normal, min_dist, max_dist, n, cos_limit, out);
}
void launch_is_in_frustum_kb8(hipStream_t s, const FrustumFrame& F, const CamParams& K, const float* P, const float* normal, const float* min_dist,
                              const float* max_dist, int n, float cos_limit, TrackPoint* out) {
  hipLaunchKernelGGL(k_is_in_frustum_kb8, dim3((n + 255) / 256), dim3(256), 0, s, F, K, P, normal, min_dist, max_dist, n, cos_limit, out);
}
void launch_project_search_kb8(hipStream_t s, const FrameView& F, int slot, const uint8_t* skip, const ProjectCam& C, const CamParams& K, const float* P,
                               const float* normal, const float* min_dist, const float* max_dist, const uint8_t* desc,
                               const uint8_t* valid, int n, const float* scale_factors, const float* gate_inv_sigma2, double gate,
                               dvm_match_pod* out, Projection* proj) {
  hipLaunchKernelGGL(k_project_search_kb8, dim3((n + 15) / 16), dim3(256), 0, s, F, slot, skip, C, K, P, normal, min_dist, max_dist, desc,
                     valid, n, scale_factors, gate_inv_sigma2, gate, out, proj);
}
void launch_match_lists(hipStream_t s, const uint8_t* tdesc, const uint8_t* qdesc, const int32_t* off, const int32_t* cand,
                        int nq, dvm_match_pod* out) {
  hipLaunchKernelGGL(k_match_lists, dim3((nq + 3) / 4), dim3(256), 0, s, tdesc, qdesc, off, cand, nq, out);
}
void launch_project_search(hipStream_t s, const FrameView& F, int slot, const uint8_t* skip, const ProjectCam& C, const float* P,
                           const float* normal, const float* min_dist, const float* max_dist, const uint8_t* desc,
                           const uint8_t* valid, int n, const float* scale_factors, const float* gate_inv_sigma2, double gate,
                           dvm_match_pod* out, Projection* proj) {
  hipLaunchKernelGGL(k_project_search, dim3((n + 15) / 16), dim3(256), 0, s, F, slot, skip, C, P, normal, min_dist, max_dist, desc,
                     valid, n, scale_factors, gate_inv_sigma2, gate, out, proj);
}
void launch_match_triangulation(hipStream_t s, const uint8_t* desc1, const dvm_keypoint_pod* kps1, const int32_t* qidx, int nq,
                                const uint8_t* desc2, const dvm_keypoint_pod* kps2, const int32_t* off, const int32_t* cand,
                                const TriGeom& G, const float* scale_factors2, const float* level_sigma2_2, int32_t* best_idx,
                                int32_t* best_dist) {
  hipLaunchKernelGGL(k_match_triangulation, dim3((nq + 15) / 16), dim3(256), 0, s, desc1, kps1, qidx, nq, desc2, kps2, off, cand, G,
                     scale_factors2, level_sigma2_2, best_idx, best_dist);
}
void launch_match_triangulation_kb8(hipStream_t s, const uint8_t* desc1, const dvm_keypoint_pod* kps1, const int32_t* qidx, int nq,
                                    const uint8_t* desc2, const dvm_keypoint_pod* kps2, const int32_t* off, const int32_t* cand,
                                    const TriGeomKB8& G, const float* level_sigma2_1, const float* scale_factors2, const float* level_sigma2_2,
                                    int n_levels, int32_t* best_idx, int32_t* best_dist) {
  hipLaunchKernelGGL(k_match_triangulation_kb8, dim3((nq + 15) / 16), dim3(256), 0, s, desc1, kps1, qidx, nq, desc2, kps2, off, cand, G,
                     level_sigma2_1, scale_factors2, level_sigma2_2, n_levels, best_idx, best_dist);
}
void launch_bowdb_query(hipStream_t s, const int64_t* kf_off, const int32_t* kf_len, const int32_t* live, int n_live, const int32_t* ids,
                        const double* vals, const int32_t* qids, const double* qvals, int nq, int32_t* common, int32_t* first_word, float* score) {
  if (n_live > 0)
    hipLaunchKernelGGL(k_bowdb_query, dim3((n_live + 3) / 4), dim3(256), 0, s, kf_off, kf_len, live, n_live, ids, vals, qids, qvals, nq,
                       common, first_word, score);
}
void launch_hamming_matrix(hipStream_t s, const uint8_t* A, int nA, const uint8_t* B, int nB, uint16_t* D) {
  hipLaunchKernelGGL(k_hamming_matrix, dim3((nB + 63) / 64, (nA + 3) / 4), dim3(256), 0, s, A, nA, B, nB, D);
}

// MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:384-453), batched over map points: point p owns
// the descriptors desc[off[p] .. off[p+1]) (its observations, in the reference's iteration order).  For every row i of
// the N x N Hamming table the median is vDists[0.5 * (N - 1)] of the SORTED row (self distance 0 included); the
// winner is the first i with the strictly smallest median.  One wavefront per map point: descriptors staged in LDS,
// row i = one distance per lane (chunks of 64), the k-th order statistic by a 9-step binary search over the value
// range [0, 256] with ballot counts -- no sort (distinctive_lds, match_device.h).  Points with more than kDistinctMaxN observations report -2.
__global__ void __launch_bounds__(64) k_distinctive(const uint8_t* __restrict__ desc, const int32_t* __restrict__ off, int npts,
                                                    int32_t* __restrict__ best_idx, int32_t* __restrict__ best_median) {
  __shared__ uint32_t s_desc[kDistinctMaxN * 8];
  __shared__ uint16_t s_row[kDistinctMaxN];
  const int p = blockIdx.x, lane = threadIdx.x;
  if (p >= npts) return;
  const int o0 = off[p], N = off[p + 1] - o0;
  if (N <= 0) { if (lane == 0) { best_idx[p] = -1; best_median[p] = -1; } return; }
  if (N > kDistinctMaxN) { if (lane == 0) { best_idx[p] = -2; best_median[p] = -2; } return; }
  const uint32_t* g = reinterpret_cast<const uint32_t*>(desc + (size_t)o0 * 32);
  for (int i = lane; i < N * 8; i += 64) s_desc[i] = g[i];
  __syncthreads();
  const uint32_t best = distinctive_lds(s_desc, s_row, N, lane);   // median << 16 | i
  if (lane == 0) { best_idx[p] = (int)(best & 0xFFFFu); best_median[p] = (int)(best >> 16); }
}
void launch_distinctive(hipStream_t s, const uint8_t* desc, const int32_t* off, int npts, int32_t* best_idx, int32_t* best_median) {
  if (npts > 0) hipLaunchKernelGGL(k_distinctive, dim3(npts), dim3(64), 0, s, desc, off, npts, best_idx, best_median);
}

// DBoW2 TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup) (reference
// Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1098-1138): walk the vocabulary tree from the root, at every node take
// the child with the smallest FORB::distance (first child wins ties: strict '<' scan), remember the node reached at
// level L - levelsup.  One DPP row (16 lanes) per feature: lane c scores child c (k = 10 in ORBvoc), the argmin of
// (distance << 16 | child position) is four DPP steps.  Nodes: CSR children lists, 32-B descriptors, weight, word id.
__global__ void __launch_bounds__(256) k_vocab_transform(const int32_t* __restrict__ child_off, const int32_t* __restrict__ children,
                                                         const uint8_t* __restrict__ node_desc, const double* __restrict__ weight,
                                                         const int32_t* __restrict__ word_id, int L, const uint8_t* __restrict__ feat,
                                                         int n, int levelsup, int32_t* __restrict__ out_word,
                                                         int32_t* __restrict__ out_node, double* __restrict__ out_weight,
                                                         const int32_t* __restrict__ d_n, const int32_t* __restrict__ run,
                                                         int64_t feat_stride) {
  const int lane = threadIdx.x & 15;
  const int f = blockIdx.x * 16 + (threadIdx.x >> 4);
  if (run) {     // a batch: frame run[blockIdx.y], its features at b * feat_stride bytes, its outputs and count at b * n / b
    const int b = run[blockIdx.y];
    feat += (size_t)b * feat_stride; out_word += (size_t)b * n; out_node += (size_t)b * n; out_weight += (size_t)b * n; d_n += b;
  }
  if (d_n) n = min(n, *d_n);     // (a count still on the device: n is then the capacity the grid covers)
  if (f >= n) return;
  uint32_t w[8];
  desc_load(feat, f, w);
  const int nid_level = L - levelsup;
  int nid = nid_level <= 0 ? 0 : -1;   // the reference leaves *nid unset if the walk ends above nid_level
  int cur = 0, level = 0;
  int c0 = child_off[0], c1 = child_off[1];
  while (c1 > c0) {
    ++level;
    uint32_t best = 0xFFFFFFFFu;
    for (int base = c0; base < c1; base += 16) {
      const int c = base + lane;
      uint32_t key = 0xFFFFFFFFu;
      if (c < c1) key = ((uint32_t)desc_distance(w, node_desc, children[c]) << 16) | (uint32_t)(c - c0);
      best = min(best, key);
    }
    best = row_min(best);
    cur = children[c0 + (int)(best & 0xFFFFu)];
    if (level == nid_level) nid = cur;
    c0 = child_off[cur]; c1 = child_off[cur + 1];
  }
  if (lane == 0) { out_word[f] = word_id[cur]; out_node[f] = nid; out_weight[f] = weight[cur]; }
}
void launch_vocab_transform(hipStream_t s, const int32_t* child_off, const int32_t* children, const uint8_t* node_desc,
                            const double* weight, const int32_t* word_id, int L, const uint8_t* feat, int n, int levelsup,
                            int32_t* out_word, int32_t* out_node, double* out_weight, const int32_t* d_n, const int32_t* run, int nrun,
                            int64_t feat_stride) {
  if (n > 0 && nrun > 0)
    hipLaunchKernelGGL(k_vocab_transform, dim3((n + 15) / 16, run ? nrun : 1), dim3(256), 0, s, child_off, children, node_desc, weight, word_id, L,
                       feat, n, levelsup, out_word, out_node, out_weight, d_n, run, feat_stride);
}

}  // namespace dvm
