// dvm_slam_amd/csrc/track_kernels.hip -- the device side of dvm_track_begin / dvm_track_finish (include/dvmslam_hip.h): what the
// reference's Tracking::TrackWithMotionModel does between the window search and the pose it ends on, as kernels of ONE stream chain
// behind the extraction of the frame (no host step in between):
//   k_track_claims   ORBmatcher::SearchByProjection(CurrentFrame, LastFrame): the sequential epilogue of src/ORBmatcher.cc:1613-1664
//                    (a keypoint taken by an earlier query is skipped by the later ones) and the rotation histogram :1652-1663,
//                    :1730-1745, replayed from the ranked candidate lists of k_match_window_ranked
//   k_track_gather   Optimizer::PoseOptimization's edge list (src/Optimizer.cc:768-838): the matched keypoints in keypoint order
//   k_track_finish   the outlier flags back in keypoint order, Tracking.cc:2636-2660 (outlier matches dropped, nmatchesMap)
// The pose itself is k_pose_optimize (pose_kernels.hip), launched between the last two.
// The second half, Tracking::TrackLocalMap (dvm_track_local_map), runs on the grid and mvKeysUn the first half left:
//   k_track_local_prologue  SearchLocalPoints (Tracking.cc:3041-3106) up to the matcher's queries
//   k_track_claims<true>    SearchByProjection(F, vpMapPoints)'s epilogue (ORBmatcher.cc:75-131)
// followed by k_track_gather, k_pose_optimize and k_track_finish as in the first half.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_sort.h"
#include "frustum_point.h"
#include "match_device.h"
#include "match_kernels.h"
#include "pose_f32.h"
#include "rot_bin.h"
#include "track_kernels.h"

namespace dvm {

namespace {
constexpr int kHisto = kRotHisto;   // HISTO_LENGTH, ORBmatcher.cc:38 (three_maxima: rot_bin.h)
}

// One wave.  Queries are decided in blocks of 64, one per lane.  Inside a block a lane's choice depends on what the lanes before it
// take: every round each undecided lane proposes its first candidate that is still free; a lane whose proposal is also proposed by
// an EARLIER undecided lane that will take it (owner[] = smallest such lane) is blocked; the lanes in front of the first blocked lane
// are final and commit, the rest propose again.  The first undecided lane is never blocked, so every round commits at least one.
//   ranked[q][0..3]  dist << 16 | keypoint, best first, dist >= 256 = end of the list (k_match_window_ranked)
//   q_claims[q]      the query's map point has Observations() > 0: its match takes the keypoint (:1620-1622)
//   q_angle[q]       LastFrame.mvKeysUn[i].angle
//   RQ               the grid the lists were ranked on and the query arrays: a query that finds all four ranked candidates taken while
//                    its list may go on has its window scanned again by the whole wave at its turn (on the dense bench stream
//                    about one query in 60: every frame has some)
// Outputs: assign[j] = the query matched to keypoint j at the end of the call or -1; res[0] = nmatches, res[1] = 1 if such a query could
// not be searched again here (RQ.F.skp == nullptr: the caller then repeats the epilogue on the host), res[2] = matches before the
// rotation check, res[3] = queries searched again.
// blockIdx.x = frame of a batch (dvm_track_finish_batch: K agents' frames in one chain): frame b's per-query arrays lie at b * B.qstride
// elements, its keypoints at b * B.kps_stride, its grid in slot b, its results at b * kp_cap / b * 8; a single frame is the batch of one.
// kLocal: the same replay for SearchByProjection(F, vpMapPoints) of the second half (ORBmatcher.cc:75-131, dvm_track_local_map): no
// rotation check; the ratio test (best > nnratio * second, both on one level) needs the best AND the second free candidate, so a lane
// takes the first two free entries of its list, a query with fewer than two free among four whose list may go on has its window scanned
// again (best two by (distance, scan position)), and a lane waits while an earlier lane of its round takes either of the two.  The
// keypoints whose frame point has Observations() > 0 start taken (LQ.skip).  Per-query state stays in global memory (the next block's
// lists are loaded while the current one is decided): the number of points in view is not bounded by LDS.  LDS: 10 B per keypoint.
template <bool kLocal>
__global__ void __launch_bounds__(256) k_track_claims(const uint32_t* __restrict__ ranked, const uint8_t* __restrict__ q_claims,
                                                      const float* __restrict__ q_angle, int nq, TrackRequery RQ, const dvm_keypoint_pod* __restrict__ kps,
                                                      const int32_t* __restrict__ d_n, int kp_cap, int th_high, int check_ori, float nnratio,
                                                      LocalQueries LQ, int32_t* __restrict__ assign, int32_t* __restrict__ res,
                                                      int32_t* __restrict__ assign_host, int32_t* __restrict__ res_host, TrackBatch B) {
  extern __shared__ __attribute__((aligned(16))) uint8_t track_smem[];
  {
    const int b = blockIdx.x;
    if (B.nq_arr) nq = B.nq_arr[b];
    const size_t qo = B.qo(b);
    ranked += qo * 4; q_claims += qo; q_angle += qo;
    RQ.qdesc += qo * 32; RQ.qx += qo; RQ.qy += qo; RQ.qr += qo; RQ.qmin += qo; RQ.qmax += qo;
    if (RQ.F.skp) RQ.F = RQ.F.slot(b);
    kps += (size_t)b * B.kps_stride; d_n += b;
    assign += (size_t)b * kp_cap; assign_host += (size_t)b * kp_cap; res += 8 * b; res_host += 8 * b;
    if constexpr (kLocal) { LQ.q_tab += qo; LQ.frame_mp += (size_t)b * kp_cap; LQ.skip += (size_t)b * kp_cap; }
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = min(*d_n, kp_cap);
  const int nq_pad = kLocal ? 0 : (nq + 63) & ~63;
  uint4* s_keys = reinterpret_cast<uint4*>(track_smem);                    // [nq_pad] the ranked lists
  int32_t* s_assign = reinterpret_cast<int32_t*>(s_keys + nq_pad);         // [kp_cap]
  uint32_t* s_owner = reinterpret_cast<uint32_t*>(s_assign + kp_cap);      // [kp_cap]
  uint32_t* s_qres = s_owner + kp_cap;                                     // [nq_pad]: keypoint | bin << 16, or 0xFFFFFFFF
  uint8_t* s_claimed = reinterpret_cast<uint8_t*>(s_qres + nq_pad);        // [kp_cap]
  uint8_t* s_qcl = s_claimed + kp_cap;                                     // [nq_pad] the query takes its keypoint
  int8_t* s_oct = reinterpret_cast<int8_t*>(s_claimed + kp_cap);           // kLocal: [kp_cap] octave of each keypoint
  __shared__ int s_rot[kHisto];
  __shared__ int s_ind[3];
  __shared__ int s_cnt[4];
  // ---- parallel prologue (four waves): everything the sequential part reads comes to LDS -- a global load inside a round would put its
  // latency on the chain of ~50 rounds per frame
  if constexpr (kLocal) {
    for (int j = tid; j < kp_cap; j += 256) {
      s_assign[j] = -1; s_owner[j] = 0xFFFFFFFFu;
      s_claimed[j] = j < N ? LQ.skip[j] : 0;
      s_oct[j] = j < N ? (int8_t)kps[j].octave : (int8_t)0;
    }
  } else {
    for (int j = tid; j < kp_cap; j += 256) { s_assign[j] = -1; s_owner[j] = 0xFFFFFFFFu; s_claimed[j] = 0; }
    for (int q = tid; q < nq_pad; q += 256) {
      s_qres[q] = 0xFFFFFFFFu;
      s_keys[q] = q < nq ? *reinterpret_cast<const uint4*>(ranked + 4 * (size_t)q) : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
      s_qcl[q] = q < nq ? q_claims[q] : 0;
    }
  }
  if (tid < kHisto) s_rot[tid] = 0;
  if (tid < 4) s_cnt[tid] = 0;
  __syncthreads();
  // ---- sequential part: wave 0 alone (the other waves wait at the barrier below; inside one wave LDS operations complete in order,
  // so the rounds need no barrier)
  int exhausted_any = 0, n_requeried = 0, n_rounds = 0, n_matched = 0;
  if (wave == 0) {
    const uint4 none4 = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    uint4 next4 = none4;
    uint8_t next_cl = 0;
    if constexpr (kLocal) {
      if (lane < nq) { next4 = *reinterpret_cast<const uint4*>(ranked + 4 * (size_t)lane); next_cl = q_claims[lane]; }
    }
    for (int q0 = 0; q0 < nq; q0 += 64) {
      const int q = q0 + lane;
      bool decided = q >= nq;
      uint4 k4;
      bool claims;
      if constexpr (kLocal) {
        k4 = next4; claims = !decided && next_cl != 0;
        const int qn = q + 64;        // the next block's lists, in flight while this block is decided
        next4 = none4; next_cl = 0;
        if (qn < nq) { next4 = *reinterpret_cast<const uint4*>(ranked + 4 * (size_t)qn); next_cl = q_claims[qn]; }
      } else {
        k4 = s_keys[q];
        claims = !decided && s_qcl[q] != 0;
      }
      const uint32_t key0 = k4.x, key1 = k4.y, key2 = k4.z, key3 = k4.w;   // (selected by compares: an indexed array would live in scratch)
      // list entries: distance >= 256 ends the list; an index >= N cannot occur (the grid holds N keypoints), guarded all the same
      const int i0 = (int)(key0 & 0xFFFFu), i1 = (int)(key1 & 0xFFFFu), i2 = (int)(key2 & 0xFFFFu), i3 = (int)(key3 & 0xFFFFu);
      const bool v0 = (key0 >> 16) < 256u && i0 < N, v1 = v0 && (key1 >> 16) < 256u && i1 < N, v2 = v1 && (key2 >> 16) < 256u && i2 < N,
                 v3 = v2 && (key3 >> 16) < 256u && i3 < N;
      while (__ballot(!decided)) {
        n_rounds++;
        // first candidate of the list no earlier query has taken (the four flags are read side by side: one LDS latency per round)
        const bool f0 = v0 && !s_claimed[v0 ? i0 : 0], f1 = v1 && !s_claimed[v1 ? i1 : 0], f2 = v2 && !s_claimed[v2 ? i2 : 0],
                   f3 = v3 && !s_claimed[v3 ? i3 : 0];
        int prop = -1, pdist = 256, sec = -1, sdist = 256;
        if (!decided) {
          if constexpr (kLocal) {     // the first two free entries: best and second of what is left
            auto put = [&](bool f, int i, uint32_t key) {
              if (!f) return;
              if (prop < 0) { prop = i; pdist = (int)(key >> 16); }
              else if (sec < 0) { sec = i; sdist = (int)(key >> 16); }
            };
            put(f0, i0, key0); put(f1, i1, key1); put(f2, i2, key2); put(f3, i3, key3);
          } else {
            if (f0) { prop = i0; pdist = (int)(key0 >> 16); }
            else if (f1) { prop = i1; pdist = (int)(key1 >> 16); }
            else if (f2) { prop = i2; pdist = (int)(key2 >> 16); }
            else if (f3) { prop = i3; pdist = (int)(key3 >> 16); }
          }
        }
        // all four taken (kLocal: fewer than two free), the list may go on
        bool exhausted = !decided && v3 && (kLocal ? sec < 0 : prop < 0);
        // A query whose four ranked candidates are all taken waits until every query in front of it is final -- it blocks the lanes behind
        // it meanwhile --, then the whole wave scans its window again, skipping what is taken by now: the reference's loop of
        // ORBmatcher.cc:1613-1650 at that query's turn (smallest (distance, scan position) among the free ones)
        const unsigned long long und = __ballot(!decided);
        const int first_und = (int)__builtin_ctzll(und);
        const bool requery = ((__ballot(exhausted) >> first_und) & 1ull) != 0ull;
        if (requery && RQ.F.skp) {
          const int qf = q0 + first_und;
          const float x = RQ.qx[qf], y = RQ.qy[qf], r = RQ.qr[qf];
          const int minLevel = RQ.qmin[qf], maxLevel = RQ.qmax[qf];
          const FrameView& F = RQ.F;
          uint32_t best = (256u << 16) | 0xFFFFu, best2 = best;
          uint32_t w[8];
          desc_load(RQ.qdesc, qf, w);
          window_scan<64>(F, x, y, r, minLevel, maxLevel, lane, [&](int p, int, float, float) {
            const int idx = F.sidx[p];
            if (idx >= N || s_claimed[idx]) return;
            const uint32_t key = ((uint32_t)desc_distance(w, F.sdesc, p) << 16) | (uint32_t)p;
            if constexpr (kLocal) top2_insert(best, best2, key);
            else best = min(best, key);
          });
          if constexpr (kLocal) wave_top2(best, best2);     // best two by (distance, scan position)
          else best = wave_min(best);
          const int bd = (int)(best >> 16);
          const int bidx = bd < 256 ? F.sidx[best & 0xFFFFu] : -1;
          if (lane == first_und) { exhausted = false; pdist = bd; prop = bidx; n_requeried++; }
          if constexpr (kLocal) {
            const int bd2 = (int)(best2 >> 16);
            const int bidx2 = bd2 < 256 ? F.sidx[best2 & 0xFFFFu] : -1;
            if (lane == first_und) { sdist = bd2; sec = bidx2; }
          }
        }
        bool matched = prop >= 0 && pdist <= th_high;
        if constexpr (kLocal) {       // ORBmatcher.cc:100-104: the ratio test only when best and second lie on one level
          const int plev = prop >= 0 ? (int)s_oct[prop] : -1, slev = sec >= 0 ? (int)s_oct[sec] : -1;
          matched = matched && !(plev == slev && (float)pdist > nnratio * (float)sdist);
        }
        const bool takes = matched && claims;
        if (!decided && takes) atomicMin(&s_owner[prop], (uint32_t)lane);
        bool blocked = !decided && ((prop >= 0 && s_owner[prop] < (uint32_t)lane) || (exhausted && RQ.F.skp != nullptr));
        if constexpr (kLocal) blocked = blocked || (!decided && sec >= 0 && s_owner[sec] < (uint32_t)lane);
        const unsigned long long bm = __ballot(blocked);
        const int first_blocked = bm ? (int)__builtin_ctzll(bm) : 64;
        if (!decided && takes) s_owner[prop] = 0xFFFFFFFFu;
        if (!decided && lane < first_blocked) {
          decided = true;
          if (exhausted) exhausted_any = 1;
          if (matched) {
            atomicMax(&s_assign[prop], q);              // the last writer in query order stays (:1651: CurrentFrame.mvpMapPoints[bestIdx2] = pMP)
            if (takes) s_claimed[prop] = 1;
            if constexpr (kLocal) n_matched++;
            else s_qres[q] = (uint32_t)prop;
          }
        }
      }
    }
    const int any_exhausted = __ballot(exhausted_any != 0) != 0ull;
    const int nrq = wave_sum(n_requeried);
    if constexpr (kLocal) n_matched = wave_sum(n_matched);
    if (lane == 0) { s_cnt[0] = any_exhausted; s_cnt[1] = nrq; s_cnt[2] = n_rounds; s_cnt[3] = n_matched; }
  }
  __syncthreads();
  if constexpr (kLocal) {
    // mvpMapPoints after the search: the last matching query's table entry, else what the frame held (bad points cleared)
    for (int j = tid; j < kp_cap; j += 256) {
      int a = -1;
      if (j < N) { const int qa = s_assign[j]; a = qa >= 0 ? LQ.q_tab[qa] : LQ.frame_mp[j]; }
      assign[j] = a;
      if (j < N) assign_host[j] = a;
    }
    if (tid == 0) {
      res[0] = s_cnt[3]; res[1] = s_cnt[0]; res[2] = s_cnt[3]; res[3] = s_cnt[1];
      res_host[0] = s_cnt[3]; res_host[1] = s_cnt[0]; res_host[2] = s_cnt[3]; res_host[3] = s_cnt[1]; res_host[4] = s_cnt[2];
    }
    return;
  }
  // ---- parallel epilogue.  Rotation histogram of the matches (:1652-1663): counts only, so the order of the additions is free
  if (check_ori) {
    for (int q = tid; q < nq; q += 256) {
      const uint32_t r = s_qres[q];
      if (r == 0xFFFFFFFFu) continue;
      const int bin = rot_bin(q_angle[q], kps[r].angle);
      atomicAdd(&s_rot[bin], 1);
      s_qres[q] = r | ((uint32_t)bin << 16);
    }
  }
  __syncthreads();
  // ComputeThreeMaxima (ORBmatcher.cc:1750-1802) on one lane, then the matches of the other bins are taken back (:1730-1745)
  if (tid == 0) three_maxima(s_rot, s_ind);
  __syncthreads();
  int nmatched = 0, ndropped = 0;
  for (int q = tid; q < nq; q += 256) {
    const uint32_t r = s_qres[q];
    if (r == 0xFFFFFFFFu) continue;
    nmatched++;
    if (check_ori) {
      if (rot_dropped((int)(r >> 16), s_ind)) { ndropped++; s_assign[r & 0xFFFFu] = -1; }
    }
  }
  __shared__ int s_nm[4], s_nd[4];
  block_sum4_put(nmatched, s_nm);
  block_sum4_put(ndropped, s_nd);
  __syncthreads();
  // (both copies: the device one feeds k_track_gather, the mapped one is what the host reads after the chain's one synchronisation)
  for (int j = tid; j < kp_cap; j += 256) {
    const int a = j < N ? s_assign[j] : -1;
    assign[j] = a;
    if (j < N) assign_host[j] = a;
  }
  if (tid == 0) {
    const int nm = block_sum4(s_nm), nd = block_sum4(s_nd);
    res[0] = nm - nd; res[1] = s_cnt[0]; res[2] = nm; res[3] = s_cnt[1];
    res_host[0] = nm - nd; res_host[1] = s_cnt[0]; res_host[2] = nm; res_host[3] = s_cnt[1]; res_host[4] = s_cnt[2];
  }
}

// PoseOptimization's edges (Optimizer.cc:768-838): keypoints with a map point, in keypoint order.  One workgroup, block scan.
//   Xw[e] = (double)pos of the query's map point, obs[e] = (double)mvKeysUn[i].pt, info[e] = (double)mvInvLevelSigma2[octave]
// edge_kp[e] = i.  n_edges[0] = count (0 if the frame has fewer than min_matches matches: the caller's retry / lost path).
__global__ void __launch_bounds__(256) k_track_gather(const int32_t* __restrict__ assign, const dvm_keypoint_pod* __restrict__ kps_un,
                                                      const int32_t* __restrict__ d_n, int kp_cap, const float* __restrict__ q_pos,
                                                      const float* __restrict__ inv_sigma2, int nlevels, double* __restrict__ Xw,
                                                      double* __restrict__ obs, double* __restrict__ info, int32_t* __restrict__ edge_kp,
                                                      int32_t* __restrict__ n_edges, const int32_t* __restrict__ res, int min_matches,
                                                      int32_t* __restrict__ n_edges_host, TrackBatch B) {
  __shared__ int s_wave[4];
  __shared__ int s_base;
  {
    const int b = blockIdx.x;
    assign += (size_t)b * kp_cap; kps_un += (size_t)b * B.kps_stride; d_n += b; q_pos += B.qo(b) * 3;
    Xw += (size_t)b * kp_cap * 3; obs += (size_t)b * kp_cap * 2; info += (size_t)b * kp_cap; edge_kp += (size_t)b * kp_cap;
    n_edges += b; n_edges_host += b; res += 8 * b;
  }
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int N = min(*d_n, kp_cap);
  if (tid == 0) s_base = 0;
  __syncthreads();
  const bool go = res[0] >= min_matches && res[1] == 0;
  for (int i0 = 0; i0 < N && go; i0 += 256) {
    const int i = i0 + tid;
    const int q = i < N ? assign[i] : -1;
    const unsigned long long m = __ballot(q >= 0);
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int pos = s_base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    for (int w = 0; w < wv; w++) pos += s_wave[w];
    if (q >= 0) {
      const dvm_keypoint_pod kp = kps_un[i];
      Xw[3 * pos] = (double)q_pos[3 * q]; Xw[3 * pos + 1] = (double)q_pos[3 * q + 1]; Xw[3 * pos + 2] = (double)q_pos[3 * q + 2];
      obs[2 * pos] = (double)kp.x; obs[2 * pos + 1] = (double)kp.y;
      info[pos] = (double)inv_sigma2[min(max(kp.octave, 0), nlevels - 1)];
      edge_kp[pos] = i;
    }
    __syncthreads();
    if (tid == 0) s_base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
  }
  if (tid == 0) { n_edges[0] = s_base; n_edges_host[0] = s_base; }
}

// mvbOutlier in keypoint order; Tracking.cc:2636-2660: a match PoseOptimization marked an outlier loses its map point, the others
// with Observations() > 0 count into nmatchesMap.  out[0] = nmatchesMap, out[1] = nmatches (res[0]) - outliers.
__global__ void __launch_bounds__(256) k_track_finish(int32_t* __restrict__ assign, const int32_t* __restrict__ d_n, int kp_cap,
                                                      const int32_t* __restrict__ edge_kp, const int32_t* __restrict__ n_edges,
                                                      const uint8_t* __restrict__ edge_outlier, const uint8_t* __restrict__ q_claims,
                                                      uint8_t* __restrict__ outlier, int32_t* __restrict__ out, const int32_t* __restrict__ res, TrackBatch B) {
  __shared__ int s_cnt[2];
  {
    const int b = blockIdx.x;
    assign += (size_t)b * kp_cap; d_n += b; edge_kp += (size_t)b * kp_cap; n_edges += b; edge_outlier += (size_t)b * kp_cap;
    q_claims += B.qo(b); outlier += (size_t)b * kp_cap; out += 4 * b; res += 8 * b;
  }
  const int tid = threadIdx.x;
  const int N = min(*d_n, kp_cap), E = n_edges[0];
  if (tid < 2) s_cnt[tid] = 0;
  for (int j = tid; j < kp_cap; j += 256) outlier[j] = 0;
  __syncthreads();
  int map = 0, left = 0;
  for (int e = tid; e < E; e += 256) {
    const int i = edge_kp[e];
    if (i < 0 || i >= N) continue;
    if (edge_outlier[e]) { outlier[i] = 1; left++; }
    else if (q_claims[assign[i]]) map++;
  }
  atomicAdd(&s_cnt[0], map);
  atomicAdd(&s_cnt[1], left);     // (outlier edges)
  __syncthreads();
  // nmatches is SearchByProjection's count (two queries without observations may have matched the same keypoint: both counted,
  // ORBmatcher.cc:1651-1653) minus one per keypoint whose match PoseOptimization rejected (Tracking.cc:2645-2653)
  if (tid == 0) { out[0] = s_cnt[0]; out[1] = res[0] - s_cnt[1]; }
}

// SearchLocalPoints (Tracking.cc:3041-3106) up to the queries of SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints)
// (ORBmatcher.cc:50-73).  One workgroup per frame, in the reference's order:
//   the frame's points: a bad one is cleared (counted), the others mark their table entry seen (mnLastFrameSeen) -- skipped below and
//     not counted in nToMatch; a keypoint whose point has Observations() > 0 is skipped by the search (LQ.skip)
//   Frame::UpdatePoseMatrices of the first half's float pose (Optimizer.cc:1023-1025: the double pose cast to float), pose_f32.h
//   isInFrustum(pMP, 0.5) of every entry (frustum_point.h); mbTrackInView false for seen and bad entries; nToMatch
//   the far-point filter (:52-53), radius RadiusByViewingCos(viewCos) * (th != 1 ? th : 1) * mvScaleFactors[level], levels
//     [level - 1, level]; the in-view points compacted into the query arrays IN TABLE ORDER (the claim replay's order)
// tables: scale[64] = mvScaleFactors.  res_host[0] = nToMatch, res_host[1] = frame points cleared as bad.  Each frame's table size, th
// and far-point filter from A.per_frame[b]; an empty table with no frame points leaves nothing to search.
// MODEL: the camera behind isInFrustum's mpCamera->project (frustum_point<MODEL>, what dvm_is_in_frustum[_cam] calls); KannalaBrandt8 reads
// A.kb8 (78 VGPRs against the pinhole's 74, no scratch: both keep the 1024-thread workgroup).
template <int MODEL>
__global__ void __launch_bounds__(1024) k_track_local_prologue(const LocalPointPod* __restrict__ pts, const int32_t* __restrict__ frame_mp_in,
                                                               const double* __restrict__ pose_first, const float* __restrict__ scale,
                                                               const int32_t* __restrict__ d_n, int kp_cap, LocalMapArgs A, LocalQueries LQ,
                                                               TrackPoint* __restrict__ tp_host, int32_t* __restrict__ res_host, TrackBatch B) {
  __shared__ int s_wave[16];
  __shared__ int s_cnt[2];
  __shared__ float s_scale[64];
  const LocalFrameArgs fa = A.per_frame[blockIdx.x];
  {
    const int b = blockIdx.x;
    const size_t qo = B.qo(b), ko = (size_t)b * kp_cap;
    pts += qo; frame_mp_in += ko; pose_first += 7 * b; d_n += b; res_host += 8 * b;
    if (tp_host) tp_host += qo;
    LQ.qdesc += qo * 32; LQ.qx += qo; LQ.qy += qo; LQ.qr += qo; LQ.qmin += qo; LQ.qmax += qo; LQ.q_claims += qo; LQ.q_tab += qo; LQ.nq += b;
    LQ.seen += qo; LQ.frame_mp += ko; LQ.skip += ko; LQ.pos += qo * 3; LQ.claims += qo; LQ.pose_in += 7 * b;
  }
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int N = min(*d_n, kp_cap), n = fa.n;
  if (tid < 2) s_cnt[tid] = 0;
  if (tid < 64) s_scale[tid] = tid < A.n_levels ? scale[tid] : 1.0f;
  for (int i = tid; i < n; i += 1024) LQ.seen[i] = 0;
  __syncthreads();
  int cleared = 0;
  for (int j = tid; j < kp_cap; j += 1024) {
    int fm = j < N ? frame_mp_in[j] : -1;      // (the host checked fm < n)
    uint8_t sk = 0;
    if (fm >= 0) {
      if (pts[fm].bad) { fm = -1; cleared++; }
      else { LQ.seen[fm] = 1; sk = pts[fm].n_obs > 0 ? 1 : 0; }
    }
    LQ.frame_mp[j] = fm;
    LQ.skip[j] = sk;
  }
  if (cleared) atomicAdd(&s_cnt[0], cleared);
  // Frame::UpdatePoseMatrices: mRcw = R(q), mtcw = t, mOw = Tcw.inverse().translation() (each thread the same float operations)
  float q[4], t[3];
#pragma unroll
  for (int k = 0; k < 3; k++) t[k] = (float)pose_first[k];
#pragma unroll
  for (int k = 0; k < 4; k++) q[k] = (float)pose_first[3 + k];
  FrustumFrame F;
  dvm_pose::quat_matrix(q, F.Rcw);
  F.tcw[0] = t[0]; F.tcw[1] = t[1]; F.tcw[2] = t[2];
  {
    float qi[4];
    dvm_pose::se3_inverse(q, t, qi, F.Ow);
  }
  F.fx = A.fx; F.fy = A.fy; F.cx = A.cx; F.cy = A.cy; F.min_x = A.min_x; F.max_x = A.max_x; F.min_y = A.min_y; F.max_y = A.max_y;
  F.bf = 0.0f; F.log_scale_factor = A.log_scale_factor; F.n_levels = A.n_levels;
  if (tid < 7) LQ.pose_in[tid] = (double)(float)pose_first[tid];   // g2o::SE3Quat of the SE3f (Optimizer.cc:759-760)
  __syncthreads();
  int base = 0, n_view = 0;
  for (int c = 0; c < n; c += 1024) {
    const int i = c + tid;
    bool query = false;
    TrackPoint o{};
    if (i < n) {
      const LocalPointPod& P = pts[i];
      o = frustum_point<MODEL>(F, P.pos[0], P.pos[1], P.pos[2], P.normal[0], P.normal[1], P.normal[2], P.min_dist, P.max_dist, 0.5f, A.kb8);
      if (LQ.seen[i] || P.bad) o.in_view = 0;
      n_view += o.in_view;
      if (tp_host) tp_host[i] = o;
      LQ.pos[3 * (size_t)i] = P.pos[0]; LQ.pos[3 * (size_t)i + 1] = P.pos[1]; LQ.pos[3 * (size_t)i + 2] = P.pos[2];
      LQ.claims[i] = P.n_obs > 0 ? 1 : 0;
      query = o.in_view && !(fa.far_points && o.depth > fa.th_far);
    }
    const unsigned long long m = __ballot(query);
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int pos = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    int total = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) {
      const int cw = s_wave[w];
      if (w < wv) pos += cw;
      total += cw;
    }
    if (query) {
      const LocalPointPod& P = pts[i];
      float r = o.view_cos > 0.998 ? 2.5f : 4.0f;            // RadiusByViewingCos (ORBmatcher.cc:207-212)
      if (fa.th != 1.0f) r *= fa.th;
      LQ.qx[pos] = o.proj_x; LQ.qy[pos] = o.proj_y; LQ.qr[pos] = r * s_scale[min(max(o.level, 0), 63)];
      LQ.qmin[pos] = o.level - 1; LQ.qmax[pos] = o.level;
      LQ.q_claims[pos] = P.n_obs > 0 ? 1 : 0; LQ.q_tab[pos] = i;
      const uint2* sd = reinterpret_cast<const uint2*>(P.desc);
      uint2* dd = reinterpret_cast<uint2*>(LQ.qdesc + (size_t)pos * 32);
#pragma unroll
      for (int k = 0; k < 4; k++) dd[k] = sd[k];
    }
    base += total;
    __syncthreads();
  }
  for (int off = 32; off >= 1; off >>= 1) n_view += __shfl_xor(n_view, off);
  if (lane == 0 && n_view) atomicAdd(&s_cnt[1], n_view);
  __syncthreads();
  if (tid == 0) { LQ.nq[0] = base; res_host[0] = s_cnt[1]; res_host[1] = s_cnt[0]; }
}

// The loop header of SearchByProjection(CurrentFrame, LastFrame) (ORBmatcher.cc:1573-1611) on the device, from LastFrame's entry list and
// the agent's map-point store (dvm_track_finish_batch_resident) -- what dvm_host::BuildFrameQueries and the three per-query arrays of
// host/tracking.cpp produce on the host, operation for operation:
//   x3Dc = Tcw * pos (dvm_pose::se3_apply: Sophus' quaternion form), invzc = (float)(1.0 / zc), the entry skipped if invzc < 0;
//   (u, v) = mpCamera->project(x3Dc): pinhole fx * xc / zc + cx in float, KannalaBrandt8 dvm_cam::kb8_project on A.kb8;
//   skipped if u < mnMinX || u > mnMaxX, or v < mnMinY || v > mnMaxY (written as the reference writes them: a NaN passes);
//   radius = th * mvScaleFactors[octave], levels octave - 1 .. octave + 1.
// One workgroup of four waves per frame, entries in rounds of 256.  The kept entries are compacted IN ENTRY ORDER (the claim replay is
// sequential in query order): inside a wave a ballot and mbcnt give the lane's offset, the four waves' counts go through LDS, and a
// running base carries over the rounds.  Per kept entry: qx qy qr qmin qmax, q_claims (n_obs > 0), q_angle, q_pos, the 32 descriptor
// bytes of the store's record, and the entry number (mapped: the host turns the chain's query numbers into entry numbers with it).
// nq goes to the device nq_arr and to mapped memory; pose_in is the predicted pose widened to double (Optimizer.cc:760).
template <int MODEL>
__global__ void __launch_bounds__(256) k_track_queries(const ResidentFrame* __restrict__ frames, const int32_t* __restrict__ slot,
                                                       const uint8_t* __restrict__ octave, const float* __restrict__ angle,
                                                       const float* __restrict__ scale, TrackQueryArgs A, int stride, TrackQueryOut O) {
  __shared__ int s_wave[4];
  __shared__ float s_scale[64];
  const int b = blockIdx.x;
  const ResidentFrame fr = frames[b];
  {
    const size_t o = (size_t)b * stride;
    slot += fr.off; octave += fr.off; angle += fr.off;
    O.qdesc += o * 32; O.qx += o; O.qy += o; O.qr += o; O.qmin += o; O.qmax += o; O.q_claims += o; O.q_angle += o; O.q_pos += o * 3;
    O.pose_in += 7 * b; O.nq_arr += b; O.q_entry_host += o; O.nq_host += b;
  }
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = fr.n;
  if (tid < 64) s_scale[tid] = scale[tid];
  if (tid == 0) {      // (constant indices: fr stays in registers)
#pragma unroll
    for (int k = 0; k < 3; k++) O.pose_in[k] = (double)fr.t[k];
#pragma unroll
    for (int k = 0; k < 4; k++) O.pose_in[3 + k] = (double)fr.q[k];
  }
  __syncthreads();
  int base = 0;
  for (int c = 0; c < n; c += 256) {
    const int i = c + tid;
    bool keep = false;
    float u = 0.0f, v = 0.0f;
    const LocalPointPod* P = nullptr;
    int oct = 0;
    if (i < n) {
      P = fr.store + slot[i];
      oct = octave[i];
      const float X[3] = {P->pos[0], P->pos[1], P->pos[2]};
      float x3Dc[3];
      dvm_pose::se3_apply(fr.q, fr.t, X, x3Dc);
      const float xc = x3Dc[0], yc = x3Dc[1], zc = x3Dc[2];
      const float invzc = (float)(1.0 / zc);
      if (MODEL == dvm_cam::kKannalaBrandt8) dvm_cam::kb8_project(A.kb8, xc, yc, zc, u, v);
      else { u = A.fx * xc / zc + A.cx; v = A.fy * yc / zc + A.cy; }
      keep = !(invzc < 0) && !(u < A.min_x || u > A.max_x) && !(v < A.min_y || v > A.max_y);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int pos = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    int total = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const int cw = s_wave[w];
      if (w < wv) pos += cw;
      total += cw;
    }
    if (keep) {
      O.qx[pos] = u; O.qy[pos] = v; O.qr[pos] = fr.th * s_scale[oct];
      O.qmin[pos] = oct - 1; O.qmax[pos] = oct + 1;
      O.q_claims[pos] = P->n_obs > 0 ? 1 : 0;
      O.q_angle[pos] = angle[i];
      O.q_pos[3 * (size_t)pos] = P->pos[0]; O.q_pos[3 * (size_t)pos + 1] = P->pos[1]; O.q_pos[3 * (size_t)pos + 2] = P->pos[2];
      const uint2* sd = reinterpret_cast<const uint2*>(P->desc);
      uint2* dd = reinterpret_cast<uint2*>(O.qdesc + (size_t)pos * 32);
#pragma unroll
      for (int k = 0; k < 4; k++) dd[k] = sd[k];
      O.q_entry_host[pos] = i;
    }
    base += total;
    __syncthreads();
  }
  if (tid == 0) { O.nq_arr[0] = base; O.nq_host[0] = base; }
}

// ---- the reference-keyframe chain: Tracking::TrackReferenceKeyFrame (Tracking.cc:2461-2520) behind the extraction of the frame

// (block_scan_1024, bitonic_sort and for_each_run: block_sort.h, shared with keyframe_put_kernels.hip)

// frame b: every per-frame pointer of A moved to that frame's slice (RefKfArgs)
__device__ __forceinline__ void refkf_at(RefKfArgs& A, int b, int cap) {
  const size_t o = (size_t)b * cap;
  A.word += o; A.node += o; A.w += o; A.fv_node += o; A.fv_feat += o; A.fv_off += o + b; A.cnt += (size_t)b * kRefKfCnt; A.match += o; A.bin += o;
  A.res += 8 * b;
  A.h_bow_ids += o; A.h_bow_vals += o; A.h_fv_node += o; A.h_fv_off += o + b; A.h_fv_feat += o; A.h_match += o; A.h_cnt += 8 * b;
  const size_t k = (size_t)A.kqoff[b];
  A.kdesc += k * 32; A.kangle += k; A.kuse += k; A.kfv_node += k; A.kfv_off += k + b; A.kfv_feat += k;
}

// Frame::ComputeBoW's bookkeeping (TemplatedVocabulary::transform's TF_IDF branch, DBoW2 TemplatedVocabulary.h:1098-1138, as the host
// mirror dvm_slam_amd/host/orb_vocabulary.cpp keeps it) on k_vocab_transform's per-feature results, in LDS by one workgroup:
//   the features with weight > 0 only (a stopped word adds nothing, not even its node entry);
//   BowVector: sort (word << 32 | feature); each word's weight is the sum of its features' weights added in feature order, the L1 norm
//     the sum of |value| in ascending word order -- both sequential double additions, the order std::map gives the host -- then each
//     value divided by the norm (correctly rounded double division);
//   FeatureVector: sort ((unsigned)node << 32 | feature): nodes ascending as unsigned (node -1 last), features ascending inside a node.
// It also resets the match state of the search behind it.  LDS: 16 B per entry of the sort (the capacity rounded up to a power of two).
// One workgroup per frame that runs (A.run).
__global__ void __launch_bounds__(1024) k_refkf_bow(RefKfArgs A, const int32_t* __restrict__ d_n, int cap, int P) {
  { const int b = A.run[blockIdx.x]; refkf_at(A, b, cap); d_n += b; }
  extern __shared__ __attribute__((aligned(16))) uint8_t refkf_smem[];
  uint64_t* keys = reinterpret_cast<uint64_t*>(refkf_smem);    // [P]
  double* vals = reinterpret_cast<double*>(keys + P);          // [P]
  __shared__ int s_wave[16];
  __shared__ int s_m;
  __shared__ double s_norm;
  const int tid = threadIdx.x;
  const int N = min(*d_n, cap);
  for (int j = tid; j < cap; j += 1024) { A.match[j] = -1; A.bin[j] = -1; }
  if (tid < kRefKfCnt) A.cnt[tid] = 0;
  if (tid == 0) s_m = 0;
  __syncthreads();
  int m = 0;
  for (int i = tid; i < P; i += 1024) {
    const bool keep = i < N && A.w[i] > 0.0;
    keys[i] = keep ? ((uint64_t)(uint32_t)A.word[i] << 32) | (uint32_t)i : ~0ull;
    m += keep ? 1 : 0;
  }
  if (m) atomicAdd(&s_m, m);
  __syncthreads();
  const int M = s_m;
  bitonic_sort(keys, P);
  // BowVector: one thread per word adds its features' weights in feature order
  const int n_bow = for_each_run(keys, M, s_wave, [&](int r, int start) {
    const uint32_t word = (uint32_t)(keys[start] >> 32);
    double v = A.w[(uint32_t)keys[start]];
    for (int i = start + 1; i < M && (uint32_t)(keys[i] >> 32) == word; i++) v += A.w[(uint32_t)keys[i]];
    vals[r] = v;
    A.h_bow_ids[r] = (int32_t)word;
  });
  __syncthreads();
  if (tid == 0) {
    double norm = 0.0;
    for (int r = 0; r < n_bow; r++) norm += fabs(vals[r]);
    s_norm = norm;
  }
  __syncthreads();
  const double norm = s_norm;
  for (int r = tid; r < n_bow; r += 1024) A.h_bow_vals[r] = norm > 0.0 ? vals[r] / norm : vals[r];
  __syncthreads();
  // FeatureVector
  for (int i = tid; i < P; i += 1024) {
    const bool keep = i < N && A.w[i] > 0.0;
    keys[i] = keep ? ((uint64_t)(uint32_t)A.node[i] << 32) | (uint32_t)i : ~0ull;
  }
  __syncthreads();
  bitonic_sort(keys, P);
  const int n_fv = for_each_run(keys, M, s_wave, [&](int r, int start) {
    const int32_t nd = (int32_t)(uint32_t)(keys[start] >> 32);
    A.fv_node[r] = nd; A.fv_off[r] = start;
    A.h_fv_node[r] = nd; A.h_fv_off[r] = start;
  });
  for (int i = tid; i < M; i += 1024) {
    const int32_t f = (int32_t)(uint32_t)keys[i];
    A.fv_feat[i] = f; A.h_fv_feat[i] = f;
  }
  if (tid == 0) {
    A.fv_off[n_fv] = M; A.h_fv_off[n_fv] = M;
    A.cnt[0] = n_bow; A.cnt[1] = n_fv;
  }
}

// ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:214-393, monocular) without a serial replay.  The reference walks the
// nodes both FeatureVectors share in ascending order; inside a node it takes the keyframe's features in order (those without a map point
// or with a bad one skipped), scans the node's frame features that no earlier match has taken (:265-266), keeps the smallest distance
// (first in scan order wins) and the second smallest (duplicates counted), and takes the best when best <= TH_LOW and best < nnratio *
// second.  A frame feature lies in exactly ONE node of the frame's FeatureVector, so what one node's matches take is never a candidate
// of another node: the nodes are independent, and the reference's sequential walk is one sequential walk per node in any node order.
// One wave per keyframe node: the node is found in the frame's list by binary search, the wave walks the node's keyframe features in
// order and scans the frame features across its lanes (bow_node_scan, match_device.h: min of (distance << 20 | scan position) and the
// two smallest distances), so every decision sees exactly the claims the reference's walk has made by then.  The rotation histogram only counts, so its
// global atomics may come in any order.  LDS: the claim flag of every frame keypoint (1 B each).
// Known limit: a vocabulary with L - levelsup <= 0 puts every feature into node 0: one wave then walks the whole frame.
// Each frame that runs has its own range of workgroups (A.wg_base), so a workgroup's claim flags -- indexed by the frame's keypoint --
// never mix two frames.
__global__ void __launch_bounds__(256) k_refkf_search(RefKfArgs A, const dvm_keypoint_pod* __restrict__ kps_un, const uint8_t* __restrict__ desc,
                                                      const int32_t* __restrict__ d_n, int cap, int th_low, float nnratio) {
  extern __shared__ __attribute__((aligned(16))) uint8_t refkf_smem[];
  uint8_t* s_claim = refkf_smem;   // [cap]
  int wg = blockIdx.x, kfv_n;
  {
    int lo = 0, hi = A.nrun - 1;            // the run r with wg_base[r] <= blockIdx.x < wg_base[r + 1]
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (A.wg_base[mid] <= wg) lo = mid; else hi = mid - 1;
    }
    const int b = A.run[lo];
    wg -= A.wg_base[lo];
    kfv_n = A.kfv_nb[b];
    refkf_at(A, b, cap);
    kps_un += (size_t)b * A.kps_stride; desc += (size_t)b * A.desc_stride; d_n += b;
  }
  for (int j = threadIdx.x; j < cap; j += 256) s_claim[j] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int a = wg * 4 + (threadIdx.x >> 6);
  if (a >= kfv_n) return;
  const int N = min(*d_n, cap), n_fv = A.cnt[1];
  const int at = fv_find(A.fv_node, n_fv, A.kfv_node[a]);     // the frame's nodes ascend as unsigned
  if (at < 0) return;                     // the frame does not have the node
  const int fb = A.fv_off[at], fe = A.fv_off[at + 1];
  for (int k = A.kfv_off[a]; k < A.kfv_off[a + 1]; k++) {
    const int r = A.kfv_feat[k];          // (the host checked 0 <= r < n)
    if (!A.kuse[r]) continue;
    int d2;
    const uint32_t best = bow_node_scan(A.kdesc, r, A.fv_feat, fb, fe, desc, lane, [&](int, int j) { return j >= N || s_claim[j]; }, d2);
    const int bd = (int)(best >> 20);
    if (bd <= th_low && (float)bd < nnratio * (float)d2) {
      const int j = A.fv_feat[fb + (int)(best & 0xFFFFFu)];
      if (lane == 0) {
        s_claim[j] = 1;
        const int bin = rot_bin(A.kangle[r], kps_un[j].angle);
        A.match[j] = r; A.bin[j] = bin;
        if (bin >= 0 && bin < kHisto) atomicAdd(&A.cnt[8 + bin], 1);     // (angles outside [0, 360) fall outside the histogram)
        atomicAdd(&A.cnt[2], 1);
      }
    }
  }
}

// the rotation check of SearchByBoW (:372-387): ComputeThreeMaxima, the matches of the other bins taken back; res[0] = nmatches for the
// edge gather, the final matches to mapped memory.  One workgroup per frame that runs.
__global__ void __launch_bounds__(256) k_refkf_settle(RefKfArgs A, const int32_t* __restrict__ d_n, int cap, int check_ori) {
  { const int b = A.run[blockIdx.x]; refkf_at(A, b, cap); d_n += b; }
  __shared__ int s_rot[kHisto];
  __shared__ int s_ind[3];
  __shared__ int s_nd[4];
  const int tid = threadIdx.x;
  const int N = min(*d_n, cap);
  if (tid < kHisto) s_rot[tid] = A.cnt[8 + tid];
  __syncthreads();
  if (tid == 0) three_maxima(s_rot, s_ind);
  __syncthreads();
  int nd = 0;
  for (int j = tid; j < cap; j += 256) {
    int m = j < N ? A.match[j] : -1;
    if (m >= 0 && check_ori) {
      if (rot_dropped(A.bin[j], s_ind)) { m = -1; nd++; A.match[j] = -1; }
    }
    if (j < N) A.h_match[j] = m;
  }
  block_sum4_put(nd, s_nd);
  __syncthreads();
  if (tid == 0) {
    const int nm = A.cnt[2], nmatches = nm - block_sum4(s_nd);
    A.res[0] = nmatches; A.res[1] = 0;
    A.h_cnt[0] = A.cnt[0]; A.h_cnt[1] = A.cnt[1]; A.h_cnt[2] = nm; A.h_cnt[3] = nmatches;
  }
}

size_t track_claims_lds(int kp_cap, int nq) { const size_t qp = ((size_t)nq + 63) & ~(size_t)63; return qp * 16 + (size_t)kp_cap * 9 + qp * 5 + 16; }

void launch_track_claims(hipStream_t s, const uint32_t* ranked, const uint8_t* q_claims, const float* q_angle, int nq, const TrackRequery& rq,
                         const dvm_keypoint_pod* kps, const int32_t* d_n, int kp_cap, int th_high, int check_ori, int32_t* assign, int32_t* res,
                         int32_t* assign_host, int32_t* res_host, const TrackBatch& B) {
  const size_t lds = track_claims_lds(kp_cap, B.count > 1 || B.nq_arr ? B.qstride : nq);
  if (lds > 48 * 1024) raise_dynamic_lds(reinterpret_cast<const void*>(k_track_claims<false>), (int)lds);
  hipLaunchKernelGGL(k_track_claims<false>, dim3(B.count), dim3(256), lds, s, ranked, q_claims, q_angle, nq, rq, kps, d_n, kp_cap, th_high,
                     check_ori, 0.0f, LocalQueries{}, assign, res, assign_host, res_host, B);
}
void launch_track_claims_local(hipStream_t s, const uint32_t* ranked, const LocalQueries& LQ, const TrackRequery& rq, const dvm_keypoint_pod* kps,
                               const int32_t* d_n, int kp_cap, int th_high, float nnratio, int32_t* assign, int32_t* res, int32_t* assign_host,
                               int32_t* res_host, const TrackBatch& B) {
  const size_t lds = (size_t)kp_cap * 10 + 16;
  if (lds > 48 * 1024) raise_dynamic_lds(reinterpret_cast<const void*>(k_track_claims<true>), (int)lds);
  hipLaunchKernelGGL(k_track_claims<true>, dim3(B.count), dim3(256), lds, s, ranked, LQ.q_claims, nullptr, 0, rq, kps, d_n, kp_cap, th_high, 0,
                     nnratio, LQ, assign, res, assign_host, res_host, B);
}
void launch_track_local_prologue(hipStream_t s, int model, const LocalPointPod* pts, const int32_t* frame_mp_in, const double* pose_first,
                                 const float* scale, const int32_t* d_n, int kp_cap, const LocalMapArgs& A, const LocalQueries& LQ,
                                 TrackPoint* track_pts_host, int32_t* res_host, const TrackBatch& B) {
  if (model == dvm_cam::kKannalaBrandt8)
    hipLaunchKernelGGL((k_track_local_prologue<dvm_cam::kKannalaBrandt8>), dim3(B.count), dim3(1024), 0, s, pts, frame_mp_in, pose_first, scale, d_n,
                       kp_cap, A, LQ, track_pts_host, res_host, B);
  else
    hipLaunchKernelGGL((k_track_local_prologue<dvm_cam::kPinhole>), dim3(B.count), dim3(1024), 0, s, pts, frame_mp_in, pose_first, scale, d_n, kp_cap,
                       A, LQ, track_pts_host, res_host, B);
}
void launch_track_queries(hipStream_t s, int model, const ResidentFrame* frames, const int32_t* slot, const uint8_t* octave, const float* angle,
                          const float* scale, const TrackQueryArgs& A, int count, int stride, const TrackQueryOut& O) {
  if (model == dvm_cam::kKannalaBrandt8)
    hipLaunchKernelGGL((k_track_queries<dvm_cam::kKannalaBrandt8>), dim3(count), dim3(256), 0, s, frames, slot, octave, angle, scale, A, stride, O);
  else
    hipLaunchKernelGGL((k_track_queries<dvm_cam::kPinhole>), dim3(count), dim3(256), 0, s, frames, slot, octave, angle, scale, A, stride, O);
}
void launch_track_gather(hipStream_t s, const int32_t* assign, const dvm_keypoint_pod* kps_un, const int32_t* d_n, int kp_cap, const float* q_pos,
                         const float* inv_sigma2, int nlevels, double* Xw, double* obs, double* info, int32_t* edge_kp, int32_t* n_edges,
                         const int32_t* res, int min_matches, int32_t* n_edges_host, const TrackBatch& B) {
  hipLaunchKernelGGL(k_track_gather, dim3(B.count), dim3(256), 0, s, assign, kps_un, d_n, kp_cap, q_pos, inv_sigma2, nlevels, Xw, obs, info, edge_kp, n_edges,
                     res, min_matches, n_edges_host, B);
}
void launch_track_finish(hipStream_t s, int32_t* assign, const int32_t* d_n, int kp_cap, const int32_t* edge_kp, const int32_t* n_edges,
                         const uint8_t* edge_outlier, const uint8_t* q_claims, uint8_t* outlier, int32_t* out, const int32_t* res, const TrackBatch& B) {
  hipLaunchKernelGGL(k_track_finish, dim3(B.count), dim3(256), 0, s, assign, d_n, kp_cap, edge_kp, n_edges, edge_outlier, q_claims, outlier, out, res, B);
}

void launch_refkf_bow(hipStream_t s, const RefKfArgs& A, const int32_t* d_n, int cap) {
  int P = 1;
  while (P < cap) P <<= 1;
  const size_t lds = (size_t)P * 16;
  if (lds > 48 * 1024) raise_dynamic_lds(reinterpret_cast<const void*>(k_refkf_bow), (int)lds);
  if (A.nrun < 1) return;
  hipLaunchKernelGGL(k_refkf_bow, dim3(A.nrun), dim3(1024), lds, s, A, d_n, cap, P);
}
void launch_refkf_search(hipStream_t s, const RefKfArgs& A, const dvm_keypoint_pod* kps_un, const uint8_t* desc, const int32_t* d_n, int cap, int th_low,
                         float nnratio) {
  if (A.nwg < 1) return;
  hipLaunchKernelGGL(k_refkf_search, dim3(A.nwg), dim3(256), (size_t)cap, s, A, kps_un, desc, d_n, cap, th_low, nnratio);
}
void launch_refkf_settle(hipStream_t s, const RefKfArgs& A, const int32_t* d_n, int cap, int check_ori) {
  if (A.nrun < 1) return;
  hipLaunchKernelGGL(k_refkf_settle, dim3(A.nrun), dim3(256), 0, s, A, d_n, cap, check_ori);
}

// ---- dvm_track_reference_keyframe_batch_resident: the packed keyframe block filled from the stores, as refkf_enqueue (track.cpp) packs
// it on the host for the uploaded call.  One 1 024-thread workgroup per frame that runs.  Descriptors, nodes and features move 16 bytes
// per thread and step: the slot's arrays begin at multiples of 64 bytes and kqoff[b] is a multiple of 64 entries, so both sides are
// aligned; the offsets land at kqoff[b] + b entries, 4-byte aligned only, and move a dword at a time.  Per keypoint: the angle out of
// the slot's 28-byte records, and out of the map point's 72-byte record the host loop's three rules.  No LDS, no barrier.
namespace {
// n4 dwords from src to dst, both at multiples of 16 bytes
__device__ __forceinline__ void refkf_move(int32_t* __restrict__ dst, const int32_t* __restrict__ src, int n4) {
  const int n16 = n4 >> 2;
  for (int i = threadIdx.x; i < n16; i += 1024) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
  for (int i = n16 * 4 + threadIdx.x; i < n4; i += 1024) dst[i] = src[i];
}
}  // namespace
__global__ void __launch_bounds__(1024) k_refkf_gather(const RefKfGatherItem* __restrict__ items, const int32_t* __restrict__ mp_slot,
                                                       const int32_t* __restrict__ run, const int32_t* __restrict__ kqoff,
                                                       const int32_t* __restrict__ kfv_nb, RefKfGatherOut O) {
  const int b = run[blockIdx.x];
  const RefKfGatherItem K = items[b];
  const size_t o = (size_t)kqoff[b];
  const int nf = kfv_nb[b];
  refkf_move(reinterpret_cast<int32_t*>(O.desc + o * 32), reinterpret_cast<const int32_t*>(K.desc), K.n * 8);
  refkf_move(O.fv_node + o, K.fv_node, nf);
  refkf_move(O.fv_feat + o, K.fv_feat, K.n_feat);
  int32_t* fo = O.fv_off + o + b;
  if (nf > 0) {
    for (int a = threadIdx.x; a <= nf; a += 1024) fo[a] = K.fv_off[a];
  } else if (threadIdx.x == 0) {
    fo[0] = 0;
  }
  const int32_t* slots = mp_slot + o;
  for (int i = threadIdx.x; i < K.n; i += 1024) {
    const int id = slots[i];
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    bool use = false, claims = false;
    if (id >= 0) {
      const LocalPointPod& R = K.recs[id];
      px = R.pos[0]; py = R.pos[1]; pz = R.pos[2];
      use = R.bad == 0;                     // SearchByBoW: no map point or a bad one -> skipped (:247-252)
      claims = R.n_obs > 0;
    }
    O.angle[o + i] = K.kps[i].angle;
    O.use[o + i] = use ? 1 : 0;
    O.claims[o + i] = claims ? 1 : 0;
    float* p = O.pos + 3 * (o + i);
    p[0] = px; p[1] = py; p[2] = pz;
  }
}
void launch_refkf_gather(hipStream_t s, const RefKfGatherItem* items, const int32_t* mp_slot, const int32_t* run, int nrun, const int32_t* kqoff,
                         const int32_t* kfv_nb, const RefKfGatherOut& O) {
  static_assert(sizeof(RefKfGatherItem) == 56, "track_kernels.h states it");
  if (nrun < 1) return;
  hipLaunchKernelGGL(k_refkf_gather, dim3(nrun), dim3(1024), 0, s, items, mp_slot, run, kqoff, kfv_nb, O);
}

}  // namespace dvm
