// dvm_slam_amd/csrc/bow_targets_kernels.hip -- ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (ORBmatcher.cc:709-834) of one current
// keyframe against many target keyframes: the searches LoopClosing::DetectCommonRegionsFromBoW runs per candidate and covisible
// (LoopClosing.cc:722-731), all in one launch plus one launch for the rotation checks.
#include <algorithm>

#include "bow_targets_kernels.h"
#include "match_device.h"
#include "rot_bin.h"
#include "track_kernels.h"   // LocalPointPod, dvm_keypoint_pod

namespace dvm {

// The reference walks the nodes both FeatureVectors share in ascending order; inside a node it takes KF1's features in list order (those
// without a map point or with a bad one skipped, :742-748), scans the node's KF2 features that have a good map point and that no earlier
// match has taken (vbMatched2, :759-767), keeps the smallest distance (first in scan order wins) and the second smallest (duplicates
// counted), and takes the best when best < TH_LOW -- STRICT, :785; the KeyFrame -> Frame form (k_refkf_search) has <= -- and
// best < nnratio * second.  A keypoint of KF2 lies in exactly ONE node of KF2's FeatureVector (the host checks it while packing), so
// vbMatched2 never couples two nodes, and targets never share anything: every (target, node of KF1) pair is one independent sequential
// walk.  One wave per pair: the node is found in the target's list by binary search, the wave walks the node's KF1 features in order and
// scans the target's features across its lanes (bow_node_scan, match_device.h, which k_refkf_search calls too), so every decision sees
// exactly the claims the reference's walk has made by then.
// Claims: lane l scans the positions l, l + 64, l + 128, ... of the node and no other lane ever reads them, so the claim flag of position
// p is bit p / 64 of a 128-bit mask in lane p % 64's registers (a node holds at most 8192 features).  Nothing is shared between pairs,
// whichever target the four waves of a workgroup belong to.
// The wave writes match (-1 included) for every KF1 feature of its node, so the rows need no initialisation; KF1 features that no node
// lists are the host's.  The histogram only counts, so its global atomics may come in any order.
__global__ void __launch_bounds__(256) k_bt_search(const BtKfDev* __restrict__ tab, int n_targets, int n1, int fv_n1, float nnratio,
                                                  int32_t* __restrict__ match, int8_t* __restrict__ bin, int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= (int64_t)n_targets * fv_n1) return;
  const int t = (int)(pair / fv_n1), a = (int)(pair - (int64_t)t * fv_n1);
  const BtKfDev C = tab[0], K = tab[1 + t];
  int32_t* row = match + (size_t)t * n1;
  int8_t* brow = bin + (size_t)t * n1;
  const int kb = C.fv_off[a], ke = C.fv_off[a + 1];
  int fb = 0, fe = 0;
  {
    const int at = fv_find(K.fv_node, K.fv_n, C.fv_node[a]);   // the target's nodes ascend as unsigned
    if (at >= 0) { fb = K.fv_off[at]; fe = K.fv_off[at + 1]; }
  }
  if (fe <= fb) {                           // the target does not have the node: nothing of it matches
    for (int k = kb + lane; k < ke; k += 64) row[C.fv_feat[k]] = -1;
    return;
  }
  uint64_t claim0 = 0, claim1 = 0;          // bit s: this lane's position lane + 64 * s (claim1: s - 64) is taken
  for (int k = kb; k < ke; k++) {
    const int r = C.fv_feat[k];             // (the host checked 0 <= r < n1)
    if (!C.use[r]) {
      if (lane == 0) row[r] = -1;
      continue;
    }
    int d2;
    const uint32_t best = bow_node_scan(C.desc, r, K.fv_feat, fb, fe, K.desc, lane, [&](int p, int j) {   // (the host checked 0 <= j < n)
      const int s = (p - fb) >> 6;
      return ((s < 64 ? claim0 >> s : claim1 >> (s - 64)) & 1) != 0 || !K.use[j];
    }, d2);
    const int bd = (int)(best >> 20);
    const bool take = bd < 50 && (float)bd < nnratio * (float)d2;     // TH_LOW, strict (:785-786)
    if (take) {
      const int pos = (int)(best & 0xFFFFFu);
      if (lane == (pos & 63)) {
        const int sb = pos >> 6;
        if (sb < 64) claim0 |= 1ull << sb; else claim1 |= 1ull << (sb - 64);
      }
      if (lane == 0) {
        const int j = K.fv_feat[fb + pos];
        const int b = rot_bin(C.angle[r], K.angle[j]);
        const bool in = b >= 0 && b < kRotHisto;                      // (angles outside [0, 360) fall outside the histogram)
        row[r] = j; brow[r] = (int8_t)(in ? b : -2);
        if (in) atomicAdd(&cnt[t * kBtCnt + b], 1);
        atomicAdd(&cnt[t * kBtCnt + 30], 1);
      }
    } else if (lane == 0) {
      row[r] = -1;
    }
  }
}

// the rotation check (:813-831): ComputeThreeMaxima on the target's histogram, the matches of the other bins taken back, nmatches.  It
// walks the features KF1's FeatureVector lists: the others hold no match.  One workgroup per target.
__global__ void __launch_bounds__(256) k_bt_settle(const BtKfDev* __restrict__ tab, int n1, int check_ori, int32_t* __restrict__ match,
                                                  const int8_t* __restrict__ bin, const int32_t* __restrict__ cnt, int32_t* __restrict__ nmatches) {
  __shared__ int s_rot[kRotHisto];
  __shared__ int s_ind[3];
  __shared__ int s_nd[4];
  const int t = blockIdx.x, tid = threadIdx.x;
  const BtKfDev C = tab[0];
  if (tid < kRotHisto) s_rot[tid] = cnt[t * kBtCnt + tid];
  __syncthreads();
  if (tid == 0) three_maxima(s_rot, s_ind);
  __syncthreads();
  int nd = 0;
  if (check_ori) {
    int32_t* row = match + (size_t)t * n1;
    const int8_t* brow = bin + (size_t)t * n1;
    const int m1 = C.fv_off[C.fv_n];
    for (int p = tid; p < m1; p += 256) {
      const int i = C.fv_feat[p];
      if (row[i] < 0) continue;
      if (rot_dropped(brow[i], s_ind)) { row[i] = -1; nd++; }
    }
  }
  block_sum4_put(nd, s_nd);
  __syncthreads();
  if (tid == 0) nmatches[t] = cnt[t * kBtCnt + 30] - block_sum4(s_nd);
}

// the resident call's prologue: what the uploaded call packs on the host, derived on the device from the keyframe-store slots and the
// map stores.  blockIdx.x = table entry (the current keyframe, the targets), blockIdx.y walks its keypoints, kBtProSpan to a workgroup:
// a thread takes four consecutive keypoints -- ONE 16-byte load of their map-point slots, four gathers of record.bad (72-byte records) and
// of the keypoint's angle (28-byte records), ONE 16-byte store of the angles and ONE 4-byte store of the flags.  The slot list, the angle
// and the flag array each begin at a multiple of 64 bytes and are rounded up to one, so the last thread's vector stays inside its item;
// what it writes past n is zero and nothing reads it.  Then all workgroups together fill the match rows with -1 (a feature of the
// current keyframe that no node lists keeps it: k_bt_search writes the listed ones only) and zero the counters, 16 bytes a thread.  No
// LDS, no barrier; four waves of 64.
__global__ void __launch_bounds__(kBtProThreads) k_bt_prologue(const BtKfDev* __restrict__ tab, const BtProKf* __restrict__ pro,
                                                               int32_t* __restrict__ match, int64_t n_match, int32_t* __restrict__ cnt, int n_cnt) {
  const BtKfDev K = tab[blockIdx.x];
  const BtProKf P = pro[blockIdx.x];
  const int i0 = ((int)blockIdx.y * kBtProThreads + (int)threadIdx.x) * 4;
  if (i0 < K.n) {
    const int4 sl = *reinterpret_cast<const int4*>(P.mp_slot + i0);
    const int slot[4] = {sl.x, sl.y, sl.z, sl.w};
    float a[4];
    uint32_t use = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bool in = i0 + j < K.n;
      a[j] = in ? reinterpret_cast<const dvm_keypoint_pod*>(P.kps)[i0 + j].angle : 0.0f;
      if (in && slot[j] >= 0 && reinterpret_cast<const LocalPointPod*>(P.recs)[slot[j]].bad == 0) use |= 1u << (8 * j);   // pMP && !pMP->isBad()
    }
    *reinterpret_cast<float4*>(const_cast<float*>(K.angle) + i0) = make_float4(a[0], a[1], a[2], a[3]);
    *reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(K.use) + i0) = use;
  }
  const int64_t stride = (int64_t)gridDim.x * gridDim.y * kBtProThreads;
  const int64_t me = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kBtProThreads + threadIdx.x;
  const int64_t m16 = n_match >> 2;
  for (int64_t i = me; i < m16; i += stride) reinterpret_cast<int4*>(match)[i] = make_int4(-1, -1, -1, -1);
  for (int64_t i = m16 * 4 + me; i < n_match; i += stride) match[i] = -1;
  for (int64_t i = me; i < (n_cnt >> 2); i += stride) reinterpret_cast<int4*>(cnt)[i] = make_int4(0, 0, 0, 0);
}

void launch_bt_prologue(hipStream_t s, const BtKfDev* tab, const BtProKf* pro, int n_kf, int n_max, int32_t* match, int64_t n_match, int32_t* cnt,
                        int n_cnt) {
  static_assert(sizeof(LocalPointPod) == 72 && sizeof(dvm_keypoint_pod) == 28 && sizeof(BtProKf) == 32, "what BtProKf's comments state");
  if (n_kf < 1) return;
  const unsigned by = (unsigned)std::max(1, (n_max + kBtProSpan - 1) / kBtProSpan);
  hipLaunchKernelGGL(k_bt_prologue, dim3((unsigned)n_kf, by), dim3(kBtProThreads), 0, s, tab, pro, match, n_match, cnt, n_cnt);
}

void launch_bt_search(hipStream_t s, const BtKfDev* tab, int n_targets, int n1, int fv_n1, float nnratio, int32_t* match, int8_t* bin, int32_t* cnt) {
  const int64_t pairs = (int64_t)n_targets * fv_n1;
  if (pairs < 1) return;
  hipLaunchKernelGGL(k_bt_search, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, s, tab, n_targets, n1, fv_n1, nnratio, match, bin, cnt);
}
void launch_bt_settle(hipStream_t s, const BtKfDev* tab, int n_targets, int n1, int check_ori, int32_t* match, const int8_t* bin, const int32_t* cnt,
                      int32_t* nmatches) {
  if (n_targets < 1) return;
  hipLaunchKernelGGL(k_bt_settle, dim3(n_targets), dim3(256), 0, s, tab, n1, check_ori, match, bin, cnt, nmatches);
}

}  // namespace dvm
