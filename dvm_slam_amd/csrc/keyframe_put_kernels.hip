// dvm_slam_amd/csrc/keyframe_put_kernels.hip -- the kernels of dvm_keyframe_store_put_device (include/dvmslam_hip.h): a keyframe whose
// mvKeysUn and descriptors are in device memory already enters its slot without a per-keypoint byte crossing the bus.  Per call, on the
// store's stream:
//   k_kfs_dev_check   one workgroup per keyframe: the count (*d_n against the arrays' capacity and slot_keypoints) and every octave
//                     against the level tables -- the two things the host cannot see.  It raises the call's flag (KfsDevHead::flag).
//   k_vocab_transform (match_kernels.hip, as it is) per keyframe: word, node and weight of every feature into the store's scratch
//   k_kfs_dev_bow     one 1 024-thread workgroup per keyframe: KeyFrame::ComputeBoW's bookkeeping as k_refkf_bow does it (block_sort.h),
//                     the FeatureVector written into the slot, the BowVector and a copy of the FeatureVector to mapped memory
//   k_kfs_dev_put     one 1 024-thread workgroup per keyframe: keypoints, descriptors and the three level tables into the slot, and the
//                     slot's grid by frame_build_block (proj_device.h), the function k_kfs_put calls -- built from the SOURCE arrays,
//                     which nothing writes during the launch, so k_kfs_put's argument holds: no ordering against the workgroup's own copy.
// The two kernels behind the flag return at once when it is set: a refused call writes no slot.
// k_kfs_dev_bow and k_kfs_dev_put stay two kernels: the sort takes 16 B per entry of dynamic LDS (128 KB at 8 192 keypoints),
// frame_build_block 32 KB of static LDS for its keys, and the two with the scan's few words exceed the 160 KB a workgroup can have.
// No index is formed from an unchecked value: a count is clamped to the arrays' capacity and to slot_keypoints before anything reads by it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_sort.h"
#include "keyframe_store.h"
#include "orb_kernels.h"   // raise_dynamic_lds
#include "proj_device.h"

namespace dvm {

namespace {
// bytes: a multiple of 4; dst a multiple of 16.  16 bytes per thread and step when src is a multiple of 16 too, else dwords.
__device__ __forceinline__ void kfs_dev_move(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, size_t bytes) {
  const size_t n4 = bytes >> 2;
  uint32_t* dw = reinterpret_cast<uint32_t*>(dst);
  const uint32_t* sw = reinterpret_cast<const uint32_t*>(src);
  size_t done4 = 0;
  if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
    const size_t n16 = bytes >> 4;
    uint4* d = reinterpret_cast<uint4*>(dst);
    const uint4* s = reinterpret_cast<const uint4*>(src);
    for (size_t i = threadIdx.x; i < n16; i += 1024) d[i] = s[i];
    done4 = n16 * 4;
  }
  for (size_t i = done4 + threadIdx.x; i < n4; i += 1024) dw[i] = sw[i];
}
template <class T> __device__ __forceinline__ T* at_bytes(T* p, size_t bytes) {
  return reinterpret_cast<T*>(reinterpret_cast<uint8_t*>(p) + bytes);
}
}  // namespace

__global__ void __launch_bounds__(256) k_kfs_dev_check(KfsDevHead* __restrict__ head, KfsDevItem* __restrict__ items, int K,
                                                       KfsDevRes* __restrict__ res, size_t res_stride) {
  const int k = blockIdx.x;
  KfsDevItem& it = items[k];
  const int cap = it.cap, nl = it.n_levels;
  int n = it.d_n ? min(*it.d_n, cap) : cap;
  n = max(n, 0);
  const bool over = n > K;
  const dvm_keypoint_pod* kps = it.kps;
  int bad = 0;
  if (!over)
    for (int i = threadIdx.x; i < n; i += 256) bad |= (uint32_t)kps[i].octave >= (uint32_t)nl ? 1 : 0;
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    it.count = over || bad ? 0 : n;
    at_bytes(res, (size_t)k * res_stride)->n = n;
    if (over || bad) atomicMin(&head->flag, (k << 1) | (over ? 0 : 1));
  }
}

// Frame::ComputeBoW's bookkeeping on k_vocab_transform's per-feature results, as k_refkf_bow (track_kernels.hip) does it: the features
// with weight > 0 only; BowVector: sort (word << 32 | feature), each word's weight the sum of its features' weights in feature order,
// the L1 norm in ascending word order (both sequential double additions), each value divided by the norm; FeatureVector: sort
// ((unsigned)node << 32 | feature).  LDS: 16 B per entry of the sort (P: slot_keypoints rounded up to a power of two).
__global__ void __launch_bounds__(1024) k_kfs_dev_bow(const KfsDevHead* __restrict__ head, const KfsDevItem* __restrict__ items, int first, int K, int P,
                                                      KfsDevScratch W, KfSlotLayout L, KfsDevOut O, size_t out_stride) {
  if (head->flag != kKfsDevNoFlag) return;
  extern __shared__ __attribute__((aligned(16))) uint8_t kfs_smem[];
  uint64_t* keys = reinterpret_cast<uint64_t*>(kfs_smem);      // [P]
  double* vals = reinterpret_cast<double*>(keys + P);          // [P]
  __shared__ int s_wave[16];
  __shared__ int s_m;
  __shared__ double s_norm;
  const int tid = threadIdx.x, r = blockIdx.x;
  const KfsDevItem& it = items[first + r];
  const int N = min(it.count, K);
  const int32_t* word = W.word + (size_t)r * K;
  const int32_t* node = W.node + (size_t)r * K;
  const double* w = W.w + (size_t)r * K;
  const size_t ob = (size_t)r * out_stride;
  KfsDevRes* res = at_bytes(O.res, ob);
  int32_t* h_bow_ids = at_bytes(O.bow_ids, ob); double* h_bow_vals = at_bytes(O.bow_vals, ob);
  int32_t *h_fv_node = at_bytes(O.fv_node, ob), *h_fv_off = at_bytes(O.fv_off, ob), *h_fv_feat = at_bytes(O.fv_feat, ob);
  int32_t* fv_node = reinterpret_cast<int32_t*>(it.slot + L.fv_node);
  int32_t* fv_off = reinterpret_cast<int32_t*>(it.slot + L.fv_off);
  int32_t* fv_feat = reinterpret_cast<int32_t*>(it.slot + L.fv_feat);
  if (tid == 0) s_m = 0;
  __syncthreads();
  int m = 0;
  for (int i = tid; i < P; i += 1024) {
    const bool keep = i < N && w[i] > 0.0;
    keys[i] = keep ? ((uint64_t)(uint32_t)word[i] << 32) | (uint32_t)i : ~0ull;
    m += keep ? 1 : 0;
  }
  if (m) atomicAdd(&s_m, m);
  __syncthreads();
  const int M = s_m;
  bitonic_sort(keys, P);
  // BowVector: one thread per word adds its features' weights in feature order
  const int n_bow = for_each_run(keys, M, s_wave, [&](int run, int start) {
    const uint32_t wd = (uint32_t)(keys[start] >> 32);
    double v = w[(uint32_t)keys[start]];
    for (int i = start + 1; i < M && (uint32_t)(keys[i] >> 32) == wd; i++) v += w[(uint32_t)keys[i]];
    vals[run] = v;
    h_bow_ids[run] = (int32_t)wd;
  });
  __syncthreads();
  if (tid == 0) {
    double norm = 0.0;
    for (int i = 0; i < n_bow; i++) norm += fabs(vals[i]);
    s_norm = norm;
  }
  __syncthreads();
  const double norm = s_norm;
  for (int i = tid; i < n_bow; i += 1024) h_bow_vals[i] = norm > 0.0 ? vals[i] / norm : vals[i];
  __syncthreads();
  // FeatureVector
  for (int i = tid; i < P; i += 1024) {
    const bool keep = i < N && w[i] > 0.0;
    keys[i] = keep ? ((uint64_t)(uint32_t)node[i] << 32) | (uint32_t)i : ~0ull;
  }
  __syncthreads();
  bitonic_sort(keys, P);
  const int n_fv = for_each_run(keys, M, s_wave, [&](int run, int start) {
    const int32_t nd = (int32_t)(uint32_t)(keys[start] >> 32);
    fv_node[run] = nd; fv_off[run] = start;
    h_fv_node[run] = nd; h_fv_off[run] = start;
  });
  for (int i = tid; i < M; i += 1024) {
    const int32_t f = (int32_t)(uint32_t)keys[i];
    fv_feat[i] = f; h_fv_feat[i] = f;
  }
  if (tid == 0) {
    if (n_fv > 0) fv_off[n_fv] = M;     // (fv_n == 0: the slot gets no fv_off, as put stages none)
    h_fv_off[n_fv] = M;
    res->n_bow = n_bow; res->n_fv = n_fv; res->n_feat = M;
  }
}

__global__ void __launch_bounds__(1024) k_kfs_dev_put(const KfsDevHead* __restrict__ head, const KfsDevItem* __restrict__ items, int first,
                                                      KfSlotLayout L, KfsDevRes* __restrict__ res, size_t res_stride) {
  const int flag = head->flag;
  if (threadIdx.x == 0) at_bytes(res, (size_t)blockIdx.x * res_stride)->flag = flag;
  if (flag != kKfsDevNoFlag) return;
  const KfsDevItem& it = items[first + blockIdx.x];
  const int n = it.count, nl = it.n_levels;
  const uint8_t* s_kps = reinterpret_cast<const uint8_t*>(it.kps);
  const uint8_t* s_desc = it.desc;
  uint8_t* slot = it.slot;
  kfs_dev_move(slot + L.kps, s_kps, (size_t)n * kKfsKeypointBytes);
  kfs_dev_move(slot + L.desc, s_desc, (size_t)n * 32);
  if ((int)threadIdx.x < nl) {
    reinterpret_cast<float*>(slot + L.sf)[threadIdx.x] = it.sf[threadIdx.x];
    reinterpret_cast<float*>(slot + L.sigma2)[threadIdx.x] = it.sigma2[threadIdx.x];
    reinterpret_cast<float*>(slot + L.inv_sigma2)[threadIdx.x] = it.inv_sigma2[threadIdx.x];
  }
  FrameView F;
  F.skp = reinterpret_cast<float4*>(slot + L.skp);
  F.sidx = reinterpret_cast<int32_t*>(slot + L.sidx);
  F.sdesc = slot + L.sdesc;
  F.cell_start = reinterpret_cast<int32_t*>(slot + L.cell_start);
  F.n_sorted = reinterpret_cast<int32_t*>(slot + L.counters);
  F.n_total = F.n_sorted + 1;
  F.n_overflow = F.n_sorted + 2;
  F.cap = n;
  F.minX = it.minX; F.minY = it.minY; F.wInv = it.wInv; F.hInv = it.hInv;
  frame_build_block(it.kps, s_desc, n, F);
}

void launch_kfs_dev_check(hipStream_t s, KfsDevHead* head, KfsDevItem* items, int n_items, int K, KfsDevRes* res, size_t res_stride) {
  if (n_items > 0) hipLaunchKernelGGL(k_kfs_dev_check, dim3(n_items), dim3(256), 0, s, head, items, K, res, res_stride);
}
bool launch_kfs_dev_bow(hipStream_t s, const KfsDevHead* head, const KfsDevItem* items, int first, int m, int K, const KfsDevScratch& W,
                        const KfSlotLayout& L, const KfsDevOut& out0, size_t out_stride) {
  int P = 1;
  while (P < K) P <<= 1;
  const size_t lds = (size_t)P * 16;
  if (lds > 48 * 1024 && !raise_dynamic_lds(reinterpret_cast<const void*>(k_kfs_dev_bow), (int)lds)) return false;
  if (m > 0) hipLaunchKernelGGL(k_kfs_dev_bow, dim3(m), dim3(1024), lds, s, head, items, first, K, P, W, L, out0, out_stride);
  return true;
}
void launch_kfs_dev_put(hipStream_t s, const KfsDevHead* head, const KfsDevItem* items, int first, int m, const KfSlotLayout& L, KfsDevRes* res0,
                        size_t res_stride) {
  static_assert(sizeof(dvm_keypoint_pod) == kKfsKeypointBytes && kCellStartStride == (int)kKfsCellStart, "kf_store_layout.h restates these");
  if (m > 0) hipLaunchKernelGGL(k_kfs_dev_put, dim3(m), dim3(1024), 0, s, head, items, first, L, res0, res_stride);
}

}  // namespace dvm
