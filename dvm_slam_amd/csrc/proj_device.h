// dvm_slam_amd/csrc/proj_device.h -- device code the searches over a feature grid share: the grid build of one frame (k_frame_build,
// k_ft_build), the best two of a window by one DPP row (window_top2: k_match_window, k_project_search, k_ft_search; the scan itself is
// window_scan of match_device.h) and the projection of one map point into a keyframe with its window search (k_project_search,
// k_ft_search).  One definition each: a kernel that batches the work of another calls the function the other calls, so their results
// agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "camera_model.h"
#include "match_device.h"
#include "match_kernels.h"
#include "pose_f32.h"

namespace dvm {

constexpr uint32_t kInvalidKey = 0xFFFFFFFFu;

// One workgroup (1024 threads) builds the grid of one frame: bitonic sort of (cell << 13 | idx) keys in LDS, then gather into F's arrays
// (sorted by grid column, grid row, keypoint index -- the order in which GetFeaturesInArea enumerates candidates).  n <= F.cap <= kFrameCap.
__device__ __forceinline__ void frame_build_block(const dvm_keypoint_pod* __restrict__ kps, const uint8_t* __restrict__ desc, int n,
                                                  const FrameView& F) {
  __shared__ uint32_t keys[kFrameCap];
  const int tid = threadIdx.x;
  int P = 64;
  while (P < n) P <<= 1;
  for (int i = tid; i < P; i += 1024) {
    uint32_t key = kInvalidKey;
    if (i < n) {
      const dvm_keypoint_pod kp = kps[i];
      // PosInGrid: round() = half away from zero; keypoints outside the grid are not indexed
      int px = (int)roundf((kp.x - F.minX) * F.wInv);
      int py = (int)roundf((kp.y - F.minY) * F.hInv);
      if (px >= 0 && px < kGridCols && py >= 0 && py < kGridRows) key = ((uint32_t)(px * kGridRows + py) << 13) | (uint32_t)i;
    }
    keys[i] = key;
  }
  __syncthreads();
  // A wave owns the 64-aligned blocks of its lanes (i = tid + 1024 t), so a stage with partner distance j < 64 only touches keys
  // the same wave wrote: between two such stages the wave's own LDS order is enough.  The workgroup barrier (16 waves, ~0.25 us,
  // and the sort is 55 stages for 1 024 keys) stays where a stage reads or has written across waves: 14 of the 55.
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += 1024) {
        int ixj = i ^ j;
        if (ixj > i) {
          uint32_t a = keys[i], b = keys[ixj];
          bool up = ((i & k) == 0);
          if ((a > b) == up) { keys[i] = b; keys[ixj] = a; }
        }
      }
      const int jn = j > 1 ? (j >> 1) : k;   // partner distance of the next stage (stage k << 1 opens with j = k)
      if (j >= 64 || jn >= 64) {
        __syncthreads();
      } else {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  // number of indexed keypoints = first invalid key (binary search by thread 0 is fine: log2(8192))
  __shared__ int s_m;
  if (tid == 0) {
    int lo = 0, hi = P;
    while (lo < hi) {
      int mid = (lo + hi) >> 1;
      if (keys[mid] == kInvalidKey) hi = mid; else lo = mid + 1;
    }
    s_m = lo;
    *F.n_sorted = lo;
    *F.n_total = n;
  }
  __syncthreads();
  const int m = s_m;
  {  // cell_start[c] = first sorted position whose cell >= c = the number of keys below c << 13, for all kGridCells + 1 entries on every
     // build (nothing of an earlier build stays).  Three cells per thread, their lower bounds side by side in steps of falling powers of
     // two over keys[0 .. P): an invalid key is above every cell's, so the search needs no m.
    const uint32_t w0 = (uint32_t)tid << 13, w1 = (uint32_t)(tid + 1024) << 13, w2 = (uint32_t)(tid + 2048) << 13;
    int l0 = 0, l1 = 0, l2 = 0;
    for (int s = P; s > 0; s >>= 1) {
      const bool in0 = l0 + s <= P, in1 = l1 + s <= P, in2 = l2 + s <= P;
      const uint32_t k0 = keys[in0 ? l0 + s - 1 : 0], k1 = keys[in1 ? l1 + s - 1 : 0], k2 = keys[in2 ? l2 + s - 1 : 0];
      if (in0 && k0 < w0) l0 += s;
      if (in1 && k1 < w1) l1 += s;
      if (in2 && k2 < w2) l2 += s;
    }
    F.cell_start[tid] = l0;
    F.cell_start[tid + 1024] = l1;
    F.cell_start[tid + 2048] = l2;
    if (tid == 0) F.cell_start[kGridCells] = m;
  }
  for (int p = tid; p < m; p += 1024) {
    const uint32_t key = keys[p];
    const int i = (int)(key & 0x1FFFu);
    const dvm_keypoint_pod kp = kps[i];
    F.skp[p] = make_float4(kp.x, kp.y, __int_as_float(kp.octave), __int_as_float((int)(key >> 13)));
    F.sidx[p] = i;
    const uint4* s = reinterpret_cast<const uint4*>(desc + (size_t)i * 32);
    uint4* d = reinterpret_cast<uint4*>(F.sdesc + (size_t)p * 32);
    d[0] = s[0];
    d[1] = s[1];
  }
}

// GetFeaturesInArea(x, y, r, minLevel, maxLevel) of frame F scanned by one DPP row (window_scan<16>, match_device.h): best / second best
// (dist << 16 | sorted position) after the row reduction, identical on all 16 lanes.  gate_inv_sigma2 != nullptr adds the
// per-candidate reprojection gate of ORBmatcher::Fuse (ORBmatcher.cc:1187-1196): skip if (ex^2 + ey^2) * invSigma2[octave]
// > gate (the comparison is made in double there: 5.99 is a double literal).
__device__ __forceinline__ void window_top2(const FrameView& F, float x, float y, float r, int minLevel, int maxLevel,
                                            const uint8_t* __restrict__ qdesc32, const uint8_t* __restrict__ skip,
                                            const float* __restrict__ gate_inv_sigma2, double gate, int lane, uint32_t& k1_out,
                                            uint32_t& k2_out) {
  uint32_t k1 = (256u << 16) | 0xFFFFu, k2 = k1;
  uint32_t w[8];
  desc_load(qdesc32, 0, w);
  window_scan<16>(F, x, y, r, minLevel, maxLevel, lane, [&](int p, int oct, float dx, float dy) {
    if (skip && skip[F.sidx[p]]) return;
    if (gate_inv_sigma2) {
      const float e2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
      if ((double)__fmul_rn(e2, gate_inv_sigma2[oct]) > gate) return;
    }
    top2_insert(k1, k2, ((uint32_t)desc_distance(w, F.sdesc, p) << 16) | (uint32_t)p);
  });
  row_top2(k1, k2);
  k1_out = k1; k2_out = k2;
}

// One map point against one keyframe, by one DPP row (every lane repeats the projection): depth > 0, KeyFrame::IsInImage, distance inside
// the scale-invariance range, viewing angle < 60 deg (PO.Pn >= 0.5 dist), MapPoint::PredictScale, radius = th * scaleFactor[level],
// candidates of octave [level-1, level] (ORBmatcher.cc:1089-1210 and the variants ProjectCam::sim3_pair selects), then window_top2.
// ok: the point takes part at all (the caller's valid / skip flags).  k1 / k2: best and second best, identical on the 16 lanes.
struct ProjectRow {
  uint32_t k1, k2;
  float u, v, r;
  int level;
};
// MODEL: the camera behind pCamera->project.  The pinhole instantiation is what every chain calls; KannalaBrandt8 (k_project_search_kb8
// only) reads mvParameters from kb8 (camera_model.h) and none of C.fx, fy, cx, cy -- except in the sim3_pair == 1 form, where the
// reference writes the pinhole formula inline whatever the camera (ORBmatcher.cc:1401-1406) and kb8[0..3] stand for fx, fy, cx, cy.
template <int MODEL = dvm_cam::kPinhole>
__device__ __forceinline__ ProjectRow project_row(const FrameView& F, const uint8_t* __restrict__ skip, const ProjectCam& C, float th,
                                                  const float* __restrict__ P, const float* __restrict__ normal,
                                                  const float* __restrict__ min_dist, const float* __restrict__ max_dist,
                                                  const uint8_t* __restrict__ desc, bool ok, int i, const float* __restrict__ scale_factors,
                                                  const float* __restrict__ gate_inv_sigma2, double gate, int lane,
                                                  const float* kb8 = nullptr) {
  float out_u = -1.f, out_v = -1.f, out_r = 0.f;
  int out_level = -1;
  const float p0 = P[3 * i], p1 = P[3 * i + 1], p2 = P[3 * i + 2];
  // p3Dc = Tcw * p3Dw: Sophus' quaternion form (so3.hpp:356-367), never a rotation matrix
  const float pw[3] = {p0, p1, p2};
  float pc[3];
  dvm_pose::se3_apply(C.q, C.t, pw, pc);
  float X = pc[0], Y = pc[1], Z = pc[2];
  float u, v;
  if (C.sim3_pair == 1) {   // SearchBySim3 (:1395-1411): p3Dc2 = S21 * (T1w * p3Dw); u = fx * (X * invz) + cx with invz = 1.0 / Z
    float p2c[3];
    dvm_pose::sim3_apply(C.q2, C.t2, pc, p2c);
    X = p2c[0]; Y = p2c[1]; Z = p2c[2];
    const float invz = (float)(1.0 / (double)Z);
    if constexpr (MODEL == dvm_cam::kKannalaBrandt8) {
      u = kb8[0] * (X * invz) + kb8[2];
      v = kb8[1] * (Y * invz) + kb8[3];
    } else {
      u = C.fx * (X * invz) + C.cx;
      v = C.fy * (Y * invz) + C.cy;
    }
  } else if constexpr (MODEL == dvm_cam::kKannalaBrandt8) {
    dvm_cam::kb8_project(kb8, X, Y, Z, u, v);
  } else {
    u = C.fx * X / Z + C.cx;
    v = C.fy * Y / Z + C.cy;
  }
  // sim3_pair == 2: SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (:1750-1860) -- no depth test, bounds
  // inclusive at both ends
  const bool reloc = C.sim3_pair == 2;
  const bool in_strict = u >= C.min_x && u < C.max_x && v >= C.min_y && v < C.max_y;
  const bool in_loose = !(u < C.min_x || u > C.max_x) && !(v < C.min_y || v > C.max_y);
  const bool front = !(Z < 0.0f);
  ok = ok && (reloc ? in_loose : (front && in_strict));
  if (ok) {
    const float maxDistance = 1.2f * max_dist[i], minDistance = 0.8f * min_dist[i];
    float q0 = p0 - C.Ow[0], q1 = p1 - C.Ow[1], q2 = p2 - C.Ow[2];
    if (C.sim3_pair == 1) { q0 = X; q1 = Y; q2 = Z; }
    const float dist = sqrtf(dvm_pose::sum3(q0 * q0, q1 * q1, q2 * q2));   // Vector3f::norm(): a0 + (a1 + a2)
    ok = !(dist < minDistance || dist > maxDistance);
    if (ok) {
      const float dot = dvm_pose::sum3(q0 * normal[3 * i], q1 * normal[3 * i + 1], q2 * normal[3 * i + 2]);
      ok = C.sim3_pair != 0 || !((double)dot < 0.5 * (double)dist);
      if (ok) {
        const int nScale = dvm_pose::predict_scale(max_dist[i], dist, C.log_scale_factor, C.n_levels);
        out_u = u; out_v = v; out_level = nScale; out_r = th * scale_factors[nScale];
      }
    }
  }
  uint32_t k1 = (256u << 16) | 0xFFFFu, k2 = k1;
  if (out_level >= 0)   // uniform inside the row: all 16 lanes computed the same projection
    window_top2(F, out_u, out_v, out_r, out_level - 1, reloc ? out_level + 1 : out_level, desc + (size_t)i * 32, skip, gate_inv_sigma2, gate, lane, k1, k2);
  ProjectRow R;
  R.k1 = k1; R.k2 = k2; R.u = out_u; R.v = out_v; R.r = out_r; R.level = out_level;
  return R;
}

}  // namespace dvm
