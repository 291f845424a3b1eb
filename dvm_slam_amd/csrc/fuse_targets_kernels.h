// dvm_slam_amd/csrc/fuse_targets_kernels.h -- launchers of the Fuse searches of LocalMapping::SearchInNeighbors (fuse_targets_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.h"

namespace dvm {

// one target keyframe inside the handle's device block: its uploaded arrays, its grid span and what k_project_search takes as arguments
struct FtTargetDev {
  const dvm_keypoint_pod* kps;   // [n] as uploaded
  const uint8_t* desc;           // [n][32]
  const float* sf;               // mvScaleFactors [n_levels]
  const float* inv_sigma2;       // mvInvLevelSigma2 [n_levels]; null: the ungated form (DVM_FT_FORM_SCW)
  FrameView F;                   // the target's span of the packed grid arrays (cap = n)
  ProjectCam C;                  // (th is a run argument: C.th is not read)
  int32_t n, model;              // model: dvm_cam::kPinhole (C.fx .. cy) / kKannalaBrandt8 (kb8)
  float kb8[8];                  // mvParameters of a KannalaBrandt8 target
};
struct FtHit { int32_t point, idx, dist; };   // == dvm_ft_hit
struct FtPoints {   // the point table of one run (device pointers)
  const float *pos, *normal, *min_dist, *max_dist;
  const uint8_t *desc, *valid, *skip;   // valid [n] / skip [T * n] may be null
  int32_t n;
};
void launch_ft_build(hipStream_t s, const FtTargetDev* targets, int n_targets);
// order [n_pinhole + n_kb8]: the targets' indices, the pinhole targets first: one launch per model type present, blockIdx.y walks its part
// of the list (rows are independent, so a mixed call is two launches over disjoint rows)
void launch_ft_search(hipStream_t s, const FtTargetDev* targets, const int32_t* order, int n_pinhole, int n_kb8, const FtPoints& P, float th,
                      int32_t* best_idx, int32_t* best_dist);
// the hits of dense rows [n_targets][n], stable, in three launches (count per target, scan over the targets, write): off [n_targets + 1]
// goes to device memory and to off_out, the hits below position cap to hits_out (both may be mapped host memory: plain vector stores)
void launch_ft_hits(hipStream_t s, const int32_t* best_idx, const int32_t* best_dist, int n_targets, int n, int32_t* cnt, int32_t* off,
                    int32_t* off_out, FtHit* hits_out, int cap);
// the scan of launch_ft_hits on its own: off[i] = off_out[i] = cnt[0] + .. + cnt[i - 1], i <= n (fuse_points_kernels.hip scans its blocks with it)
void launch_ft_scan(hipStream_t s, const int32_t* cnt, int n, int32_t* off, int32_t* off_out);

// ---- fuse_points_kernels.hip: the point table of a run from the records of a dvm_map_store (18 words each, `records` = the store's block)
// k_ft_gather: row k < n from records[slot[k]] into the SoA arrays of FtPoints; valid[k] = slot[k] >= 0 && the record is not bad &&
// (valid_in == null || valid_in[k]) && (mark == null || !mark[slot[k]]).  A row at or beyond *n_live (n_live != null) is written invalid
// and its slot is not read.  The arrays of an invalid row hold anything: the search leaves before reading them.
struct FtGather {
  const uint32_t* records;
  const int32_t* slot;
  const uint8_t* valid_in;
  const int32_t* n_live;
  const uint8_t* mark;
  uint32_t *pos, *normal, *min_dist, *max_dist, *desc;   // (bit copies of the records' words)
  uint8_t* valid;
  int32_t n;
};
void launch_ft_gather(hipStream_t s, const FtGather& G);
// the candidate list of dvm_fuse_targets_run_hits_candidates: entry [n_entries] the flat lists, exclude [n_exclude]; first [map capacity]
// (idle: every word kFtFirstIdle) and mark [map capacity] (idle: zero) are the handle's per-slot tables
constexpr int32_t kFtFirstIdle = 0x7f7f7f7f;   // (what a byte-wise memset writes; above every flat index)
struct FtCand {
  const uint32_t* records;
  const int32_t *entry, *exclude;
  int32_t n_entries, n_exclude;
  int32_t* first;
  uint8_t* mark;
};
// mark (first[slot] = the lowest flat index of a non-bad entry naming it; mark[exclude[j]] = 1), count per block of 256 entries, scan
// (off [blocks + 1] to device memory and to off_out: off[blocks] is the list's length), write (stable: cand[p] to device memory, and to
// cand_out where p < cap).  cnt / off: [blocks] / [blocks + 1] device words, blocks = ceil(n_entries / 256)
void launch_ft_candidates(hipStream_t s, const FtCand& C, int32_t* cnt, int32_t* off, int32_t* off_out, int32_t* cand, int32_t* cand_out, int cap);
// both tables back to idle through the entries the call touched
void launch_ft_cand_reset(hipStream_t s, const FtCand& C);

}  // namespace dvm
