// dvm_slam_amd/csrc/update_local_map_kernels.h -- what update_local_map.cpp hands to update_local_map_kernels.hip: the per-frame parameter
// block that travels up, the call's argument struct, the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dvm {

// one frame of a call (64 B, uploaded): its stores' blocks and its lists inside the upload
struct UlmFrameDev {
  const uint32_t* records;       // the frame's map store: [capacity] records of 18 words, word 17 = bad
  const int32_t* rows;           // the keyframe store's rows of the kind the call reads (OBSERVED: keyframes, MATCHES: points); may be null
  const int32_t* len;            // [kf_capacity] the rows' lengths; null with rows
  int32_t n, n_kfs;              // the frame's keypoints; the named keyframes (points call)
  int32_t kf_capacity, row_words;
  int32_t mp_off, kf_off;        // where mp_slot and kf_slot lie in the upload's lists, in words
  int32_t local_cap, pad[3];
};
static_assert(sizeof(UlmFrameDev) == 64, "the per-frame parameter block");

struct UlmArgs {
  const UlmFrameDev* frames;     // [count]
  const int32_t* lists;          // the upload's lists
  // the handle's per-frame tables, frame b at b * map_capacity; idle between calls: mult 0, first kUlmFirstIdle, pos -1
  int32_t *mult, *first, *pos;
  int32_t map_capacity;
  // the compaction's scratch, frame b at b * (blocks_max + 1): candidates per workgroup, their exclusive scan
  int32_t *cnt, *off;
  int32_t blocks_max, row_blocks;
  // results, in mapped page-locked memory: frame b's votes at b * kf_capacity_res, frame_bad at b * n_pad (bytes), local at
  // b * map_capacity, frame_mp at b * n_pad, counts (n_local, n_outside) at b * 2
  int32_t* votes; uint8_t* frame_bad; int32_t* local; int32_t* frame_mp; int32_t* counts;
  int32_t kf_capacity_res, n_pad;
};

// the vote loop: mult from the frames' lists (and frame_bad), one wavefront per (frame, keyframe slot), mult idle again.
// n_max: the largest frame list; c_max: the largest keyframe-store capacity of the call
void launch_ulm_keyframes(hipStream_t s, const UlmArgs& A, int count, int n_max, int c_max);
// UpdateLocalPoints: mark, count, scan, write (+ pos), frame_mp and n_outside, first and pos idle again.  kfs_max: the largest n_kfs
void launch_ulm_points(hipStream_t s, const UlmArgs& A, int count, int kfs_max);

}  // namespace dvm
