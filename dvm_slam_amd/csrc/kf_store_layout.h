// dvm_slam_amd/csrc/kf_store_layout.h -- the byte layout of one slot of dvm_keyframe_store (keyframe_store.cpp), written ONCE: the offsets
// of a slot's arrays from the slot's base and the slot stride, as functions of slot_keypoints.  Every array begins at a multiple of 64
// bytes and is sized for the largest keyframe the slot admits (n = fv_n = features = slot_keypoints, 64 levels).  Host-only and free of
// HIP headers: the store includes it, and so does tools/check_kf_store_layout.cpp, which walks it as a plain program.  The three
// constants below restate kernel-side ones; keyframe_store.cpp asserts that they agree.
#pragma once
#include <cstddef>
#include <cstdint>

namespace dvm {

constexpr size_t kKfsAlign = 64;
constexpr size_t kKfsKeypointBytes = 28;     // sizeof(dvm_keypoint)
constexpr size_t kKfsCellStart = 3076;       // kCellStartStride (match_kernels.h): 64 x 48 cells + 1, rounded to 16 bytes
constexpr size_t kKfsLevels = 64;            // the longest level table
constexpr size_t kKfsCounters = 4;           // n_sorted, n_total, n_overflow, one spare

struct KfSlotLayout {
  // as put
  size_t kps, desc, fv_node, fv_off, fv_feat, sf, sigma2, inv_sigma2;
  // the FrameView span k_kfs_put builds
  size_t skp, sidx, sdesc, cell_start, counters;
  size_t stride;                              // bytes from one slot to the next
};

constexpr size_t kfs_pad(size_t b) { return (b + kKfsAlign - 1) & ~(kKfsAlign - 1); }

// the bytes of each array at K = slot_keypoints, in the order of KfSlotLayout's members
struct KfSlotBytes { size_t kps, desc, fv_node, fv_off, fv_feat, sf, sigma2, inv_sigma2, skp, sidx, sdesc, cell_start, counters; };
constexpr KfSlotBytes kf_slot_bytes(size_t K) {
  return KfSlotBytes{K * kKfsKeypointBytes, K * 32, K * 4, (K + 1) * 4, K * 4, kKfsLevels * 4, kKfsLevels * 4, kKfsLevels * 4,
                     K * 16, K * 4, K * 32, kKfsCellStart * 4, kKfsCounters * 4};
}
constexpr KfSlotLayout kf_slot_layout(size_t K) {
  const KfSlotBytes b = kf_slot_bytes(K);
  KfSlotLayout l{};
  size_t at = 0;
  l.kps = at; at += kfs_pad(b.kps);
  l.desc = at; at += kfs_pad(b.desc);
  l.fv_node = at; at += kfs_pad(b.fv_node);
  l.fv_off = at; at += kfs_pad(b.fv_off);
  l.fv_feat = at; at += kfs_pad(b.fv_feat);
  l.sf = at; at += kfs_pad(b.sf);
  l.sigma2 = at; at += kfs_pad(b.sigma2);
  l.inv_sigma2 = at; at += kfs_pad(b.inv_sigma2);
  l.skp = at; at += kfs_pad(b.skp);
  l.sidx = at; at += kfs_pad(b.sidx);
  l.sdesc = at; at += kfs_pad(b.sdesc);
  l.cell_start = at; at += kfs_pad(b.cell_start);
  l.counters = at; at += kfs_pad(b.counters);
  l.stride = at;
  return l;
}

// what one keyframe takes in the staging block at most (its eight put arrays, each rounded up), and exactly for given counts
constexpr size_t kf_stage_bytes(size_t n, size_t fv_n, size_t n_feat, size_t n_levels) {
  return kfs_pad(n * kKfsKeypointBytes) + kfs_pad(n * 32) + kfs_pad(fv_n * 4) + kfs_pad(fv_n ? (fv_n + 1) * 4 : 0) + kfs_pad(n_feat * 4) +
         3 * kfs_pad(n_levels * 4);
}
constexpr size_t kf_stage_bytes_max(size_t K) { return kf_stage_bytes(K, K, K, kKfsLevels); }

}  // namespace dvm
