// dvm_slam_amd/csrc/fv_once.h -- the listed-once rule of a FeatureVector: every feature lies in at most ONE node.  k_bt_search rests on it
// (a claim made in one node never reaches another); dvm_search_by_bow_targets checks it per call, dvm_keyframe_store_put records it per
// slot with this scan, and dvm_search_by_bow_targets_resident refuses a slot where it does not hold.  Host-only and free of HIP headers:
// the store includes it, and so does tools/check_fv_once.cpp, which walks it as a plain program.
#pragma once
#include <cstdint>
#include <cstring>

namespace dvm {

// fv_feat [n_feat]: the features of all nodes back to back, each in [0, n) (the caller has checked); seen [>= n]: scratch.
// Returns the first feature listed a second time, or -1 when every feature is listed at most once.
inline int32_t fv_first_repeat(const int32_t* fv_feat, int32_t n_feat, int32_t n, uint8_t* seen) {
  if (n_feat < 2) return -1;
  std::memset(seen, 0, (size_t)n);
  for (int32_t p = 0; p < n_feat; p++) {
    const int32_t i = fv_feat[p];
    if (seen[i]) return i;
    seen[i] = 1;
  }
  return -1;
}

}  // namespace dvm
