// dvm_slam_amd/csrc/ba_resident_lists.h -- host side of dvm_ba_resident_optimize's prepare step: a point's edges IN THE CALLER'S ORDER
// (MapPoint::GetObservations() order: the order UpdateNormalAndDepth sums the normal in; the cluster tables' pt_edges is in the sorted
// order), and the checks of ref_edge.  Pure host code, no HIP: tools/check_ba_resident_lists.cpp walks it under the sanitizers
// (tests/test_ba_resident_lists.py).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/dvmslam_hip.h"

namespace dvm {

struct ResidentLists {
  std::vector<int32_t> pe_start, pe_edges;   // [L + 1], [E]: point l's edges are pe_edges[pe_start[l] .. pe_start[l + 1]), ascending
};

// 0: built.  1: an edge's pose outside [0, P) or its point outside [0, L) (nothing usable built).
inline int resident_lists_build(const dvm_ba_obs* obs, int P, int L, int E, ResidentLists& r) {
  r.pe_start.assign((size_t)L + 1, 0);
  r.pe_edges.assign((size_t)E, 0);
  for (int e = 0; e < E; e++) {
    if (obs[e].pose < 0 || obs[e].pose >= P || obs[e].point < 0 || obs[e].point >= L) return 1;
    r.pe_start[(size_t)obs[e].point + 1]++;
  }
  for (int l = 0; l < L; l++) r.pe_start[(size_t)l + 1] += r.pe_start[l];
  std::vector<int32_t> fill(r.pe_start.begin(), r.pe_start.end() - 1);
  for (int e = 0; e < E; e++) r.pe_edges[(size_t)fill[obs[e].point]++] = e;   // (a counting sort by point: stable, so ascending per point)
  return 0;
}

// ref_edge[l] must be an edge of point l; -1 is legal on a point without edges only.  0: fine; 1: out of range; 2: not an edge of
// point l; 3: -1 on a point that has edges.  *at: the first offending point.
inline int resident_ref_check(const dvm_ba_obs* obs, int L, int E, const ResidentLists& r, const int32_t* ref_edge, int* at) {
  for (int l = 0; l < L; l++) {
    const int32_t re = ref_edge[l];
    const bool used = r.pe_start[(size_t)l + 1] > r.pe_start[l];
    int bad = 0;
    if (re == -1) bad = used ? 3 : 0;
    else if (re < 0 || re >= E) bad = 1;
    else if (obs[re].point != l) bad = 2;
    if (bad) { if (at) *at = l; return bad; }
  }
  return 0;
}

}  // namespace dvm
