// tests/bow_shim_driver/bow_shim_driver.cpp -- TEST INFRASTRUCTURE: runs SearchByBoWCovisibles (host/LoopClosing_shim.h) -- the BoW
// searches of LoopClosing::DetectCommonRegionsFromBoW (src/LoopClosing.cc:708-747) for all candidates in one device call -- on a mock
// world and hands everything it returns back as indices into the world's tables.  tests/test_gpu_bow_targets_shim.py compares that with
// :708-747 restated in Python around the oracle.
#include "../shim_driver/shim_driver.cpp"

#include "LoopClosing_shim.h"

extern "C" {

// lists: the keyframes of all vpCovKFi back to back (-1: a null pointer), list c = lists[list_off[c] .. list_off[c + 1]); N = the
// current keyframe's keypoints.  Per list entry e: n_e[e] = SearchByBoW's return value, row_size[e] = vvpMatchedMPs[j].size(),
// mp_rows / idx2_rows [e][N] (map point index / keypoint of the covisible, -1: none).  Per list c: summary[c] = {nMostBoWNumMatches,
// nIndexMostBoWMatchesKF, numBoWMatches}, matched_mp / matched_kf [c][N] = vpMatchedPoints / vpKeyFrameMatchedMP.
int swb_search_covisibles(World* w, int cur, const int32_t* lists, const int32_t* list_off, int n_lists, float nnratio, int check_ori, int32_t* n_e,
                          int32_t* row_size, int32_t* mp_rows, int32_t* idx2_rows, int32_t* summary, int32_t* matched_mp, int32_t* matched_kf) {
  return guarded(w, [&] {
    KeyFrame* pCurrentKF = w->kfs[cur].get();
    const size_t N = pCurrentKF->GetMapPointMatches().size();
    std::vector<std::vector<KeyFrame*>> vvpCovKFs((size_t)n_lists);
    for (int c = 0; c < n_lists; c++)
      for (int e = list_off[c]; e < list_off[c + 1]; e++) vvpCovKFs[c].push_back(lists[e] < 0 ? nullptr : w->kfs[lists[e]].get());
    const std::vector<BoWCovisibleMatches> out = SearchByBoWCovisibles(pCurrentKF, vvpCovKFs, nnratio, check_ori != 0);
    if ((int)out.size() != n_lists) throw std::runtime_error("one result per list expected");
    for (int c = 0; c < n_lists; c++) {
      const BoWCovisibleMatches& B = out[c];
      for (size_t j = 0; j < vvpCovKFs[c].size(); j++) {
        const size_t e = (size_t)list_off[c] + j;
        n_e[e] = B.vnMatches[j];
        row_size[e] = (int32_t)B.vvpMatchedMPs[j].size();
        if (B.vvnMatchIdx2[j].size() != B.vvpMatchedMPs[j].size()) throw std::runtime_error("the index row and the point row differ in length");
        for (size_t i = 0; i < N; i++) {
          const bool has = i < B.vvpMatchedMPs[j].size();
          mp_rows[e * N + i] = has ? w->mp_index(B.vvpMatchedMPs[j][i]) : -1;
          idx2_rows[e * N + i] = has ? B.vvnMatchIdx2[j][i] : -1;
        }
      }
      summary[3 * c] = B.nMostBoWNumMatches; summary[3 * c + 1] = B.nIndexMostBoWMatchesKF; summary[3 * c + 2] = B.numBoWMatches;
      if (B.vpMatchedPoints.size() != N || B.vpKeyFrameMatchedMP.size() != N) throw std::runtime_error("vpMatchedPoints: one entry per keypoint expected");
      for (size_t i = 0; i < N; i++) {
        matched_mp[(size_t)c * N + i] = w->mp_index(B.vpMatchedPoints[i]);
        matched_kf[(size_t)c * N + i] = B.vpKeyFrameMatchedMP[i] ? w->kf_index(B.vpKeyFrameMatchedMP[i]) : -1;
      }
    }
    return 0;
  });
}

}  // extern "C"
