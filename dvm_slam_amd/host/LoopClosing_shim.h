// dvm_slam_amd/host/LoopClosing_shim.h -- the BoW searches of ORB_SLAM3::LoopClosing::DetectCommonRegionsFromBoW
// (src/LoopClosing.cc:644-953) on the HIP library.  For every BoW candidate that survives the tests of :677 and :692-704 the reference
// calls ORBmatcher::SearchByBoW(mpCurrentKF, vpCovKFi[j], vvpMatchedMPs[j]) against the candidate and up to ten of its covisible
// keyframes (:722-731) -- up to 11 blocking calls per candidate, 33 per candidate list, each uploading the current keyframe again.
// SearchByBoWCovisibles runs ALL of them, for all candidates, through ONE dvmh_search_by_bow_targets call (dvm_search_by_bow_targets,
// include/dvmslam_hip.h: one upload, two launches, one synchronisation) and hands back per candidate what :708-747 computes.  The
// candidate loop then reads
//
//   std::vector<std::vector<KeyFrame*>> vvpCovKFs; std::vector<KeyFrame*> vpCand;          // :676-704, unchanged, only collecting
//   for (KeyFrame* pKFi : vpBowCand) { ... build vpCovKFi, bAbortByNearKF ...; vvpCovKFs.push_back(vpCovKFi); vpCand.push_back(pKFi); }
//   const std::vector<BoWCovisibleMatches> vBoW = SearchByBoWCovisibles(mpCurrentKF, vvpCovKFs, 0.9f, true);   // matcherBoW(0.9, true), :657
//   for (size_t c = 0; c < vpCand.size(); c++) {
//     KeyFrame* pKFi = vpCand[c];
//     const BoWCovisibleMatches& B = vBoW[c];
//     KeyFrame* pMostBoWMatchesKF = pKFi;                    // (:713; the commented-out :749 would index vvpCovKFs[c] with B.nIndexMostBoWMatchesKF)
//     if (B.numBoWMatches >= nBoWMatches) { Sim3Solver solver(mpCurrentKF, pMostBoWMatchesKF, B.vpMatchedPoints, bFixedScale, B.vpKeyFrameMatchedMP); ... }
//   }
//
// A snapshot, taken at entry: GetMapPointMatches() of every keyframe and isBad() of every map point are read ONCE while the views are
// gathered, where the reference reads them call by call; LoopClosing holds no lock across its calls either, so both see some state of
// the concurrent LocalMapping thread.  The isBad() test of :736 on the matched points is evaluated on the results, as the reference does.
// Not covered: keyframes of a stereo / fisheye pair (NLeft != -1) -- DVM-SLAM's agents are monocular; they throw.
#pragma once
#include <cstdint>
#include <set>
#include <stdexcept>
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "dvm_device.h"
#include "dvmslam_host.h"

namespace ORB_SLAM3 {

// what LoopClosing.cc:708-747 leaves for one candidate (the names are the reference's)
struct BoWCovisibleMatches {
  std::vector<std::vector<MapPoint*>> vvpMatchedMPs;   // [vpCovKFi.size()][N]; the row of a null / bad keyframe stays empty (:723-724)
  std::vector<std::vector<int>> vvnMatchIdx2;          // the same shape: the matched keypoint of vpCovKFi[j] (-1: none)
  std::vector<int> vnMatches;                          // SearchByBoW's return value per keyframe (0 for a skipped one)
  int nMostBoWNumMatches = 0, nIndexMostBoWMatchesKF = 0;   // (:727-730, strict >)
  std::vector<MapPoint*> vpMatchedPoints;              // [N] first-seen-wins over spMatchedMPi (:733-747)
  std::vector<KeyFrame*> vpKeyFrameMatchedMP;          // [N]
  int numBoWMatches = 0;
};

inline std::vector<BoWCovisibleMatches> SearchByBoWCovisibles(KeyFrame* pCurrentKF, const std::vector<std::vector<KeyFrame*>>& vvpCovKFs,
                                                              float nnratio, bool bCheckOri) {
  static_assert(sizeof(cv::KeyPoint) == sizeof(dvm_keypoint), "cv::KeyPoint is passed as dvm_keypoint");
  // the members of a KeyFrame the search reads, as the view the matcher functions take
  struct Pack {
    std::vector<MapPoint*> mps;
    std::vector<int32_t> mp, node, off, feat;
    std::vector<uint8_t> bad;
    dvmh_keyframe_view v;
    explicit Pack(KeyFrame* kf) : mps(kf->GetMapPointMatches()) {
      if (kf->NLeft != -1) throw std::runtime_error("SearchByBoWCovisibles: stereo / fisheye pairs (NLeft != -1) are outside the accelerated path");
      mp.resize(mps.size()); bad.resize(mps.size());
      for (size_t i = 0; i < mps.size(); i++) {
        mp[i] = mps[i] ? (int32_t)i : -1;                                 // the id of a point is its keypoint: unique inside the keyframe
        bad[i] = mps[i] && mps[i]->isBad() ? 1 : 0;
      }
      off.push_back(0);
      for (const auto& kv : kf->mFeatVec) {
        node.push_back((int32_t)kv.first);
        for (unsigned f : kv.second) feat.push_back((int32_t)f);
        off.push_back((int32_t)feat.size());
      }
      v = dvmh_keyframe_view();
      v.N = kf->N; v.mvKeysUn = reinterpret_cast<const dvm_keypoint*>(kf->mvKeysUn.data()); v.mDescriptors = kf->mDescriptors.data;
      v.mvpMapPoints = mp.data(); v.mpBad = bad.data();
      v.mFeatVec.n = (int32_t)node.size(); v.mFeatVec.node = node.data(); v.mFeatVec.off = off.data(); v.mFeatVec.feat = feat.data();
    }
  };
  const Pack cur(pCurrentKF);
  const size_t N = cur.mps.size();
  std::vector<Pack> packs;
  size_t total = 0;
  for (const auto& cov : vvpCovKFs) total += cov.size();
  packs.reserve(total);                                                   // (the views point into the packs: they must not move)
  std::vector<dvmh_keyframe_view> views;
  std::vector<std::vector<int>> sent(vvpCovKFs.size());                   // the target index of vpCovKFi[j]; -1: null or bad, not sent (:723-724)
  for (size_t c = 0; c < vvpCovKFs.size(); c++)
    for (KeyFrame* kf : vvpCovKFs[c]) {
      const bool skip = !kf || kf->isBad();
      sent[c].push_back(skip ? -1 : (int)views.size());
      if (skip) continue;
      packs.emplace_back(kf);
      views.push_back(packs.back().v);
    }
  const int T = (int)views.size();
  std::vector<int32_t> ids(N * (size_t)T + 1), idx2(N * (size_t)T + 1), nm((size_t)T + 1);
  if (T > 0 && dvmh_search_by_bow_targets(dvm_host::device(), &cur.v, T, views.data(), nnratio, bCheckOri ? 1 : 0, ids.data(), idx2.data(), nm.data()) < 0)
    throw std::runtime_error(dvm_last_error());

  std::vector<BoWCovisibleMatches> out(vvpCovKFs.size());
  for (size_t c = 0; c < vvpCovKFs.size(); c++) {
    const std::vector<KeyFrame*>& vpCovKFi = vvpCovKFs[c];
    BoWCovisibleMatches& B = out[c];
    B.vvpMatchedMPs.resize(vpCovKFi.size()); B.vvnMatchIdx2.resize(vpCovKFi.size()); B.vnMatches.assign(vpCovKFi.size(), 0);
    B.vpMatchedPoints.assign(N, static_cast<MapPoint*>(NULL)); B.vpKeyFrameMatchedMP.assign(N, static_cast<KeyFrame*>(NULL));
    for (size_t j = 0; j < vpCovKFi.size(); j++) {                        // (:722-731)
      if (sent[c][j] < 0) continue;
      const size_t t = (size_t)sent[c][j];
      const Pack& P = packs[t];
      B.vvpMatchedMPs[j].assign(N, static_cast<MapPoint*>(NULL)); B.vvnMatchIdx2[j].assign(N, -1);
      for (size_t i = 0; i < N; i++) {
        const int32_t k = idx2[t * N + i];
        if (k >= 0) { B.vvpMatchedMPs[j][i] = P.mps[k]; B.vvnMatchIdx2[j][i] = k; }
      }
      const int num = B.vnMatches[j] = nm[t];
      if (num > B.nMostBoWNumMatches) { B.nMostBoWNumMatches = num; B.nIndexMostBoWMatchesKF = (int)j; }
    }
    std::set<MapPoint*> spMatchedMPi;
    for (size_t j = 0; j < vpCovKFi.size(); j++)                          // (:733-747)
      for (size_t k = 0; k < B.vvpMatchedMPs[j].size(); k++) {
        MapPoint* pMPi_j = B.vvpMatchedMPs[j][k];
        if (!pMPi_j || pMPi_j->isBad()) continue;
        if (spMatchedMPi.insert(pMPi_j).second) {
          B.numBoWMatches++;
          B.vpMatchedPoints[k] = pMPi_j;
          B.vpKeyFrameMatchedMP[k] = vpCovKFi[j];
        }
      }
  }
  return out;
}

}  // namespace ORB_SLAM3
