// dvm_slam_amd/host/LocalMapping_shim.h -- the geometry of ORB_SLAM3::LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:446-745)
// on the HIP library.  CreateNewMapPoints stays the reference's function: neighbour selection, the baseline / median-depth test,
// ORBmatcher::SearchForTriangulation (host/ORBmatcher_shim.h) and the creation of the MapPoints are unchanged.  What moves to the
// device is the body of its per-match loop for one neighbour keyframe (:534-741, monocular pinhole branch): parallax of the two
// rays, GeometricTools::Triangulate, the depth / reprojection / distance / scale-consistency tests -- all matches of the
// neighbour in one launch (dvm_triangulate_matches).  The loop then reads
//
//   std::vector<Eigen::Vector3f> vX3D; std::vector<int> vStatus;
//   TriangulateMatches(mpCurrentKeyFrame, pKF2, vMatchedIndices, mbInertial, mbFarPoints, mThFarPoints, vX3D, vStatus);
//   for (int ikp = 0; ikp < nmatches; ikp++) {
//     if (vStatus[ikp] != 0) continue;                       // one of the reference's `continue`s (status = which one)
//     MapPoint* pMP = new MapPoint(vX3D[ikp], mpCurrentKeyFrame, mpAtlas->GetCurrentMap(), mpAtlas->GetAgentId());
//     ... AddObservation x2, AddMapPoint x2, ComputeDistinctiveDescriptors, UpdateNormalAndDepth, mpAtlas->AddMapPoint: as before
//   }
//
// CreateNewMapPointsChain goes one step further: the WHOLE loop over the neighbours -- baseline test, SearchForTriangulation against the
// table the earlier neighbours left, the geometry, the table update -- is one device chain (dvm_create_new_map_points: one upload, three
// launches, one synchronisation instead of two blocking calls per neighbour).  The loop of LocalMapping.cc:489-745 then reads
//
//   std::vector<float> vMedianDepth;                         // the map points live on the host
//   for (KeyFrame* pKF2 : vpNeighKFs) vMedianDepth.push_back(pKF2->ComputeSceneMedianDepth(2));
//   const NewPointRecords rec = CreateNewMapPointsChain(mpCurrentKeyFrame, vpNeighKFs, vMedianDepth, mbInertial, bCoarse, mbFarPoints, mThFarPoints);
//   for (size_t i = 0; i < vpNeighKFs.size(); i++) {
//     if (i > 0 && CheckNewKeyFrames()) return;              // records of neighbour i do not depend on later neighbours: the rest is dropped
//     KeyFrame* pKF2 = vpNeighKFs[i];
//     for (int m = rec.pair_off[i]; m < rec.pair_off[i + 1]; m++) {
//       if (rec.status[m] != 0) continue;
//       const int idx1 = rec.pairs[m].first, idx2 = rec.pairs[m].second;
//       MapPoint* pMP = new MapPoint(rec.x3D[m], mpCurrentKeyFrame, mpAtlas->GetCurrentMap(), mpAtlas->GetAgentId());
//       ... AddObservation x2, AddMapPoint x2 (a second record naming idx2 overwrites, as in the reference), ComputeDistinctiveDescriptors,
//           UpdateNormalAndDepth, mpAtlas->AddMapPoint, mlpRecentAddedMapPoints.push_back: as before
//     }
//   }
//
// (bCoarse is computed once in front of the loop; the matcher of :467 is ORBmatcher(0.6f, false), so the rotation check is off.)
//
// Not covered: the stereo / two-camera-rig branches (bStereo1 / bStereo2, mpCamera2) -- DVM-SLAM's agents are monocular.
// Parity: float arithmetic in Eigen's evaluation order; the homogeneous point comes from a double Jacobi diagonalisation of
// A^T A where the reference runs Eigen::JacobiSVD<Matrix4f> -- the same vector up to float SVD error (tolerance parity, as for
// Sim3Solver's eigen-decomposition; decisions equal away from the thresholds).
#pragma once
#include <stdexcept>
#include <utility>
#include <vector>

#include "KeyFrame.h"
#include "dvm_device.h"
#include "dvmslam_host.h"

namespace ORB_SLAM3 {

inline void TriangulateMatches(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<std::pair<size_t, size_t>>& vMatchedIndices, bool bInertial,
                               bool bFarPoints, float thFarPoints, std::vector<Eigen::Vector3f>& vX3D, std::vector<int>& vStatus) {
  static_assert(sizeof(cv::KeyPoint) == sizeof(dvm_keypoint), "cv::KeyPoint is passed as dvm_keypoint");
  const int n = (int)vMatchedIndices.size();
  vX3D.assign(n, Eigen::Vector3f());
  vStatus.assign(n, 0);
  if (n == 0) return;
  dvm_tri_pair P;
  P.cos_parallax_max = bInertial ? 0.9996 : 0.9998;                     // (:655-656)
  auto fill = [](KeyFrame* kf, float* K, float* T, float* Ow) {
    for (int i = 0; i < 4; i++) K[i] = kf->mpCamera->getParameter(i);
    const Sophus::SE3f Tcw = kf->GetPose();                            // eigTcw = sophTcw.matrix3x4() (:470, :519)
    const Eigen::Matrix3f R = Tcw.rotationMatrix();
    const Eigen::Vector3f t = Tcw.translation(), O = kf->GetCameraCenter();
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) T[4 * r + c] = R(r, c);
      T[4 * r + 3] = t(r);
      Ow[r] = O(r);
    }
  };
  fill(pKF1, P.K1, P.T1w, P.Ow1);
  fill(pKF2, P.K2, P.T2w, P.Ow2);
  P.ratio_factor = 1.5f * pKF1->mfScaleFactor;                          // (:483)
  P.th_far = thFarPoints;
  P.far_points = bFarPoints ? 1 : 0;
  P.n_levels = (int)pKF1->mvLevelSigma2.size();
  if (pKF2->mvLevelSigma2.size() != pKF1->mvLevelSigma2.size() || pKF1->mvScaleFactors.size() != pKF1->mvLevelSigma2.size() ||
      pKF2->mvScaleFactors.size() != pKF1->mvLevelSigma2.size())
    throw std::invalid_argument("TriangulateMatches: the two keyframes' pyramid tables differ in length");
  std::vector<int32_t> pairs(2 * (size_t)n);
  for (int i = 0; i < n; i++) { pairs[2 * i] = (int32_t)vMatchedIndices[i].first; pairs[2 * i + 1] = (int32_t)vMatchedIndices[i].second; }
  std::vector<float> X(3 * (size_t)n);
  std::vector<int32_t> st(n);
  dvm_host::use_device();
  if (dvm_triangulate_matches(&P, reinterpret_cast<const dvm_keypoint*>(pKF1->mvKeysUn.data()), (int)pKF1->mvKeysUn.size(),
                              reinterpret_cast<const dvm_keypoint*>(pKF2->mvKeysUn.data()), (int)pKF2->mvKeysUn.size(), pairs.data(), n,
                              pKF1->mvLevelSigma2.data(), pKF2->mvLevelSigma2.data(), pKF1->mvScaleFactors.data(), pKF2->mvScaleFactors.data(),
                              X.data(), st.data(), 0, nullptr) != DVM_OK)
    throw std::runtime_error(dvm_last_error());
  for (int i = 0; i < n; i++) {
    for (int k = 0; k < 3; k++) vX3D[i](k) = X[3 * i + k];
    vStatus[i] = st[i];
  }
}

// what dvm_create_new_map_points hands back (include/dvmslam_hip.h): per neighbour its status (0 ran, 1 skipped by the baseline test),
// SearchForTriangulation's return value and its range of records; the records in vMatchedIndices order; per KF1 keypoint the record that
// gave it its point (-1: none)
struct NewPointRecords {
  std::vector<int> nb_status, nb_matches, pair_off;
  std::vector<std::pair<size_t, size_t>> pairs;
  std::vector<int> status;
  std::vector<Eigen::Vector3f> x3D;
  std::vector<int> new_point;
};

inline NewPointRecords CreateNewMapPointsChain(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpNeighKFs, const std::vector<float>& vMedianDepth,
                                               bool bInertial, bool bCoarse, bool bFarPoints, float thFarPoints, bool bCheckOrientation = false) {
  static_assert(sizeof(cv::KeyPoint) == sizeof(dvm_keypoint), "cv::KeyPoint is passed as dvm_keypoint");
  if (vMedianDepth.size() != vpNeighKFs.size()) throw std::invalid_argument("CreateNewMapPointsChain: one median depth per neighbour");
  // the members of a KeyFrame the chain reads, as the view the matcher functions take
  struct Pack {
    std::vector<int32_t> mp, node, off, feat;
    dvmh_keyframe_view v;
    explicit Pack(KeyFrame* kf) {
      const std::vector<MapPoint*> mps = kf->GetMapPointMatches();
      mp.resize(mps.size());
      for (size_t i = 0; i < mps.size(); i++) mp[i] = mps[i] ? 0 : -1;       // the chain only asks whether there is a point
      off.push_back(0);
      for (const auto& kv : kf->mFeatVec) {
        node.push_back((int32_t)kv.first);
        for (unsigned f : kv.second) feat.push_back((int32_t)f);
        off.push_back((int32_t)feat.size());
      }
      v = dvmh_keyframe_view();
      v.N = kf->N; v.mvKeysUn = reinterpret_cast<const dvm_keypoint*>(kf->mvKeysUn.data()); v.mDescriptors = kf->mDescriptors.data;
      v.mvpMapPoints = mp.data(); v.mpBad = nullptr;
      v.mFeatVec.n = (int32_t)node.size(); v.mFeatVec.node = node.data(); v.mFeatVec.off = off.data(); v.mFeatVec.feat = feat.data();
      const Sophus::SE3f Tcw = kf->GetPose(), Twc = kf->GetPoseInverse();
      for (int i = 0; i < 4; i++) { v.Tcw.q[i] = Tcw.unit_quaternion().coeffs()(i); v.Twc.q[i] = Twc.unit_quaternion().coeffs()(i); }
      for (int i = 0; i < 3; i++) { v.Tcw.t[i] = Tcw.translation()(i); v.Twc.t[i] = Twc.translation()(i); }
      v.fx = kf->fx; v.fy = kf->fy; v.cx = kf->cx; v.cy = kf->cy;
      v.mnMinX = (float)kf->mnMinX; v.mnMaxX = (float)kf->mnMaxX; v.mnMinY = (float)kf->mnMinY; v.mnMaxY = (float)kf->mnMaxY;
      v.mvScaleFactors = kf->mvScaleFactors.data(); v.mvLevelSigma2 = kf->mvLevelSigma2.data(); v.mvInvLevelSigma2 = kf->mvInvLevelSigma2.data();
      v.mfLogScaleFactor = kf->mfLogScaleFactor; v.nLevels = (int32_t)kf->mvLevelSigma2.size();
    }
  };
  Pack K1(pKF1);
  std::vector<Pack> packs;
  packs.reserve(vpNeighKFs.size());
  std::vector<dvmh_keyframe_view> views;
  for (KeyFrame* kf : vpNeighKFs) {
    if (kf->mvScaleFactors.size() != kf->mvLevelSigma2.size() || pKF1->mvScaleFactors.size() != pKF1->mvLevelSigma2.size())
      throw std::invalid_argument("CreateNewMapPointsChain: a keyframe's pyramid tables differ in length");
    packs.emplace_back(kf);
    views.push_back(packs.back().v);
  }
  const int nn = (int)vpNeighKFs.size();
  dvm_np_params P;
  P.cos_parallax_max = bInertial ? 0.9996 : 0.9998;                     // (:655-656)
  P.ratio_factor = 1.5f * pKF1->mfScaleFactor;                          // (:483)
  P.th_far = thFarPoints; P.far_points = bFarPoints ? 1 : 0;
  P.coarse = bCoarse ? 1 : 0; P.check_ori = bCheckOrientation ? 1 : 0; P.monocular = 1;
  size_t free1 = 0;
  for (int32_t m : K1.mp) free1 += m < 0 ? 1 : 0;
  const size_t cap = free1 * (size_t)nn;                                 // a neighbour yields at most one record per keypoint without a point
  NewPointRecords R;
  R.nb_status.assign(nn + 1, 0); R.nb_matches.assign(nn + 1, 0); R.pair_off.assign(nn + 1, 0);
  R.status.assign(cap + 1, 0); R.new_point.assign(K1.mp.size() + 1, -1);
  std::vector<int32_t> pairs(2 * cap + 2);
  std::vector<float> X(3 * cap + 3);
  dvm_np_out O;
  O.nb_status = R.nb_status.data(); O.nb_matches = R.nb_matches.data(); O.pair_off = R.pair_off.data();
  O.pairs = pairs.data(); O.status = R.status.data(); O.x3D = X.data(); O.new_point = R.new_point.data(); O.record_cap = (int32_t)cap;
  static_assert(sizeof(int) == sizeof(int32_t), "int32_t results are written into vector<int>");
  if (dvmh_create_new_map_points(dvm_host::device(), &K1.v, nn, views.data(), vMedianDepth.data(), &P, &O) != DVM_OK)
    throw std::runtime_error(dvm_last_error());
  const size_t n = (size_t)R.pair_off[nn];
  R.nb_status.resize(nn); R.nb_matches.resize(nn); R.status.resize(n); R.new_point.resize(K1.mp.size());
  R.pairs.resize(n); R.x3D.resize(n);
  for (size_t m = 0; m < n; m++) {
    R.pairs[m] = std::make_pair((size_t)pairs[2 * m], (size_t)pairs[2 * m + 1]);
    for (int k = 0; k < 3; k++) R.x3D[m](k) = X[3 * m + k];
  }
  return R;
}

}  // namespace ORB_SLAM3
