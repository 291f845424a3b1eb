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
// SearchInNeighborsChain does the same for LocalMapping::SearchInNeighbors (src/LocalMapping.cc:757-865): both Fuse directions (:812-849)
// on dvm_fuse_targets -- all target keyframes uploaded once, their grids built in one launch, all (target, point) searches in one launch,
// one synchronisation per direction -- where the reference's loop makes one blocking Fuse call per target.  The function then reads
//
//   ... the target selection of :759-810, unchanged, fills vpTargetKFs ...
//   const SearchInNeighborsCounts fused = SearchInNeighborsChain(keyFrame, vpTargetKFs, &mbAbortBA);
//   if (fused.aborted) return;                               // mbAbortBA was set between the two directions (:823)
//   vpMapPointMatches = keyFrame->GetMapPointMatches();      // the point update of :851-861 and UpdateConnections (:864): as before
//
// The searches are speculative: they read the descriptors as they are at entry, and the rows are replayed target by target exactly as
// ORBmatcher::Fuse applies them (isBad() / IsInKeyFrame() tested again at each row).  MapPoint::Replace ends in
// ComputeDistinctiveDescriptors, so the survivor of a Replace may carry a new descriptor for the later targets: its descriptor is compared
// with the bytes that were uploaded, and before a row of such a point is applied ONE further run refreshes the rows of all points stale at
// that moment against the targets not yet finished.  No row of a stale point is applied unrefreshed.
//
// Not covered: the stereo / two-camera-rig branches (bStereo1 / bStereo2, mpCamera2) -- DVM-SLAM's agents are monocular.
// Parity: float arithmetic in Eigen's evaluation order; the homogeneous point comes from a double Jacobi diagonalisation of
// A^T A where the reference runs Eigen::JacobiSVD<Matrix4f> -- the same vector up to float SVD error (tolerance parity, as for
// Sim3Solver's eigen-decomposition; decisions equal away from the thresholds).
#pragma once
#include <cstring>
#include <stdexcept>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "KeyFrame.h"
#include "chain_handle.h"
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

// ---- LocalMapping::SearchInNeighbors (:812-849) on dvm_fuse_targets
namespace dvm_fuse_detail {
// the calling thread's chain handle (chain_handle.h), cap: {points, targets, their keypoints}; growth with headroom on the points and on
// the keypoints
using Handle = dvm_host::ChainHandle<dvm_fuse_targets, dvm_fuse_targets_create, dvm_fuse_targets_destroy, dvm_fuse_targets_reserve>;
inline Handle& handle(int dev, int n_points, int n_targets, long total_keypoints) {
  thread_local Handle H;
  if (H.open(dev) != DVM_OK) throw std::runtime_error(dvm_last_error());
  if (!H.holds(n_points, n_targets, total_keypoints)) {
    const int p = std::max(H.cap[0], n_points + n_points / 4), t = std::max(H.cap[1], n_targets);
    const int tot = (int)std::min<long>(std::max<long>(H.cap[2], total_keypoints + total_keypoints / 4), (long)t * 8192);
    if (H.reserve(p, t, tot) != DVM_OK) throw std::runtime_error(dvm_last_error());
  }
  return H;
}
inline void read_descriptor(MapPoint* p, uint8_t* dst) {
  const cv::Mat d = p->GetDescriptor();
  std::memcpy(dst, d.ptr<uint8_t>(), 32);
}
// LocalMapping.cc:840-842: a point is a fuse candidate once per keyframe, `pMP->mnFuseCandidateForKF == keyFrame->mnId` says it has been
// taken.  The first overload is the reference's test and mark; it is chosen wherever the point class has the member.  A point class
// without it (a reduced MapPoint) gets the same answer from a set that lives for the call.  Returns true the first time a point is seen.
template <class MP>
inline auto MarkFuseCandidate(MP* pMP, long unsigned int kfId, std::unordered_set<MP*>&, int) -> decltype(pMP->mnFuseCandidateForKF == kfId) {
  if (pMP->mnFuseCandidateForKF == kfId) return false;
  pMP->mnFuseCandidateForKF = kfId;
  return true;
}
template <class MP>
inline bool MarkFuseCandidate(MP* pMP, long unsigned int, std::unordered_set<MP*>& seen, long) {
  return seen.insert(pMP).second;
}
struct NoSeam {
  void operator()(MapPoint*, MapPoint*) const {}
};

// ORBmatcher::Fuse(pKF, vpPoints, th) for every pKF of vpKFs in order (ORBmatcher.cc:1060-1234): nFused[t] = its return value
template <class AfterReplace>
inline void FusePass(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpPoints, float th, AfterReplace& afterReplace,
                     std::vector<int>& nFused, int& nDeviceCalls) {
  static_assert(sizeof(cv::KeyPoint) == sizeof(dvm_keypoint), "cv::KeyPoint is passed as dvm_keypoint");
  const size_t T = vpKFs.size(), n = vpPoints.size();
  nFused.assign(T, 0);
  if (T == 0 || n == 0) return;
  std::vector<dvm_ft_target> targets(T);
  long total = 0;
  for (size_t t = 0; t < T; t++) {
    KeyFrame* kf = vpKFs[t];
    if (kf->NLeft != -1) throw std::runtime_error("SearchInNeighborsChain: stereo / fisheye pairs (NLeft != -1) are outside the accelerated path");
    if (kf->mvScaleFactors.size() != kf->mvInvLevelSigma2.size()) throw std::invalid_argument("SearchInNeighborsChain: a keyframe's pyramid tables differ in length");
    dvm_ft_target& k = targets[t];
    std::memset(&k, 0, sizeof(k));
    k.n = kf->N; k.kps = reinterpret_cast<const dvm_keypoint*>(kf->mvKeysUn.data()); k.desc = kf->mDescriptors.data;
    const Sophus::SE3f Tcw = kf->GetPose();
    const Eigen::Vector3f Ow = kf->GetCameraCenter();
    for (int i = 0; i < 4; i++) k.Tcw.q[i] = Tcw.unit_quaternion().coeffs()(i);
    for (int i = 0; i < 3; i++) { k.Tcw.t[i] = Tcw.translation()(i); k.Ow[i] = Ow(i); }
    k.fx = kf->fx; k.fy = kf->fy; k.cx = kf->cx; k.cy = kf->cy;
    k.min_x = (float)kf->mnMinX; k.max_x = (float)kf->mnMaxX; k.min_y = (float)kf->mnMinY; k.max_y = (float)kf->mnMaxY;
    k.scale_factors = kf->mvScaleFactors.data(); k.inv_level_sigma2 = kf->mvInvLevelSigma2.data();
    k.log_scale_factor = kf->mfLogScaleFactor; k.n_levels = (int32_t)kf->mvScaleFactors.size();
    total += kf->N;
  }
  // the point table as it is at entry: position, normal and distance range do not move inside the loop; the descriptor may
  std::vector<float> pos(3 * n, 0.f), normal(3 * n, 0.f), mind(n, 1.f), maxd(n, 1.f);
  std::vector<uint8_t> desc(32 * n, 0), valid(n, 0), skip(T * n, 0);
  std::unordered_map<MapPoint*, std::vector<size_t>> where;             // a point may sit at two keypoints
  for (size_t i = 0; i < n; i++) {
    MapPoint* p = vpPoints[i];
    if (!p || p->isBad()) continue;
    valid[i] = 1;
    const Eigen::Vector3f X = p->GetWorldPos(), Nn = p->GetNormal();
    for (int c = 0; c < 3; c++) { pos[3 * i + c] = X(c); normal[3 * i + c] = Nn(c); }
    mind[i] = p->GetMinDistance(); maxd[i] = p->GetMaxDistance();
    read_descriptor(p, &desc[32 * i]);
    where[p].push_back(i);
    for (size_t t = 0; t < T; t++) skip[t * n + i] = p->IsInKeyFrame(vpKFs[t]) ? 1 : 0;
  }
  dvm_ft_points P;
  P.n = (int32_t)n; P.pos = pos.data(); P.normal = normal.data(); P.min_dist = mind.data(); P.max_dist = maxd.data(); P.desc = desc.data();
  P.valid = valid.data();
  dvm_host::use_device();
  Handle& H = handle(dvm_host::device(), (int)n, (int)T, total);
  if (dvm_fuse_targets_set(H.h, (int)T, targets.data()) != DVM_OK) throw std::runtime_error(dvm_last_error());
  std::vector<int32_t> best(T * n, -1), fresh;
  if (dvm_fuse_targets_run(H.h, &P, skip.data(), th, best.data(), nullptr) != DVM_OK) throw std::runtime_error(dvm_last_error());
  nDeviceCalls++;

  std::vector<uint8_t> stale(n, 0);
  size_t nStale = 0;
  // rows (t.., i) of every stale point, searched again with the descriptors the points carry now
  auto refresh = [&](size_t t0) {
    std::vector<uint8_t> mask(T * n, 1);
    for (size_t i = 0; i < n; i++) {
      if (!stale[i]) continue;
      MapPoint* p = vpPoints[i];
      read_descriptor(p, &desc[32 * i]);
      for (size_t t = t0; t < T; t++) mask[t * n + i] = (p->isBad() || p->IsInKeyFrame(vpKFs[t])) ? 1 : 0;
    }
    fresh.assign(T * n, -1);
    if (dvm_fuse_targets_run(H.h, &P, mask.data(), th, fresh.data(), nullptr) != DVM_OK) throw std::runtime_error(dvm_last_error());
    nDeviceCalls++;
    for (size_t i = 0; i < n; i++) {
      if (!stale[i]) continue;
      for (size_t t = t0; t < T; t++) best[t * n + i] = fresh[t * n + i];
      stale[i] = 0;
    }
    nStale = 0;
  };
  // the descriptor of a Replace's survivor against the bytes the device holds
  auto check_survivor = [&](MapPoint* s) {
    const auto it = where.find(s);
    if (it == where.end()) return;
    uint8_t now[32];
    read_descriptor(s, now);
    for (size_t i : it->second)
      if (!stale[i] && std::memcmp(now, &desc[32 * i], 32) != 0) { stale[i] = 1; nStale++; }
  };
  for (size_t t = 0; t < T; t++) {
    KeyFrame* pKF = vpKFs[t];
    for (size_t i = 0; i < n; i++) {
      MapPoint* pMP = vpPoints[i];
      if (!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;      // state may have changed through an earlier Replace
      if (nStale && stale[i]) refresh(t);
      const int32_t idx = best[t * n + i];
      if (idx < 0) continue;
      MapPoint* pMPinKF = pKF->GetMapPoint(idx);
      if (pMPinKF) {
        if (!pMPinKF->isBad()) {
          if (pMPinKF->Observations() > pMP->Observations()) { pMP->Replace(pMPinKF); afterReplace(pMPinKF, pMP); check_survivor(pMPinKF); }
          else { pMPinKF->Replace(pMP); afterReplace(pMP, pMPinKF); check_survivor(pMP); }
        }
      } else {
        pMP->AddObservation(pKF, idx);
        pKF->AddMapPoint(pMP, idx);
      }
      nFused[t]++;
    }
  }
}
}  // namespace dvm_fuse_detail

// what SearchInNeighborsChain hands back: ORBmatcher::Fuse's return value per target keyframe (first direction) and for the current
// keyframe (second direction), the blocking device calls made (two without a stale descriptor), and whether *pbAbort ended it in between
struct SearchInNeighborsCounts {
  std::vector<int> nFused;
  int nFusedCurrent = 0;
  int nDeviceCalls = 0;
  bool aborted = false;
};

// LocalMapping.cc:812-849.  afterReplace(survivor, replaced) is called after each MapPoint::Replace: a seam for tests whose mock Replace
// does not recompute descriptors; it does nothing in production (MapPoint::Replace itself ends in ComputeDistinctiveDescriptors).
template <class AfterReplace = dvm_fuse_detail::NoSeam>
inline SearchInNeighborsCounts SearchInNeighborsChain(KeyFrame* keyFrame, const std::vector<KeyFrame*>& vpTargetKFs, const bool* pbAbort,
                                                      AfterReplace afterReplace = AfterReplace(), const float th = 3.0f) {
  SearchInNeighborsCounts R;
  // Search matches by projection from current KF in target KFs
  const std::vector<MapPoint*> vpMapPointMatches = keyFrame->GetMapPointMatches();
  dvm_fuse_detail::FusePass(vpTargetKFs, vpMapPointMatches, th, afterReplace, R.nFused, R.nDeviceCalls);
  if (pbAbort && *pbAbort) { R.aborted = true; return R; }
  // Search matches by projection from target KFs in current KF
  std::vector<MapPoint*> vpFuseCandidates;
  vpFuseCandidates.reserve(vpTargetKFs.size() * vpMapPointMatches.size());
  std::unordered_set<MapPoint*> seen;                                  // (only read where MapPoint has no mnFuseCandidateForKF)
  for (KeyFrame* pKFi : vpTargetKFs) {
    for (MapPoint* pMP : pKFi->GetMapPointMatches()) {
      if (!pMP) continue;
      if (pMP->isBad() || !dvm_fuse_detail::MarkFuseCandidate(pMP, keyFrame->mnId, seen, 0)) continue;
      vpFuseCandidates.push_back(pMP);
    }
  }
  std::vector<int> nCur;
  dvm_fuse_detail::FusePass(std::vector<KeyFrame*>(1, keyFrame), vpFuseCandidates, th, afterReplace, nCur, R.nDeviceCalls);
  R.nFusedCurrent = nCur.empty() ? 0 : nCur[0];
  return R;
}

}  // namespace ORB_SLAM3
