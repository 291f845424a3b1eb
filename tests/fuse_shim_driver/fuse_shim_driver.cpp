// tests/fuse_shim_driver/fuse_shim_driver.cpp -- TEST INFRASTRUCTURE: runs both Fuse directions of LocalMapping::SearchInNeighbors
// (src/LocalMapping.cc:812-849) on a mock world twice over -- swf_chain through SearchInNeighborsChain (host/LocalMapping_shim.h: one
// speculative device run per direction plus the refreshes of stale rows), swf_loop as the plain loop: one dvmh_fuse call per target with
// the descriptors the points carry at that moment, the rows applied as ORBmatcher::Fuse applies them.  The mock MapPoint::Replace does
// not recompute descriptors, so both take the same stand-in for it (`seam` != 0): the survivor of a Replace takes the replaced point's
// descriptor.  tests/test_gpu_fuse_targets_shim.py builds two identical worlds, runs one function on each and compares the maps.
#include "../shim_driver/shim_driver.cpp"

#include <set>
#include <unordered_set>

namespace {
void take_descriptor(MapPoint* survivor, MapPoint* replaced) {
  const cv::Mat d = replaced->GetDescriptor();
  std::memcpy(MapPoint::MockAccess::descriptor(survivor).data, d.ptr<uint8_t>(), 32);
}
dvm_se3f se3_pod(const Sophus::SE3f& T) {
  dvm_se3f o;
  for (int i = 0; i < 4; i++) o.q[i] = T.unit_quaternion().coeffs()(i);
  for (int i = 0; i < 3; i++) o.t[i] = T.translation()(i);
  return o;
}
// ORBmatcher::Fuse(pKF, vpPoints, 3.0) (ORBmatcher.cc:1060-1234): dvmh_fuse on the state of this moment, then the apply loop
int fuse_one(KeyFrame* pKF, const std::vector<MapPoint*>& vpPoints, bool seam) {
  const size_t n = vpPoints.size();
  if (n == 0) return 0;
  dvmh_keyframe_view K = dvmh_keyframe_view();
  K.N = pKF->N; K.mvKeysUn = reinterpret_cast<const dvm_keypoint*>(pKF->mvKeysUn.data()); K.mDescriptors = pKF->mDescriptors.data;
  K.Tcw = se3_pod(pKF->GetPose()); K.Twc = se3_pod(pKF->GetPoseInverse());
  K.fx = pKF->fx; K.fy = pKF->fy; K.cx = pKF->cx; K.cy = pKF->cy;
  K.mnMinX = (float)pKF->mnMinX; K.mnMaxX = (float)pKF->mnMaxX; K.mnMinY = (float)pKF->mnMinY; K.mnMaxY = (float)pKF->mnMaxY;
  K.mvScaleFactors = pKF->mvScaleFactors.data(); K.mvLevelSigma2 = pKF->mvLevelSigma2.data(); K.mvInvLevelSigma2 = pKF->mvInvLevelSigma2.data();
  K.mfLogScaleFactor = pKF->mfLogScaleFactor; K.nLevels = pKF->mnScaleLevels;
  std::vector<int32_t> id(n, -1), best(n, -1);
  std::vector<uint8_t> bad(n, 1), desc(32 * n, 0), inKF(n, 0);
  std::vector<float> pos(3 * n, 0.f), normal(3 * n, 0.f), mind(n, 1.f), maxd(n, 1.f);
  for (size_t i = 0; i < n; i++) {
    MapPoint* p = vpPoints[i];
    if (!p) continue;
    id[i] = (int32_t)i; bad[i] = p->isBad();
    const Eigen::Vector3f X = p->GetWorldPos(), Nn = p->GetNormal();
    for (int c = 0; c < 3; c++) { pos[3 * i + c] = X(c); normal[3 * i + c] = Nn(c); }
    mind[i] = p->GetMinDistance(); maxd[i] = p->GetMaxDistance();
    const cv::Mat d = p->GetDescriptor();
    std::memcpy(&desc[32 * i], d.ptr<uint8_t>(), 32);
    inKF[i] = !p->isBad() && p->IsInKeyFrame(pKF);
  }
  dvmh_map_points_view P;
  P.n = (int32_t)n; P.id = id.data(); P.bad = bad.data(); P.pos = pos.data(); P.normal = normal.data(); P.min_dist = mind.data(); P.max_dist = maxd.data();
  P.desc = desc.data();
  if (dvmh_fuse(dvm_host::device(), &K, &P, inKF.data(), 3.0f, best.data()) < 0) throw std::runtime_error(dvm_last_error());
  int nFused = 0;
  for (size_t i = 0; i < n; i++) {
    MapPoint* pMP = vpPoints[i];
    if (best[i] < 0 || !pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
    MapPoint* pMPinKF = pKF->GetMapPoint(best[i]);
    if (pMPinKF) {
      if (!pMPinKF->isBad()) {
        if (pMPinKF->Observations() > pMP->Observations()) { pMP->Replace(pMPinKF); if (seam) take_descriptor(pMPinKF, pMP); }
        else { pMPinKF->Replace(pMP); if (seam) take_descriptor(pMP, pMPinKF); }
      }
    } else {
      pMP->AddObservation(pKF, best[i]);
      pKF->AddMapPoint(pMP, best[i]);
    }
    nFused++;
  }
  return nFused;
}
}  // namespace

extern "C" {

// nFused: n_targets entries (first direction) + 1 (second direction); returns the number of blocking device calls
int swf_chain(World* w, int kf, const int32_t* targets, int n_targets, int seam, int32_t* nFused) {
  return guarded(w, [&] {
    const std::vector<KeyFrame*> tg = kf_list(w, targets, n_targets);
    bool abort = false;
    SearchInNeighborsCounts r;
    if (seam) r = SearchInNeighborsChain(w->kfs[kf].get(), tg, &abort, [](MapPoint* survivor, MapPoint* replaced) { take_descriptor(survivor, replaced); });
    else r = SearchInNeighborsChain(w->kfs[kf].get(), tg, &abort);
    for (int t = 0; t < n_targets; t++) nFused[t] = r.nFused[t];
    nFused[n_targets] = r.nFusedCurrent;
    return r.nDeviceCalls;
  });
}
int swf_loop(World* w, int kf, const int32_t* targets, int n_targets, int seam, int32_t* nFused) {
  return guarded(w, [&] {
    KeyFrame* keyFrame = w->kfs[kf].get();
    const std::vector<KeyFrame*> tg = kf_list(w, targets, n_targets);
    const std::vector<MapPoint*> vpMapPointMatches = keyFrame->GetMapPointMatches();
    int calls = 0;
    for (int t = 0; t < n_targets; t++) { nFused[t] = fuse_one(tg[t], vpMapPointMatches, seam != 0); calls++; }
    std::vector<MapPoint*> vpFuseCandidates;
    std::set<MapPoint*> taken;
    for (KeyFrame* pKFi : tg)
      for (MapPoint* pMP : pKFi->GetMapPointMatches()) {
        if (!pMP) continue;
        if (pMP->isBad() || !taken.insert(pMP).second) continue;      // (mnFuseCandidateForKF, which the mock MapPoint does not have)
        vpFuseCandidates.push_back(pMP);
      }
    nFused[n_targets] = fuse_one(keyFrame, vpFuseCandidates, seam != 0);
    return calls + 1;
  });
}

// the shim marks fuse candidates through MapPoint::mnFuseCandidateForKF where the class has it: that overload on a point class that does.
// out[k] = whether the k-th of (a, 7), (a, 7), (b, 7), (a, 8), (a, 8) was a first sighting; out[5], out[6] = the members afterwards
void swf_mark_candidate_with_member(int32_t* out) {
  struct Point { long unsigned int mnFuseCandidateForKF = ~0ul; } a, b;
  std::unordered_set<Point*> unused;
  Point* seq[5] = {&a, &a, &b, &a, &a};
  const long unsigned int ids[5] = {7, 7, 7, 8, 8};
  for (int k = 0; k < 5; k++) out[k] = dvm_fuse_detail::MarkFuseCandidate(seq[k], ids[k], unused, 0) ? 1 : 0;
  out[5] = (int32_t)a.mnFuseCandidateForKF; out[6] = (int32_t)b.mnFuseCandidateForKF; out[7] = (int32_t)unused.size();
}

}  // extern "C"
