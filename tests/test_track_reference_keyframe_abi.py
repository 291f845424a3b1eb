"""The reference-keyframe chain's C ABI (include/dvmslam_hip.h: dvm_ref_keyframe, dvm_track_refkf_params, dvm_track_refkf_out,
dvm_track_refkf_result, dvm_track_reference_keyframe) without a GPU: the call pattern INTEGRATION.md gives for Tracking::TrackReferenceKeyFrame
compiles against the header (over minimal stand-ins of the reference's classes), and the layouts the header defines are the ones the Python side
(capi.RefKeyframe, capi.TrackRefKfParams, capi.TrackRefKfOut, capi.TrackRefKfResult) reads and writes."""
import ctypes as C
import os
import re
import subprocess

from dvm_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# just enough of ORB_SLAM3 / DBoW2 / Eigen / Sophus / OpenCV for the snippet to type-check (declarations only: -fsyntax-only)
PRELUDE = r"""
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>
#include "dvmslam_hip.h"
namespace Eigen {
struct Vector3f { Vector3f(float, float, float); float operator()(int) const; };
struct Quaternionf { Quaternionf(float w, float x, float y, float z); float x() const; float y() const; float z() const; float w() const; };
}
namespace Sophus {
struct SE3f { SE3f(const Eigen::Quaternionf&, const Eigen::Vector3f&); Eigen::Quaternionf unit_quaternion() const; Eigen::Vector3f translation() const; };
}
namespace cv {
struct KeyPoint { float angle; };
struct Mat { int rows, cols; size_t step; template <class T> const T* ptr(int row) const; };
}
namespace DBoW2 { typedef std::map<unsigned, double> BowVector; typedef std::map<unsigned, std::vector<unsigned>> FeatureVector; }
struct MapPoint {
  Eigen::Vector3f GetWorldPos(); int Observations(); bool isBad();
  bool mbTrackInView; unsigned long mnLastFrameSeen;
};
struct KeyFrame {
  int N; std::vector<cv::KeyPoint> mvKeysUn; cv::Mat mDescriptors; DBoW2::FeatureVector mFeatVec;
  std::vector<MapPoint*> GetMapPointMatches();
};
struct Frame {
  int N; unsigned long mnId; std::vector<MapPoint*> mvpMapPoints; std::vector<bool> mvbOutlier;
  DBoW2::BowVector mBowVec; DBoW2::FeatureVector mFeatVec;
  void SetPose(const Sophus::SE3f&); Sophus::SE3f GetPose() const;
};
// the sections before it in INTEGRATION.md
bool TrackWithMotionModelOnDevice(dvm_tracker* trk, dvm_orb* extractor, const cv::Mat& im, Frame& mCurrentFrame, const Frame& mLastFrame);
int TrackLocalMapOnDevice(dvm_tracker* trk, dvm_orb* extractor, Frame& mCurrentFrame, const std::vector<MapPoint*>& mvpLocalMapPoints, float th,
                          bool bFarPoints, float thFarPoints, int& mnMatchesInliers);
"""

HEADER_NAMES = {"RefKeyframe": "dvm_ref_keyframe", "TrackRefKfParams": "dvm_track_refkf_params", "TrackRefKfOut": "dvm_track_refkf_out",
                "TrackRefKfResult": "dvm_track_refkf_result"}


def _snippet():
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = txt[txt.index("## `Tracking::TrackReferenceKeyFrame` on the device"):]
    m = re.search(r"```cpp\n(.*?)```", sec, re.S)
    assert m, "INTEGRATION.md: the reference-keyframe call pattern is missing"
    return m.group(1)


def _layout_asserts():
    out = []
    for py, c in HEADER_NAMES.items():
        S = getattr(capi, py)
        out.append(f"static_assert(sizeof({c}) == {C.sizeof(S)}, \"{c} size\");")
        for name, _ in S._fields_:
            out.append(f"static_assert(offsetof({c}, {name}) == {getattr(S, name).offset}, \"{c}.{name}\");")
    out.append(f"static_assert(sizeof(dvm_keypoint) == {capi.KP_DTYPE.itemsize}, \"dvm_keypoint size\");")
    out.append("static_assert(DVM_TRACK_COMPLETE == 0 && DVM_TRACK_FEW_MATCHES == 1 && DVM_TRACK_REPLAY_ON_HOST == 2 && DVM_TRACK_FEW_MAP_MATCHES == 3, "
               "\"statuses\");")
    return "\n".join(out)


def test_layouts_are_pinned():
    assert C.sizeof(capi.RefKeyframe) == 88 and C.sizeof(capi.TrackRefKfParams) == 160
    assert C.sizeof(capi.TrackRefKfOut) == 96 and C.sizeof(capi.TrackRefKfResult) == 136
    assert [f for f, _ in capi.TrackRefKfResult._fields_][:11] == ["n", "mono_index", "status", "nmatches", "nmatches_before_rotation", "n_edges",
                                                                 "n_inliers", "nmatches_after", "nmatches_map", "n_bow", "n_fv"]
    assert capi.TrackRefKfResult.pose.offset == 48 and capi.TrackRefKfResult.Tcw.offset == 104
    assert (capi.DVM_TRACK_COMPLETE, capi.DVM_TRACK_FEW_MATCHES, capi.DVM_TRACK_FEW_MAP_MATCHES) == (0, 1, 3)


def test_header_declares_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "dvmslam_hip.h")).read()
    assert re.search(r"int dvm_tracker_reserve_reference_keyframe\(dvm_tracker\* t, int max_kf_keypoints\);", txt)
    assert re.search(r"int dvm_track_reference_keyframe\(dvm_tracker\* t, dvm_orb\* h, const dvm_vocab\* voc, const dvm_ref_keyframe\* kf,\s*"
                     r"const dvm_track_refkf_params\* p,\s*dvm_track_refkf_out\* out, dvm_track_refkf_result\* res\);", txt)


def test_integration_call_pattern_compiles_against_the_header(tmp_path):
    src = tmp_path / "track_reference_keyframe_pattern.cpp"
    src.write_text(PRELUDE + "\n" + _layout_asserts() + "\n" + _snippet())
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
