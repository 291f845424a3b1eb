"""The second half's C ABI (include/dvmslam_hip.h: dvm_local_point, dvm_track_local_result, dvm_track_local_map) without a GPU: the call
pattern INTEGRATION.md gives for Tracking::TrackLocalMap compiles against the header (over minimal stand-ins of the reference's classes), and
the layouts the header defines are the ones the Python side (capi.LOCAL_POINT_DTYPE, capi.TrackLocalResult) reads and writes."""
import ctypes as C
import os
import re
import subprocess

from dvm_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# just enough of ORB_SLAM3 / Eigen / Sophus / OpenCV for the snippet to type-check (declarations only: -fsyntax-only)
PRELUDE = r"""
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>
#include "dvmslam_hip.h"
namespace Eigen {
struct Vector3f { Vector3f(float, float, float); float operator()(int) const; };
struct Quaternionf { Quaternionf(float w, float x, float y, float z); };
}
namespace Sophus { struct SE3f { SE3f(const Eigen::Quaternionf&, const Eigen::Vector3f&); }; }
namespace cv { struct Mat { template <class T> const T* ptr(int row) const; }; }
struct MapPoint {
  Eigen::Vector3f GetWorldPos(); Eigen::Vector3f GetNormal(); cv::Mat GetDescriptor(); int Observations(); bool isBad();
  void IncreaseVisible(int n = 1); void IncreaseFound(int n = 1);
  float mfMinDistance, mfMaxDistance, mTrackProjX, mTrackProjY; bool mbTrackInView; unsigned long mnLastFrameSeen;
};
struct Frame {
  int N; unsigned long mnId; std::vector<MapPoint*> mvpMapPoints; std::vector<bool> mvbOutlier;
  void SetPose(const Sophus::SE3f&);
};
"""


def _snippet():
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = txt[txt.index("## The second half"):]
    m = re.search(r"```cpp\n(.*?)```", sec, re.S)
    assert m, "INTEGRATION.md: the second half's call pattern is missing"
    return m.group(1)


def _layout_asserts():
    out = []
    lp = capi.LOCAL_POINT_DTYPE
    out.append(f"static_assert(sizeof(dvm_local_point) == {lp.itemsize}, \"dvm_local_point size\");")
    for name, (_, off) in lp.fields.items():
        out.append(f"static_assert(offsetof(dvm_local_point, {name}) == {off}, \"dvm_local_point.{name}\");")
    R = capi.TrackLocalResult
    out.append(f"static_assert(sizeof(dvm_track_local_result) == {C.sizeof(R)}, \"dvm_track_local_result size\");")
    for name, _ in R._fields_:
        out.append(f"static_assert(offsetof(dvm_track_local_result, {name}) == {getattr(R, name).offset}, \"dvm_track_local_result.{name}\");")
    out.append(f"static_assert(sizeof(dvm_track_point) == {capi.TRACK_DTYPE.itemsize}, \"dvm_track_point size\");")
    return "\n".join(out)


def test_layouts_are_pinned():
    assert capi.LOCAL_POINT_DTYPE.itemsize == 72 and C.sizeof(capi.TrackLocalResult) == 120
    assert list(capi.LOCAL_POINT_DTYPE.names) == ["pos", "normal", "min_dist", "max_dist", "desc", "n_obs", "bad"]


def test_integration_call_pattern_compiles_against_the_header(tmp_path):
    src = tmp_path / "track_local_map_pattern.cpp"
    src.write_text(PRELUDE + "\n" + _layout_asserts() + "\n" + _snippet())
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
