"""The batched reference-keyframe chain's C ABI (include/dvmslam_hip.h: dvm_tracker_reserve_reference_keyframe_batch,
dvm_track_reference_keyframe_batch) without a GPU: both are declared, the per-tick call pattern INTEGRATION.md gives for the fallback compiles
against the headers, and the Python side (capi.TrackerBatch) wraps both."""
import os
import re
import subprocess

from dvm_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = r"""
#include <cstddef>
#include <cstdint>
#include <vector>
#include "dvmslam_hip.h"
#include "dvmslam_host.h"
"""


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvmslam_hip.h")).read(), flags=re.S)


def _snippet():
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    head = "**The reference-keyframe fallback in a batched tick.**"
    assert head in txt, "INTEGRATION.md: the batched reference-keyframe fallback is missing"
    m = re.search(r"```cpp\n(.*?)```", txt[txt.index(head):], re.S)
    assert m, "INTEGRATION.md: the batched fallback's call pattern is missing"
    for name in ("dvmh_track_with_motion_model_batch", "dvm_track_reference_keyframe_batch", "dvm_track_local_map_batch"):
        assert name in m.group(1), name
    return m.group(1)


def test_both_calls_are_declared():
    txt = _header()
    assert re.search(r"int\s+dvm_tracker_reserve_reference_keyframe_batch\s*\(\s*dvm_tracker\*\s*t,\s*int\s+max_total_kf_keypoints\s*\)", txt)
    assert re.search(r"int\s+dvm_track_reference_keyframe_batch\s*\(\s*dvm_tracker\*\s*t,\s*dvm_orb\*\s*h,\s*const\s+dvm_vocab\*\s*voc,\s*int\s+count,"
                     r"\s*const\s+dvm_ref_keyframe\*\s*const\*\s*kfs,\s*const\s+dvm_track_refkf_params\*\s*ps,\s*const\s+dvm_track_refkf_out\*\s*outs,"
                     r"\s*dvm_track_refkf_result\*\s*res,\s*int32_t\*\s*status\s*\)", txt)
    # the single call and its reservation keep their signatures
    assert re.search(r"int\s+dvm_tracker_reserve_reference_keyframe\s*\(\s*dvm_tracker\*\s*t,\s*int\s+max_kf_keypoints\s*\)", txt)
    assert re.search(r"int\s+dvm_track_reference_keyframe\s*\(\s*dvm_tracker\*\s*t,\s*dvm_orb\*\s*h,\s*const\s+dvm_vocab\*\s*voc,"
                     r"\s*const\s+dvm_ref_keyframe\*\s*kf,", txt)


def test_fallback_tick_pattern_compiles_against_the_header(tmp_path):
    src = tmp_path / "track_refkf_tick_pattern.cpp"
    src.write_text(PRELUDE + "\n" + _snippet())
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_tracker_batch_wraps_both_calls():
    import inspect
    assert callable(getattr(capi.TrackerBatch, "reserve_reference_keyframe", None))
    assert callable(getattr(capi.TrackerBatch, "track_reference_keyframe", None))
    params = list(inspect.signature(capi.TrackerBatch.track_reference_keyframe).parameters)
    assert params[:6] == ["self", "voc", "kfs", "poses_last", "K", "inv_sigma2"]
    for k in ("nnratio", "check_ori", "th_low", "min_matches", "min_map", "levelsup"):
        assert k in params, k
