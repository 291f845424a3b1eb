"""The batched second half's C ABI (include/dvmslam_hip.h: dvm_local_map_in, dvm_local_map_out, dvm_track_local_map_batch) without a GPU:
the per-tick call pattern INTEGRATION.md gives for several agents compiles against the headers, and the layouts the header defines are the
ones the Python side (capi.LocalMapIn, capi.LocalMapOut) writes."""
import ctypes as C
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


def _snippet():
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = txt[txt.index("**The whole tracked frame of several agents per tick.**"):]
    m = re.search(r"```cpp\n(.*?)```", sec, re.S)
    assert m, "INTEGRATION.md: the batched second half's call pattern is missing"
    assert "dvm_track_local_map_batch" in m.group(1)
    return m.group(1)


def _layout_asserts():
    out = []
    for cname, S in (("dvm_local_map_in", capi.LocalMapIn), ("dvm_local_map_out", capi.LocalMapOut)):
        out.append(f"static_assert(sizeof({cname}) == {C.sizeof(S)}, \"{cname} size\");")
        for name, _ in S._fields_:
            out.append(f"static_assert(offsetof({cname}, {name}) == {getattr(S, name).offset}, \"{cname}.{name}\");")
    return "\n".join(out)


def test_layouts_are_pinned():
    assert C.sizeof(capi.LocalMapIn) == 40 and C.sizeof(capi.LocalMapOut) == 24
    assert [(n, getattr(capi.LocalMapIn, n).offset) for n, _ in capi.LocalMapIn._fields_] == [
        ("pts", 0), ("n", 8), ("frame_mp", 16), ("th", 24), ("far_points", 28), ("th_far", 32)]
    assert [(n, getattr(capi.LocalMapOut, n).offset) for n, _ in capi.LocalMapOut._fields_] == [("mp_out", 0), ("outlier", 8), ("track_pts", 16)]


def test_batch_call_is_declared():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvmslam_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+dvm_track_local_map_batch\s*\(\s*dvm_tracker\*\s*t,\s*dvm_orb\*\s*h,\s*int\s+count,\s*const\s+dvm_local_map_in\*\s*in,"
                     r"\s*const\s+dvm_local_map_out\*\s*out,\s*dvm_track_local_result\*\s*res,\s*int32_t\*\s*status\)", txt)


def test_per_tick_call_pattern_compiles_against_the_header(tmp_path):
    src = tmp_path / "track_tick_pattern.cpp"
    src.write_text(PRELUDE + "\n" + _layout_asserts() + "\n" + _snippet())
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
