"""The C ABI of the device-resident map-point store and the tracked-frame halves that read it: INTEGRATION.md's "An agent's map points
resident on the device" snippet compiles against both headers, the new structs keep their sizes, both libraries export the new entry
points, and the host's query builder (dvmh_build_frame_queries) equals a numpy float32 restatement of the loop header of
SearchByProjection(CurrentFrame, LastFrame)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import resident_scene as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dvm_slam_amd", "lib")

SIZES = ('static_assert(sizeof(dvm_local_point) == 72, "dvm_local_point");\n'
         'static_assert(sizeof(dvm_track_last) == 72, "dvm_track_last");\n'
         'static_assert(sizeof(dvm_track_shared) == 104, "dvm_track_shared");\n'
         'static_assert(sizeof(dvm_local_map_in_resident) == 48, "dvm_local_map_in_resident");\n'
         'static_assert(sizeof(dvmh_track_in_resident) == sizeof(dvmh_track_in), "dvmh_track_in_resident");\n')


def _snippet():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## An agent's map points resident on the device"):]
    m = re.search(r"```cpp\n(.*?)```", sec, re.S)
    assert m, "no cpp block under the resident section"
    return m.group(1)


def test_integration_snippet_compiles_and_struct_sizes_are_pinned():
    code = _snippet()
    for name in ("dvm_map_store_update", "dvmh_track_with_motion_model_batch_resident", "dvm_track_local_map_batch_resident"):
        assert name in code, name
    src = '#include <cstddef>\n#include <cstdint>\n#include <vector>\n#include "dvmslam_hip.h"\n#include "dvmslam_host.h"\n' + SIZES + code
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "snippet.cpp")
        open(p, "w").write(src)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), p], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_structs_match_the_header():
    from dvm_slam_amd import capi
    assert C.sizeof(capi.TrackLast) == 72 and C.sizeof(capi.TrackShared) == 104 and C.sizeof(capi.LocalMapInResident) == 48
    assert capi.LOCAL_POINT_DTYPE.itemsize == 72 and capi.LOCAL_POINT_DTYPE == rs.LOCAL_POINT_DTYPE


def _exports(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_new_symbols_are_exported():
    hip = _exports("libdvmslam_hip.so")
    for s in ("dvm_map_store_create", "dvm_map_store_destroy", "dvm_map_store_capacity", "dvm_map_store_update", "dvm_map_store_read",
              "dvm_track_finish_batch_resident", "dvm_track_debug_build_queries", "dvm_tracker_last_upload_bytes",
              "dvm_track_local_map_batch_resident"):
        assert s in hip, s
    host = _exports("libdvmslam_host.so")
    assert "dvmh_build_frame_queries" in host and "dvmh_track_with_motion_model_batch_resident" in host


def test_host_query_builder_equals_numpy_restatement():
    from dvm_slam_amd import capi
    e = rs.entries(200, "mix", seed=12345, store_cap=260)
    assert all((e["fate"] == f).any() for f in range(6))
    for th in (15.0, 30.0):
        host = capi.build_frame_queries_host(dict(e, th=th), rs.K, rs.BOUNDS, rs.SCALE, e["records"])
        ref = rs.loop_header_numpy(e, th)
        rs.assert_queries_equal(host, ref)
        assert 0 < host["nq"] == int((e["fate"] == 0).sum()) < 200
    assert (host["q_claims"] == 0).any() and (host["q_claims"] == 1).any()
