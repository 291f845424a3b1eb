"""The C ABI of the KannalaBrandt8 tracked-frame chains: INTEGRATION.md's "A fisheye agent's tracked frame" snippet compiles against the
headers, dvm_camera_model keeps its size, and both libraries export the new entry points."""
import ctypes as C
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dvm_slam_amd", "lib")


def _snippet():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("A fisheye agent's tracked frame"):]
    m = re.search(r"```cpp\n(.*?)```", sec, re.S)
    assert m, "no cpp block under the fisheye section"
    return m.group(1)


def test_integration_snippet_compiles():
    code = _snippet()
    assert "dvmh_track_with_motion_model_cam" in code and "dvm_track_local_map" in code
    src = ('#include <cstddef>\n#include <cstdint>\n#include <vector>\n#include "dvmslam_hip.h"\n#include "dvmslam_host.h"\n'
           "static_assert(sizeof(dvm_camera_model) == 36, \"dvm_camera_model\");\n" + code)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "snippet.cpp")
        open(p, "w").write(src)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), p], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_camera_model_is_36_bytes():
    class M(C.Structure):
        _fields_ = [("model", C.c_int32), ("p", C.c_float * 8)]
    assert C.sizeof(M) == 36
    hdr = open(os.path.join(ROOT, "include", "dvmslam_hip.h")).read()
    assert re.search(r"typedef struct \{ int32_t model;.*?float p\[8\];.*?\} dvm_camera_model;", hdr, re.S)


def _exports(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_new_symbols_are_exported():
    assert "dvm_tracker_set_camera_model" in _exports("libdvmslam_hip.so")
    host = _exports("libdvmslam_host.so")
    assert "dvmh_track_with_motion_model_cam" in host and "dvmh_track_with_motion_model_batch_cam" in host
