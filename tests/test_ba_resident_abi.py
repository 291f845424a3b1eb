"""The C ABI of dvm_ba_resident (LocalBundleAdjustment on the resident stores): INTEGRATION.md's "LocalBundleAdjustment on the resident
stores" snippet compiles against the header, dvm_ba_obs and dvm_ba_window_resident keep their sizes and field offsets, the ctypes
structure and the numpy dtype of capi are the same layout, and the library exports the entry points."""
import ctypes as C
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dvm_slam_amd", "lib")

# field -> offset (LP64), written out by hand
OBS = dict(pose=0, point=4, kp=8)
WINDOW = dict(n_poses=0, n_points=4, n_edges=8, iterations=12, poses=16, fixed=24, keyframes=32, kf_slot=40, ow=48, points=56, mp_slot=64, obs=72,
              ref_edge=80, cam=88, chi2_erase=128, poses_out=136, points_out=144, edge_chi2_out=152, depth_positive_out=160, geometry_out=168,
              point_dirty_out=176, ow_out=184)


def _asserts():
    s = 'static_assert(sizeof(dvm_ba_obs) == 12, "dvm_ba_obs");\nstatic_assert(sizeof(dvm_ba_window_resident) == 192, "dvm_ba_window_resident");\n'
    s += "".join(f'static_assert(offsetof(dvm_ba_obs, {k}) == {v}, "{k}");\n' for k, v in OBS.items())
    s += "".join(f'static_assert(offsetof(dvm_ba_window_resident, {k}) == {v}, "{k}");\n' for k, v in WINDOW.items())
    return s


def _snippet():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## LocalBundleAdjustment on the resident stores"):]
    m = re.search(r"```cpp\n(.*?)```", sec, re.S)
    assert m, "no cpp block under the section"
    return m.group(1)


def test_integration_snippet_compiles_and_layouts_are_pinned():
    code = _snippet()
    for name in ("dvm_ba_resident_create", "dvm_ba_resident_optimize", "dvm_ba_resident_commit", "dvm_map_store_update", "dvm_ba_resident_destroy"):
        assert name in code, name
    src = '#include <cstddef>\n#include <cstdint>\n#include <vector>\n#include "dvmslam_hip.h"\n' + _asserts() + code
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "snippet.cpp")
        open(p, "w").write(src)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), p], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_structs_match_the_header():
    from dvm_slam_amd import capi
    assert capi.BA_OBS_DTYPE.itemsize == 12
    assert {k: capi.BA_OBS_DTYPE.fields[k][1] for k in OBS} == OBS
    assert C.sizeof(capi.BaWindowResident) == 192
    assert {k: getattr(capi.BaWindowResident, k).offset for k in WINDOW} == WINDOW
    assert [f[0] for f in capi.BaWindowResident._fields_] == list(WINDOW)


def test_new_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, "libdvmslam_hip.so")], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in ("dvm_ba_resident_create", "dvm_ba_resident_destroy", "dvm_ba_resident_optimize", "dvm_ba_resident_commit", "dvm_ba_resident_last_bytes"):
        assert s in syms, s
