"""The C ABI of the batched local-BA windows on a camera model: INTEGRATION.md's "A fisheye fleet's local BA windows" snippet compiles
against the headers, libdvmslam_hip.so exports dvm_ba_optimize_windows_fast_cam and dvm_ba_pool_optimize_cam, and a bad model is
DVM_ERR_INVALID before the device is looked for (so also on a machine without one)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dvm_slam_amd", "lib")
DVM_ERR_INVALID = -1


def _snippet():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    title = "\n### A fisheye fleet's local BA windows\n"
    assert text.index("\n## A KannalaBrandt8 agent") < text.index(title)
    assert "\n## " not in text[text.index("\n## A KannalaBrandt8 agent") + 4:text.index(title)]      # a subsection of that section
    sec = text[text.index(title):]
    m = re.search(r"```cpp\n(.*?)```", sec, re.S)
    assert m, "no cpp block under the fisheye fleet section"
    return m.group(1)


def test_integration_snippet_compiles():
    code = _snippet()
    assert "dvm_ba_optimize_windows_fast_cam" in code and "dvm_ba_pool_optimize_cam" in code
    src = ('#include <cstddef>\n#include <cstdint>\n#include <vector>\n#include "dvmslam_hip.h"\n'
           "static_assert(sizeof(dvm_camera_model) == 36, \"dvm_camera_model\");\n" + code)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "snippet.cpp")
        open(p, "w").write(src)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), p], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_new_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, "libdvmslam_hip.so")], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "dvm_ba_optimize_windows_fast_cam" in names and "dvm_ba_pool_optimize_cam" in names
    assert "dvm_ba_optimize_windows_fast" in names and "dvm_ba_pool_optimize" in names


def _one_window(capi):
    poses = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (2, 1)); points = np.array([[0.1, 0.2, 5.0]])
    edges = np.zeros(2, capi.BA_EDGE_DTYPE); edges["pose"] = [0, 1]; edges["inv_sigma2"] = 1.0
    return dict(poses=poses, fixed=np.array([1, 0], np.uint8), points=points, edges=edges, huber_delta=2.0, iterations=1)


@pytest.mark.parametrize("bad", ["unknown", "zero_fx", "zero_fy_pinhole", "null"])
def test_bad_model_is_invalid_before_the_device(capi, bad):
    """Two windows, the bad model second: DVM_ERR_INVALID -- not DVM_ERR_NO_DEVICE where there is no GPU -- and no output written."""
    good = capi.CameraModel.robomaster()
    m = {"unknown": capi.CameraModel.make(7, list(good.p)), "zero_fx": capi.CameraModel.make(1, [0.0] + list(good.p)[1:]),
         "zero_fy_pinhole": capi.CameraModel.make(0, [400.0, 0.0, 480.0, 270.0]), "null": None}[bad]
    batch = capi.BaWindowBatch([dict(_one_window(capi), model=good), dict(_one_window(capi), model=good)])
    if m is not None:
        batch.models[1] = m
    for o in batch.outs:
        o["poses"][:] = 7.0
    f = capi.lib().dvm_ba_optimize_windows_fast_cam
    f.restype = C.c_int32; f.argtypes = None
    rc = f(C.c_int32(0), batch.wins, batch.models if m is not None else None, C.c_int32(2), None, batch.stats)
    assert rc == DVM_ERR_INVALID
    assert all(np.all(o["poses"] == 7.0) for o in batch.outs)
    g = capi.lib().dvm_ba_pool_optimize_cam                   # the pool entry checks the model before it looks at the pool
    g.restype = C.c_int32; g.argtypes = None
    one = (capi.CameraModel * 1)(m) if m is not None else None
    assert g(None, batch.wins, one, batch.stats, None) == DVM_ERR_INVALID


def test_python_wrapper_refuses_a_model_outside_the_fast_form(capi):
    batch = capi.BaWindowBatch([dict(_one_window(capi), model=capi.CameraModel.tum())])
    with pytest.raises(ValueError):
        batch.run(fast=False)
    assert capi.BaWindowBatch([dict(_one_window(capi), intrinsics=(400.0, 380.0, 480.0, 270.0))]).models is None
