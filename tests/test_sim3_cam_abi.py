"""The C ABI of the two Sim3 entries on a camera model per keyframe (include/dvmslam_hip.h: dvm_sim3_hypotheses_cam,
dvm_optimize_sim3_cam) without a GPU: the header compiles as C with the stated size and argument order, the library exports the
symbols, and a NULL model, a model outside {0, 1} or a zero focal length is refused with DVM_ERR_INVALID before anything is written."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dvm_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dvm_sim3_hypotheses_cam", "dvm_optimize_sim3_cam"]

USE = r"""
#include <stddef.h>
#include "dvmslam_hip.h"
_Static_assert(sizeof(dvm_camera_model) == 36, "dvm_camera_model size");
_Static_assert(offsetof(dvm_camera_model, model) == 0 && offsetof(dvm_camera_model, p) == 4, "dvm_camera_model layout");
int (*hyp)(int, const float*, const float*, const float*, const float*, int, const dvm_camera_model*, const dvm_camera_model*, const int32_t*, int,
           int, float*, int32_t*, uint8_t*) = dvm_sim3_hypotheses_cam;
int (*opt)(int, double*, int, const double*, const double*, const double*, const double*, const double*, const double*, int,
           const dvm_camera_model*, const dvm_camera_model*, double, uint8_t*, int32_t*) = dvm_optimize_sim3_cam;
"""


def test_header_compiles_as_c_with_the_stated_signatures(tmp_path):
    src = tmp_path / "sim3_cam_abi.c"
    src.write_text(USE)
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert C.sizeof(capi.CameraModel) == 36


def test_library_exports_the_symbols():
    lib = capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dvm_slam_amd", "lib", "libdvmslam_hip.so")], capture_output=True, text=True).stdout
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert f" T {s}\n" in out, s
    assert callable(capi.sim3_hypotheses_cam) and callable(capi.optimize_sim3_cam)
    from dvm_slam_amd import merge
    assert hasattr(merge.GpuOps, "sim3_hypotheses_cam") and hasattr(merge.GpuOps, "optimize_sim3_cam")


def _bad_models():
    good = capi.CameraModel.robomaster()
    two = capi.CameraModel.make(2, list(good.params))
    fx0 = capi.CameraModel.make(1, [0.0] + list(good.params)[1:])
    fy0 = capi.CameraModel.make(0, [500.0, 0.0, 320.0, 240.0])
    return good, [("NULL", None), ("model 2", two), ("fx == 0", fx0), ("fy == 0", fy0)]


@pytest.mark.parametrize("side", [0, 1])
def test_refused_models(side):
    """Each bad model on either side: DVM_ERR_INVALID, the outputs as they were.  (No device is needed: the check comes first.)"""
    lib = capi.lib()
    vp, i32 = C.c_void_p, C.c_int32
    lib.dvm_sim3_hypotheses_cam.restype = i32
    lib.dvm_sim3_hypotheses_cam.argtypes = [i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, vp, vp]
    lib.dvm_optimize_sim3_cam.restype = i32
    lib.dvm_optimize_sim3_cam.argtypes = [i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, C.c_double, vp, vp]
    n, h = 12, 4
    rng = np.random.default_rng(0)
    P = rng.uniform(1, 5, (n, 3))
    Pf, e, tri = P.astype(np.float32), np.full(n, 9.0, np.float32), np.array([[0, 1, 2]] * h, np.int32)
    o, w = rng.uniform(0, 500, (n, 2)), np.ones(n)
    good, bad = _bad_models()
    p = lambda a: a.ctypes.data
    for what, m in bad:
        pair = [C.addressof(good), C.addressof(good)]
        pair[side] = None if m is None else C.addressof(m)
        T = np.full((h, 13), 7.5, np.float32); nin = np.full(h, -77, np.int32); mask = np.full((h, n), 0xAA, np.uint8)
        assert lib.dvm_sim3_hypotheses_cam(0, p(Pf), p(Pf), p(e), p(e), n, pair[0], pair[1], p(tri), h, 0, p(T), p(nin), p(mask)) == -1, what
        assert (T == 7.5).all() and (nin == -77).all() and (mask == 0xAA).all(), what
        S = np.array([0, 0, 0, 1, 0.1, 0.2, 0.3, 1.1]); S0 = S.copy()
        inl = np.full(n, 0xAA, np.uint8); cnt = np.full(1, -77, np.int32)
        assert lib.dvm_optimize_sim3_cam(0, p(S), 0, p(P), p(P), p(o), p(o), p(w), p(w), n, pair[0], pair[1], 10.0, p(inl), p(cnt)) == -1, what
        assert np.array_equal(S, S0) and (inl == 0xAA).all() and cnt[0] == -77, what
