"""The C ABI of the Fuse chain's camera-model, Scw-form and hits entries (include/dvmslam_hip.h: dvm_fuse_targets_set_cam, dvm_ft_hit,
dvm_fuse_targets_reserve_hits, dvm_fuse_targets_run_hits; include/dvmslam_host.h: dvmh_fuse_targets_cam, dvmh_fuse_sim3_targets,
dvmh_fuse_sim3_apply) without a GPU: the headers compile as C with the stated sizes, the libraries export the symbols, and the argument
refusals that need no device answer DVM_ERR_INVALID."""
import ctypes as C
import os
import subprocess

import numpy as np

from dvm_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = ["dvm_fuse_targets_set_cam", "dvm_fuse_targets_reserve_hits", "dvm_fuse_targets_run_hits"]
HOST_SYMBOLS = ["dvmh_fuse_targets_cam", "dvmh_fuse_sim3_targets", "dvmh_fuse_sim3_apply"]

USE = r"""
#include <stddef.h>
#include "dvmslam_host.h"
_Static_assert(sizeof(dvm_ft_hit) == 12, "dvm_ft_hit size");
_Static_assert(sizeof(dvm_ft_target) == 120, "dvm_ft_target size");
_Static_assert(sizeof(dvm_camera_model) == 36, "dvm_camera_model size");
_Static_assert(offsetof(dvm_ft_hit, point) == 0 && offsetof(dvm_ft_hit, idx) == 4 && offsetof(dvm_ft_hit, dist) == 8, "dvm_ft_hit layout");
_Static_assert(DVM_FT_FORM_POINTS == 0 && DVM_FT_FORM_SCW == 1, "forms");
int use(dvm_fuse_targets* h, const dvm_ft_target* t, const dvm_camera_model* m, const unsigned char* forms, const dvm_ft_points* p,
        const unsigned char* skip, int* off, dvm_ft_hit* hits, int* n_hits, dvmh_keyframe_view* kfs, const dvm_sim3f* S,
        const dvmh_map_points_view* P, int* idx, int* replace) {
  int rc = dvm_fuse_targets_set_cam(h, 140, t, m, forms);
  rc |= dvm_fuse_targets_set_cam(h, 140, t, NULL, NULL);
  rc |= dvm_fuse_targets_reserve_hits(h, 4000);
  rc |= dvm_fuse_targets_run_hits(h, p, skip, 4.0f, off, hits, 4000, n_hits);
  rc |= dvmh_fuse_targets_cam(0, 140, kfs, m, P, skip, 3.0f, idx);
  rc |= dvmh_fuse_sim3_targets(0, 140, kfs, S, m, P, 4.0f, off, hits, 4000);
  return rc | dvmh_fuse_sim3_apply(kfs, P, hits, 10, replace);
}
"""


def test_headers_compile_as_c_with_the_stated_layouts(tmp_path):
    src = tmp_path / "fuse_cam_abi.c"
    src.write_text(USE)
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert capi.HIT_DTYPE.itemsize == 12 and capi.HIT_DTYPE.names == ("point", "idx", "dist")
    assert C.sizeof(capi._FtTarget) == 120 and C.sizeof(capi.CameraModel) == 36


def test_libraries_export_the_symbols():
    lib, host = capi.lib(), capi.host_lib()
    for s in DEVICE_SYMBOLS:
        assert hasattr(lib, s), s
    for s in HOST_SYMBOLS:
        assert hasattr(host, s), s
    for name, syms in (("libdvmslam_hip.so", DEVICE_SYMBOLS), ("libdvmslam_host.so", HOST_SYMBOLS)):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dvm_slam_amd", "lib", name)], capture_output=True, text=True).stdout
        for s in syms:
            assert f" T {s}\n" in out, s


def test_refusals_that_need_no_device():
    lib, host = capi.lib(), capi.host_lib()
    vp, i32 = C.c_void_p, C.c_int32
    lib.dvm_fuse_targets_set_cam.restype = i32; lib.dvm_fuse_targets_set_cam.argtypes = [vp, i32, vp, vp, vp]
    lib.dvm_fuse_targets_reserve_hits.restype = i32; lib.dvm_fuse_targets_reserve_hits.argtypes = [vp, i32]
    lib.dvm_fuse_targets_run_hits.restype = i32; lib.dvm_fuse_targets_run_hits.argtypes = [vp, vp, vp, C.c_float, vp, vp, i32, vp]
    assert lib.dvm_fuse_targets_set_cam(None, 0, None, None, None) == -1
    assert lib.dvm_fuse_targets_reserve_hits(None, 10) == -1
    off = np.full(4, -7, np.int32)
    assert lib.dvm_fuse_targets_run_hits(None, None, None, 4.0, off.ctypes.data, None, 0, None) == -1 and np.all(off == -7)
    P, _ = capi.map_points_view(dict(pos=np.zeros((3, 3), np.float32), normal=np.zeros((3, 3), np.float32), min_dist=np.ones(3, np.float32),
                                     max_dist=np.ones(3, np.float32), desc=np.zeros((3, 32), np.uint8), id=np.arange(3, dtype=np.int32)))
    for fn in (host.dvmh_fuse_targets_cam, host.dvmh_fuse_sim3_targets, host.dvmh_fuse_sim3_apply):
        fn.restype = i32; fn.argtypes = None
    assert host.dvmh_fuse_targets_cam(i32(0), i32(-1), None, None, C.byref(P), None, C.c_float(3.0), None) == -1
    assert host.dvmh_fuse_targets_cam(i32(0), i32(2), None, None, C.byref(P), None, C.c_float(3.0), None) == -1          # targets missing
    assert host.dvmh_fuse_sim3_targets(i32(0), i32(-1), None, None, None, C.byref(P), C.c_float(4.0), vp(off.ctypes.data), None, i32(0)) == -1
    assert host.dvmh_fuse_sim3_targets(i32(0), i32(0), None, None, None, C.byref(P), C.c_float(4.0), None, None, i32(0)) == -1   # hit_off missing
    assert host.dvmh_fuse_sim3_targets(i32(0), i32(0), None, None, None, C.byref(P), C.c_float(4.0), vp(off.ctypes.data), None, i32(5)) == -1   # hits missing
    # the apply step: a hit outside the point table or outside the keyframe is refused and nothing is written
    kf = dict(kps=np.zeros(4, capi.KP_DTYPE), desc=np.zeros((4, 32), np.uint8), mp=np.full(4, -1, np.int32), bounds=(0.0, 640.0, 0.0, 480.0))
    KF = capi.keyframe_view(kf)
    hit = np.zeros(1, capi.HIT_DTYPE)
    for point, idx in ((3, 0), (-1, 0), (0, 4), (0, -1)):
        hit["point"], hit["idx"] = point, idx
        rep = np.full(3, -7, np.int32)
        assert host.dvmh_fuse_sim3_apply(C.byref(KF[0]), C.byref(P), vp(hit.ctypes.data), i32(1), vp(rep.ctypes.data)) == -1
        assert np.all(rep == -7) and np.all(kf["mp"] == -1)
    assert host.dvmh_fuse_sim3_apply(C.byref(KF[0]), C.byref(P), None, i32(1), vp(rep.ctypes.data)) == -1
    assert host.dvmh_fuse_sim3_apply(None, C.byref(P), None, i32(0), vp(rep.ctypes.data)) == -1
    hit["point"], hit["idx"] = 2, 1
    n, rep = capi.fuse_sim3_apply(KF, (P, None), hit)
    assert n == 1 and list(rep) == [-1, -1, -1] and list(kf["mp"]) == [-1, 2, -1, -1]
