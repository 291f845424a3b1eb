"""The C ABI of the BoW-targets chain (include/dvmslam_hip.h: dvm_bt_keyframe, dvm_bow_targets_*, dvm_search_by_bow_targets;
include/dvmslam_host.h: dvmh_search_by_bow_targets) without a GPU: both headers compile as C, the struct has the size the header states
and the layout the Python side (capi._BtKeyFrame) uses, the built libraries export the symbols, and create refuses without a device."""
import ctypes as C
import os
import subprocess

import pytest

from dvm_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = ["dvm_bow_targets_create", "dvm_bow_targets_destroy", "dvm_bow_targets_reserve", "dvm_search_by_bow_targets",
                  "dvm_bow_targets_profiling", "dvm_bow_targets_last_kernel_ms"]

USE = r"""
#include <stddef.h>
#include "dvmslam_host.h"
_Static_assert(sizeof(dvm_bt_keyframe) == 64, "dvm_bt_keyframe size");
%s
int use(dvm_bow_targets* h, const dvm_bt_keyframe* cur, const dvm_bt_keyframe* targets, int* idx2, int* nm, float* ms,
        const dvmh_keyframe_view* KF1, const dvmh_keyframe_view* kfs, int* m12) {
  int rc = dvm_bow_targets_create(0, &h);
  rc |= dvm_bow_targets_reserve(h, 1200, 33, 33 * 1200);
  rc |= dvm_search_by_bow_targets(h, cur, 33, targets, 0.9f, 1, idx2, nm);
  rc |= dvm_bow_targets_profiling(h, 1);
  rc |= dvm_bow_targets_last_kernel_ms(h, ms);
  dvm_bow_targets_destroy(h);
  return rc | dvmh_search_by_bow_targets(0, KF1, 33, kfs, 0.9f, 1, m12, idx2, nm);
}
"""


def _offset_asserts():
    S = capi._BtKeyFrame
    out = [f"_Static_assert(sizeof(dvm_bt_keyframe) == {C.sizeof(S)}, \"dvm_bt_keyframe against the Python mirror\");"]
    for f, _ in S._fields_:
        out.append(f"_Static_assert(offsetof(dvm_bt_keyframe, {f}) == {getattr(S, f).offset}, \"dvm_bt_keyframe.{f}\");")
    return "\n".join(out)


def test_headers_compile_as_c_with_the_stated_layout(tmp_path):
    src = tmp_path / "bow_targets_abi.c"
    src.write_text(USE % _offset_asserts())
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_layout_is_pinned():
    assert C.sizeof(capi._BtKeyFrame) == 64
    assert [f for f, _ in capi._BtKeyFrame._fields_] == ["n", "fv_n", "kps", "desc", "mp", "bad", "fv_node", "fv_off", "fv_feat"]


def test_libraries_export_the_symbols():
    lib, host = capi.lib(), capi.host_lib()
    for s in DEVICE_SYMBOLS:
        assert hasattr(lib, s), s
    assert hasattr(host, "dvmh_search_by_bow_targets")
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dvm_slam_amd", "lib", "libdvmslam_hip.so")], capture_output=True, text=True).stdout
    for s in DEVICE_SYMBOLS:
        assert f" T {s}\n" in out, s


def test_create_needs_a_device():
    if capi.device_count() > 0:
        h = capi.BowTargets()          # with a device the handle opens, and closes
        h.close()
        return
    out = C.c_void_p(0xdead)
    L = capi.lib()
    L.dvm_bow_targets_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    assert L.dvm_bow_targets_create(0, C.byref(out)) == -5 and not out.value
    with pytest.raises(capi.DvmError) as e:
        capi.BowTargets()
    assert e.value.code == -5
    with pytest.raises(capi.DvmError) as e:   # the host entry opens the calling thread's handle first: the same refusal
        import bow_targets_scene as bts
        sc = bts.scene(0, 1)
        capi.search_by_bow_targets(capi.keyframe_view(sc["cur"]), [capi.keyframe_view(k) for k in sc["targets"]])
    assert e.value.code == -5
