"""The C ABI of the rows beside the keyframes and of dvm_update_local_map (include/dvmslam_hip.h) without a GPU: the header compiles as C,
the struct sizes and offsets are the ones the Python mirrors use, and the built libraries export the new symbols."""
import ctypes as C
import os
import subprocess

import numpy as np

from dvm_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dvm_keyframe_store_set_rows", "dvm_keyframe_store_patch_rows", "dvm_keyframe_store_debug_read_rows", "dvm_update_local_map_create",
           "dvm_update_local_map_destroy", "dvm_update_local_map_reserve", "dvm_update_local_map_keyframes", "dvm_update_local_map_points",
           "dvm_update_local_map_last_bytes", "dvm_update_local_map_profile", "dvm_update_local_map_last_ms"]
MIRRORS = (("dvm_ulm_keyframes_in", "_UlmKeyframesIn", 32), ("dvm_ulm_keyframes_out", "_UlmKeyframesOut", 16), ("dvm_ulm_points_in", "_UlmPointsIn", 48),
           ("dvm_ulm_points_out", "_UlmPointsOut", 32))

USE = r"""
#include <stddef.h>
#include "dvmslam_hip.h"
%s
_Static_assert(sizeof(dvm_kfs_row_edit) == 12 && offsetof(dvm_kfs_row_edit, kp) == 4 && offsetof(dvm_kfs_row_edit, value) == 8, "dvm_kfs_row_edit");
_Static_assert(DVM_KFS_ROW_MATCHES == 0 && DVM_KFS_ROW_OBSERVED == 1, "row kinds");
int use(dvm_keyframe_store* ks, const dvm_map_store* ms, const int32_t* i32, int32_t* o32, const dvm_kfs_row_edit* e,
        const dvm_ulm_keyframes_in* ki, const dvm_ulm_keyframes_out* ko, const dvm_ulm_points_in* pi, dvm_ulm_points_out* po, int64_t* b, float* ms_out) {
  const int32_t* rows[1] = {i32};
  dvm_update_local_map* h = 0;
  int rc = dvm_keyframe_store_set_rows(ks, DVM_KFS_ROW_MATCHES, ms, 1, i32, rows);
  rc |= dvm_keyframe_store_patch_rows(ks, DVM_KFS_ROW_OBSERVED, ms, 1, e);
  rc |= dvm_keyframe_store_debug_read_rows(ks, DVM_KFS_ROW_MATCHES, 0, o32, 8, o32);
  rc |= dvm_update_local_map_create(0, &h);
  rc |= dvm_update_local_map_reserve(h, 32, 2048, 80, 100000, 2000, 2048);
  rc |= dvm_update_local_map_keyframes(h, 1, ki, ko);
  rc |= dvm_update_local_map_points(h, 1, pi, po);
  rc |= dvm_update_local_map_last_bytes(h, b, b);
  rc |= dvm_update_local_map_profile(h, 1);
  rc |= dvm_update_local_map_last_ms(h, ms_out);
  dvm_update_local_map_destroy(h);
  return rc;
}
"""


def _offset_asserts():
    out = []
    for name, mirror, size in MIRRORS:
        S = getattr(capi, mirror)
        out.append(f"_Static_assert(sizeof({name}) == {size}, \"{name} size as the header states it\");")
        out.append(f"_Static_assert(sizeof({name}) == {C.sizeof(S)}, \"{name} against the Python mirror\");")
        for f, _ in S._fields_:
            out.append(f"_Static_assert(offsetof({name}, {f}) == {getattr(S, f).offset}, \"{name}.{f}\");")
    return "\n".join(out)


def test_header_compiles_as_c_with_the_mirrored_layouts(tmp_path):
    src = tmp_path / "update_local_map_abi.c"
    src.write_text(USE % _offset_asserts())
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_layouts_are_pinned():
    for _, mirror, size in MIRRORS:
        assert C.sizeof(getattr(capi, mirror)) == size, mirror
    assert [f for f, _ in capi._UlmKeyframesIn._fields_] == ["kfs", "points", "n", "mp_slot"]
    assert [f for f, _ in capi._UlmKeyframesOut._fields_] == ["votes", "frame_bad"]
    assert [f for f, _ in capi._UlmPointsIn._fields_] == ["kfs", "points", "n_kfs", "kf_slot", "n", "mp_slot"]
    assert [f for f, _ in capi._UlmPointsOut._fields_] == ["local_slot", "local_cap", "n_local", "frame_mp", "n_outside"]
    assert [capi._UlmPointsOut.n_local.offset, capi._UlmPointsOut.frame_mp.offset, capi._UlmPointsOut.n_outside.offset] == [12, 16, 24]
    assert capi.KFS_ROW_EDIT_DTYPE.itemsize == 12 and capi.KFS_ROW_EDIT_DTYPE.names == ("slot", "kp", "value")
    assert (capi.KFS_ROW_MATCHES, capi.KFS_ROW_OBSERVED) == (0, 1)
    e = np.array([(1, 2, 3)], capi.KFS_ROW_EDIT_DTYPE)
    assert e.view(np.int32).tolist() == [1, 2, 3]


def test_library_exports_the_symbols():
    lib = capi.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dvm_slam_amd", "lib", "libdvmslam_hip.so")], capture_output=True, text=True).stdout
    for s in SYMBOLS:
        assert f" T {s}\n" in out, s
    host = capi.host_lib()                          # the host library links the device library
    for s in SYMBOLS:
        assert hasattr(host, s), s
    for name in ("set_rows", "patch_rows", "read_rows"):
        assert callable(getattr(capi.KeyframeStore, name))
    for name in ("reserve", "keyframes", "points", "last_bytes", "close"):
        assert callable(getattr(capi.UpdateLocalMap, name))
