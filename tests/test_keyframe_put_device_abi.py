"""The C ABI of dvm_keyframe_store_put_device / _put_tracked / _last_put_bytes (include/dvmslam_hip.h: dvm_kfs_device_keyframe,
dvm_kfs_bow_out) without a GPU: the header compiles as C, the struct sizes and offsets are the ones the header states and the Python
mirrors use, the built libraries export the symbols, and the entries refuse what they can refuse without a device."""
import ctypes as C
import os
import re
import subprocess

from dvm_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = ["dvm_keyframe_store_put_device", "dvm_keyframe_store_put_tracked", "dvm_keyframe_store_last_put_bytes", "dvm_keyframe_store_profile",
                  "dvm_keyframe_store_last_put_ms"]
MIRRORS = (("dvm_kfs_device_keyframe", "_KfsDeviceKeyframe", 96), ("dvm_kfs_bow_out", "_KfsBowOut", 56))

USE = r"""
#include <stddef.h>
#include "dvmslam_hip.h"
%s
int use(dvm_keyframe_store* st, dvm_tracker* t, dvm_orb* h, const dvm_vocab* voc, void* stream, const int32_t* frames, const int32_t* slots,
        const dvm_kfs_device_keyframe* kfs, dvm_kfs_bow_out* outs, int64_t* bytes, float* ms) {
  int rc = dvm_keyframe_store_put_device(st, voc, 4, stream, 3, slots, kfs, outs);
  rc |= dvm_keyframe_store_put_tracked(st, t, h, voc, 4, 3, frames, slots, kfs, outs);
  rc |= dvm_keyframe_store_last_put_bytes(st, bytes);
  rc |= dvm_keyframe_store_profile(st, 1);
  rc |= dvm_keyframe_store_last_put_ms(st, ms);
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
    src = tmp_path / "keyframe_put_device_abi.c"
    src.write_text(USE % _offset_asserts())
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_header_states_the_sizes():
    txt = open(os.path.join(ROOT, "include", "dvmslam_hip.h")).read()
    for name, mirror, size in MIRRORS:
        assert C.sizeof(getattr(capi, mirror)) == size, mirror
        assert re.search(rf"sizeof\({name}\) == {size}\b", txt), name
    assert [f for f, _ in capi._KfsDeviceKeyframe._fields_][:4] == ["d_kps", "d_desc", "d_n", "n"]
    assert [f for f, _ in capi._KfsBowOut._fields_] == ["n", "n_bow", "n_fv", "n_feat", "bow_ids", "bow_vals", "fv_node", "fv_off", "fv_feat"]


def test_library_exports_the_symbols():
    lib = capi.lib()
    for s in DEVICE_SYMBOLS:
        assert hasattr(lib, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dvm_slam_amd", "lib", "libdvmslam_hip.so")], capture_output=True, text=True).stdout
    for s in DEVICE_SYMBOLS:
        assert f" T {s}\n" in out, s
    host = capi.host_lib()
    for s in DEVICE_SYMBOLS:
        assert hasattr(host, s), s
    for name in ("put_device", "put_tracked", "last_put_bytes", "device_records"):
        assert hasattr(capi.KeyframeStore, name), name


def test_missing_arguments_are_refused_without_a_device():
    L = capi.lib()
    vp, i32 = C.c_void_p, C.c_int32
    L.dvm_keyframe_store_put_device.restype = i32; L.dvm_keyframe_store_put_device.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp]
    L.dvm_keyframe_store_put_tracked.restype = i32; L.dvm_keyframe_store_put_tracked.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
    L.dvm_keyframe_store_last_put_bytes.restype = i32; L.dvm_keyframe_store_last_put_bytes.argtypes = [vp, vp]
    L.dvm_keyframe_store_last_put_ms.restype = i32; L.dvm_keyframe_store_last_put_ms.argtypes = [vp, vp]
    L.dvm_keyframe_store_profile.restype = i32; L.dvm_keyframe_store_profile.argtypes = [vp, i32]
    slots = (C.c_int32 * 1)(0)
    kf = capi._KfsDeviceKeyframe()
    b = C.c_int64(0)
    INVALID = -1
    assert L.dvm_keyframe_store_put_device(None, None, 4, None, 1, slots, C.byref(kf), None) == INVALID     # no store, no vocabulary
    assert L.dvm_keyframe_store_put_tracked(None, None, None, None, 4, 1, slots, slots, C.byref(kf), None) == INVALID
    assert L.dvm_keyframe_store_last_put_bytes(None, C.byref(b)) == INVALID
    assert L.dvm_keyframe_store_last_put_ms(None, None) == INVALID and L.dvm_keyframe_store_profile(None, 1) == INVALID
