"""The C ABI of dvm_keyframe_store and of the chains that read it (include/dvmslam_hip.h: dvm_kfs_keyframe, dvm_kfs_readback,
dvm_ft_target_resident, dvm_np_keyframe_resident, dvm_np_neighbour_resident) without a GPU: the header compiles as C, the struct sizes
and offsets are the ones the Python mirrors use, the built libraries export the new symbols, and create names the missing device."""
import ctypes as C
import os
import subprocess

from dvm_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = ["dvm_keyframe_store_create", "dvm_keyframe_store_destroy", "dvm_keyframe_store_capacity", "dvm_keyframe_store_slot_keypoints",
                  "dvm_keyframe_store_put", "dvm_keyframe_store_remove", "dvm_keyframe_store_debug_read", "dvm_fuse_targets_set_resident",
                  "dvm_fuse_targets_last_upload_bytes", "dvm_create_new_map_points_resident", "dvm_new_points_last_upload_bytes"]
MIRRORS = (("dvm_kfs_keyframe", "_KfsKeyframe", 120), ("dvm_kfs_readback", "_KfsReadback", 160), ("dvm_ft_target_resident", "_FtTargetResident", 44),
           ("dvm_np_keyframe_resident", "_NpKeyFrameResident", 88), ("dvm_np_neighbour_resident", "_NpNeighbourResident", 136))

USE = r"""
#include <stddef.h>
#include "dvmslam_hip.h"
%s
int use(dvm_keyframe_store* st, dvm_fuse_targets* ft, dvm_new_points* np, const int32_t* slots, const dvm_kfs_keyframe* kfs, dvm_kfs_readback* back,
        const dvm_ft_target_resident* t, const dvm_camera_model* m, const unsigned char* forms, const dvm_np_keyframe_resident* cur,
        const dvm_np_neighbour_resident* nbs, const dvm_pair_pose* poses, const dvm_np_params* p, dvm_np_out* out, int64_t* bytes) {
  int rc = dvm_keyframe_store_create(0, 128, 2048, &st);
  rc |= dvm_keyframe_store_capacity(st) | dvm_keyframe_store_slot_keypoints(st);
  rc |= dvm_keyframe_store_put(st, 3, slots, kfs);
  rc |= dvm_keyframe_store_remove(st, 1, slots);
  rc |= dvm_keyframe_store_debug_read(st, 2, back);
  rc |= dvm_fuse_targets_set_resident(ft, st, 3, t, m, forms);
  rc |= dvm_fuse_targets_last_upload_bytes(ft, bytes, bytes + 1);
  rc |= dvm_create_new_map_points_resident(np, st, cur, m, 2, nbs, m, poses, p, out);
  rc |= dvm_new_points_last_upload_bytes(np, bytes);
  dvm_keyframe_store_destroy(st);
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
    src = tmp_path / "keyframe_store_abi.c"
    src.write_text(USE % _offset_asserts())
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_layouts_are_pinned():
    for _, mirror, size in MIRRORS:
        assert C.sizeof(getattr(capi, mirror)) == size, mirror
    assert [f for f, _ in capi._FtTargetResident._fields_] == ["slot", "Tcw", "Ow"]
    assert [f for f, _ in capi._NpKeyFrameResident._fields_] == ["slot", "mp", "Tcw", "Twc", "Ow"]
    assert capi.KFS_CELL_START == 3076


def test_library_exports_the_symbols():
    lib = capi.lib()
    for s in DEVICE_SYMBOLS:
        assert hasattr(lib, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dvm_slam_amd", "lib", "libdvmslam_hip.so")], capture_output=True, text=True).stdout
    for s in DEVICE_SYMBOLS:
        assert f" T {s}\n" in out, s
    # the host library links the device library: a program that loads it reaches the new entries through it as well
    host = capi.host_lib()
    for s in DEVICE_SYMBOLS:
        assert hasattr(host, s), s


def test_create_without_a_device_names_it():
    if capi.device_count() > 0:
        return                                      # (on a GPU machine tests/test_gpu_keyframe_store.py creates stores)
    h = C.c_void_p()
    f = capi.lib().dvm_keyframe_store_create
    f.restype = C.c_int32; f.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    assert f(0, 8, 64, C.byref(h)) == -5            # DVM_ERR_NO_DEVICE
    assert not h.value
    assert f(0, 0, 64, C.byref(h)) == -1 and f(0, 8, 0, C.byref(h)) == -1 and f(0, 8, 8193, C.byref(h)) == -1   # DVM_ERR_INVALID comes first
