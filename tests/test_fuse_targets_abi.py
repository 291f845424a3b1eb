"""The C ABI of the Fuse-targets chain (include/dvmslam_hip.h: dvm_ft_target, dvm_ft_points, dvm_fuse_targets_*; include/dvmslam_host.h:
dvmh_fuse_targets) without a GPU: both headers compile as C, the struct sizes are the ones the header states and the Python side
(capi._FtTarget, capi._FtPoints) uses, and the built libraries export the new symbols."""
import ctypes as C
import os
import subprocess

from dvm_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SYMBOLS = ["dvm_fuse_targets_create", "dvm_fuse_targets_destroy", "dvm_fuse_targets_reserve", "dvm_fuse_targets_set", "dvm_fuse_targets_run",
                  "dvm_fuse_targets_profiling", "dvm_fuse_targets_last_kernel_ms"]

USE = r"""
#include <stddef.h>
#include "dvmslam_host.h"
_Static_assert(sizeof(dvm_ft_target) == 120, "dvm_ft_target size");
_Static_assert(sizeof(dvm_ft_points) == 56, "dvm_ft_points size");
%s
int use(dvm_fuse_targets* h, const dvm_ft_target* t, const dvm_ft_points* p, const unsigned char* skip, int* idx, int* dist, float* ms,
        const dvmh_keyframe_view* kfs, const dvmh_map_points_view* P) {
  int rc = dvm_fuse_targets_create(0, &h);
  rc |= dvm_fuse_targets_reserve(h, 900, 140, 140 * 1900);
  rc |= dvm_fuse_targets_set(h, 140, t);
  rc |= dvm_fuse_targets_run(h, p, skip, 3.0f, idx, dist);
  rc |= dvm_fuse_targets_profiling(h, 1);
  rc |= dvm_fuse_targets_last_kernel_ms(h, ms);
  dvm_fuse_targets_destroy(h);
  return rc | dvmh_fuse_targets(0, 140, kfs, P, skip, 3.0f, idx);
}
"""


def _offset_asserts():
    out = []
    for name, S in (("dvm_ft_target", capi._FtTarget), ("dvm_ft_points", capi._FtPoints)):
        out.append(f"_Static_assert(sizeof({name}) == {C.sizeof(S)}, \"{name} against the Python mirror\");")
        for f, _ in S._fields_:
            out.append(f"_Static_assert(offsetof({name}, {f}) == {getattr(S, f).offset}, \"{name}.{f}\");")
    return "\n".join(out)


def test_headers_compile_as_c_with_the_stated_layouts(tmp_path):
    src = tmp_path / "fuse_targets_abi.c"
    src.write_text(USE % _offset_asserts())
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_layouts_are_pinned():
    assert C.sizeof(capi._FtTarget) == 120 and C.sizeof(capi._FtPoints) == 56
    assert [f for f, _ in capi._FtPoints._fields_] == ["n", "pos", "normal", "min_dist", "max_dist", "desc", "valid"]


def test_libraries_export_the_symbols():
    lib, host = capi.lib(), capi.host_lib()
    for s in DEVICE_SYMBOLS:
        assert hasattr(lib, s), s
    assert hasattr(host, "dvmh_fuse_targets")
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dvm_slam_amd", "lib", "libdvmslam_hip.so")], capture_output=True, text=True).stdout
    for s in DEVICE_SYMBOLS:
        assert f" T {s}\n" in out, s
