"""The C ABI of the Fuse runs on map-store slots (include/dvmslam_hip.h: dvm_ft_points_resident, dvm_ft_candidates) without a GPU: the
header compiles as C, the struct sizes and offsets are the ones the Python mirrors use, and the built libraries export the new symbols."""
import ctypes as C
import os
import subprocess

from dvm_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dvm_fuse_targets_run_resident", "dvm_fuse_targets_run_hits_resident", "dvm_fuse_targets_reserve_candidates",
           "dvm_fuse_targets_run_hits_candidates"]
MIRRORS = (("dvm_ft_points_resident", "_FtPointsResident", 32), ("dvm_ft_candidates", "_FtCandidates", 48))

USE = r"""
#include <stddef.h>
#include "dvmslam_hip.h"
%s
int use(dvm_fuse_targets* ft, const dvm_ft_points_resident* P, const dvm_ft_candidates* cand, const unsigned char* skip, int32_t* i32, dvm_ft_hit* hits) {
  int rc = dvm_fuse_targets_run_resident(ft, P, skip, 3.0f, i32, i32);
  rc |= dvm_fuse_targets_run_hits_resident(ft, P, skip, 3.0f, i32, hits, 8, i32);
  rc |= dvm_fuse_targets_reserve_candidates(ft, 57000, 100000);
  rc |= dvm_fuse_targets_run_hits_candidates(ft, cand, 3.0f, i32, 8, i32, i32, hits, 8, i32);
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
    src = tmp_path / "fuse_points_abi.c"
    src.write_text(USE % _offset_asserts())
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_layouts_are_pinned():
    for _, mirror, size in MIRRORS:
        assert C.sizeof(getattr(capi, mirror)) == size, mirror
    assert [f for f, _ in capi._FtPointsResident._fields_] == ["points", "n", "slot", "valid"]
    assert [f for f, _ in capi._FtCandidates._fields_] == ["points", "n_lists", "mp_slot", "n", "exclude", "n_exclude"]


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
    for name in ("run_resident", "run_hits_resident", "reserve_candidates", "run_hits_candidates"):
        assert callable(getattr(capi.FuseTargets, name))
