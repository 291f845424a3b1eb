"""The C ABI of dvm_map_store_refresh: INTEGRATION.md's "Map points refreshed on the resident stores" snippet compiles against the header,
dvm_mp_obs, dvm_mp_refresh_kf and dvm_mp_refresh keep their sizes and field offsets, the ctypes structure and the numpy dtypes of capi are
the same layout, and the library exports the entry points."""
import ctypes as C
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dvm_slam_amd", "lib")

# field -> offset (LP64), written out by hand
OBS = dict(kf=0, kp=4)
KF = dict(slot=0, flags=4, ow=8)
REFRESH = dict(n_points=0, n_kfs=4, n_obs=8, what=12, mp_slot=16, obs_off=24, obs=32, ref_obs=40, kfs=48, is_new=56, new_pos=64, best_obs_out=72,
               best_median_out=80, geometry_out=88)


def _asserts():
    s = ('static_assert(sizeof(dvm_mp_obs) == 8, "dvm_mp_obs");\nstatic_assert(sizeof(dvm_mp_refresh_kf) == 20, "dvm_mp_refresh_kf");\n'
         'static_assert(sizeof(dvm_mp_refresh) == 96, "dvm_mp_refresh");\n'
         'static_assert(DVM_MPR_KF_BAD == 1u && DVM_MPR_DESCRIPTOR == 1u && DVM_MPR_GEOMETRY == 2u, "flags");\n')
    for name, table in (("dvm_mp_obs", OBS), ("dvm_mp_refresh_kf", KF), ("dvm_mp_refresh", REFRESH)):
        s += "".join(f'static_assert(offsetof({name}, {k}) == {v}, "{k}");\n' for k, v in table.items())
    return s


def _section():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## Map points refreshed on the resident stores"):]
    return sec[:sec.index("\n## ", 4)]


def test_integration_snippet_compiles_and_layouts_are_pinned():
    blocks = re.findall(r"```cpp\n(.*?)```", _section(), re.S)
    assert len(blocks) == 1, "the section has one cpp block"
    code = blocks[0]
    for name in ("dvm_map_store_refresh", "process_new_keyframe", "create_new_map_points_end", "search_in_neighbors_end", "best_obs_out"):
        assert name in code, name
    src = '#include <cstddef>\n#include <cstdint>\n#include <vector>\n#include "dvmslam_hip.h"\n' + _asserts() + code
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "snippet.cpp")
        open(p, "w").write(src)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), p], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_section_says_what_the_host_still_does():
    sec = _section()
    for phrase in ("mDescriptor = own row [best_obs]", "UpdateNormalAndDepth", "AddObservation", "EraseObservation", "Replace"):
        assert phrase in sec, phrase


def test_python_structs_match_the_header():
    from dvm_slam_amd import capi
    assert capi.MP_OBS_DTYPE.itemsize == 8 and {k: capi.MP_OBS_DTYPE.fields[k][1] for k in OBS} == OBS
    assert capi.MP_REFRESH_KF_DTYPE.itemsize == 20 and {k: capi.MP_REFRESH_KF_DTYPE.fields[k][1] for k in KF} == KF
    assert capi.MP_REFRESH_KF_DTYPE.fields["ow"][0].shape == (3,) and capi.MP_REFRESH_KF_DTYPE.fields["flags"][0].base == "<u4"
    assert C.sizeof(capi.MpRefresh) == 96
    assert {k: getattr(capi.MpRefresh, k).offset for k in REFRESH} == REFRESH
    assert [f[0] for f in capi.MpRefresh._fields_] == list(REFRESH)
    assert (capi.MPR_KF_BAD, capi.MPR_DESCRIPTOR, capi.MPR_GEOMETRY) == (1, 1, 2)


def test_new_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, "libdvmslam_hip.so")], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in ("dvm_map_store_refresh", "dvm_map_store_last_refresh_bytes"):
        assert s in syms, s
