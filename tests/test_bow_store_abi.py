"""The C ABI of the resident place-recognition and TrackReferenceKeyFrame calls (include/dvmslam_hip.h: dvm_kf_resident,
dvm_search_by_bow_targets_resident, dvm_track_reference_keyframe_batch_resident and their counters) without a GPU: the header compiles
as C, sizeof(dvm_kf_resident) is the figure the header states and the one the Python mirror has, the built libraries export the new
symbols, and the header's upload formula stays inside the bound it promises.  The listed-once scan of dvm_keyframe_store_put
(csrc/fv_once.h) runs as a plain program of its own, once as it is and once under AddressSanitizer + UBSan."""
import ctypes as C
import os
import re
import subprocess

from dvm_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dvm_search_by_bow_targets_resident", "dvm_bow_targets_last_upload_bytes", "dvm_bow_targets_last_prologue_ms",
           "dvm_track_reference_keyframe_batch_resident", "dvm_tracker_last_refkf_upload_bytes"]

USE = r"""
#include <stddef.h>
#include "dvmslam_hip.h"
%s
int use(dvm_bow_targets* h, dvm_tracker* t, dvm_orb* o, const dvm_vocab* voc, const dvm_keyframe_store* kfs, const dvm_map_store* map,
        const int32_t* mp_slot, const dvm_track_refkf_params* ps, const dvm_track_refkf_out* outs, dvm_track_refkf_result* res,
        int32_t* idx, int32_t* nm, int64_t* bytes, float* ms) {
  dvm_kf_resident cur = {3, map, mp_slot}, tg[2] = {{4, map, mp_slot}, {5, NULL, NULL}};
  const dvm_kf_resident* frames[2] = {&cur, NULL};
  int rc = dvm_search_by_bow_targets_resident(h, kfs, &cur, 2, tg, 0.9f, 1, idx, nm);
  rc |= dvm_bow_targets_last_upload_bytes(h, bytes);
  rc |= dvm_bow_targets_last_prologue_ms(h, ms);
  rc |= dvm_track_reference_keyframe_batch_resident(t, o, voc, kfs, 2, frames, ps, outs, res, nm);
  rc |= dvm_tracker_last_refkf_upload_bytes(t, bytes);
  return rc;
}
"""


def _header():
    return open(os.path.join(ROOT, "include", "dvmslam_hip.h")).read()


def test_header_states_the_size_and_compiles_as_c(tmp_path):
    m = re.search(r"sizeof\(dvm_kf_resident\) == (\d+)", _header())
    assert m, "the header states sizeof(dvm_kf_resident) as the other structs do"
    size = int(m.group(1))
    S = capi.KfResident
    asserts = [f"_Static_assert(sizeof(dvm_kf_resident) == {size}, \"dvm_kf_resident size as the header states it\");",
               f"_Static_assert(sizeof(dvm_kf_resident) == {C.sizeof(S)}, \"dvm_kf_resident against the Python mirror\");"]
    asserts += [f"_Static_assert(offsetof(dvm_kf_resident, {f}) == {getattr(S, f).offset}, \"dvm_kf_resident.{f}\");" for f, _ in S._fields_]
    src = tmp_path / "bow_store_abi.c"
    src.write_text(USE % "\n".join(asserts))
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ctypes_structs_match():
    assert C.sizeof(capi.KfResident) == 24
    assert [f for f, _ in capi.KfResident._fields_] == ["slot", "points", "mp_slot"]
    assert (capi.KfResident.slot.offset, capi.KfResident.points.offset, capi.KfResident.mp_slot.offset) == (0, 8, 16)
    api = capi._TRACK_API
    assert len(api["dvm_track_reference_keyframe_batch_resident"]) == len(api["dvm_track_reference_keyframe_batch"]) + 1
    assert len(api["dvm_tracker_last_refkf_upload_bytes"]) == 2
    for name in ("search_resident", "prepare_resident", "last_upload_bytes", "last_prologue_ms"):
        assert callable(getattr(capi.BowTargets, name)), name
    assert callable(capi.TrackerBatch.track_reference_keyframe_resident) and callable(capi.Tracker.track_reference_keyframe_resident)


def test_library_exports_the_symbols():
    lib = capi.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dvm_slam_amd", "lib", "libdvmslam_hip.so")], capture_output=True, text=True).stdout
    for s in SYMBOLS:
        assert f" T {s}\n" in out, s
    host = capi.host_lib()
    for s in SYMBOLS:
        assert hasattr(host, s), s


def test_upload_formula_keeps_the_headers_bound():
    """exactly 64 * ceil(56 (T + 1) / 64) + 64 * ceil(32 (T + 1) / 64) + sum of 64 * ceil(4 n / 64): at most 4 B per keypoint, each list
    rounded up to 64 B, plus 256 B per keyframe -- at T = 0 (one keyframe) as at 65 535 targets"""
    txt = " ".join(_header().split())
    assert "64 * ceil(56 * (T + 1) / 64) + 64 * ceil(32 * (T + 1) / 64) + sum over cur and the T targets of 64 * ceil(4 * n / 64)" in txt
    r64 = lambda b: (b + 63) // 64 * 64  # noqa: E731
    for T in (0, 1, 2, 7, 11, 33, 66, 65535):
        assert r64(56 * (T + 1)) + r64(32 * (T + 1)) <= 256 * (T + 1), T


def test_listed_once_scan(tmp_path):
    src = os.path.join(ROOT, "tools", "check_fv_once.cpp")
    for tag, extra in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = tmp_path / f"check_fv_once_{tag}"
        subprocess.check_call(["g++", "-std=c++17", *extra, "-Wall", "-Werror", "-o", str(exe), src])
        out = subprocess.run([str(exe)], capture_output=True, text=True)
        assert out.returncode == 0, (tag, out.stdout[-3000:] + out.stderr[-3000:])
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, (tag, out.stderr[-3000:])
        assert "fv_first_repeat agrees on" in out.stdout
