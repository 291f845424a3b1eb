"""dvm_slam_amd/csrc/kf_store_layout.h (tools/check_kf_store_layout.cpp): over slot_keypoints in {1, 63, 64, 65, 1 024, 1 900, 8 192} a
slot's arrays are 64-byte aligned, pairwise disjoint, inside the slot stride and large enough for n = fv_n = slot_keypoints and 64
levels.  The checker is a plain program with its own main, built once as it is and once with AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run_tool(tmp_path, name, flags):
    """tools/<name>.cpp as a plain program and once more with AddressSanitizer + UBSan (its own main, nothing preloaded): both runs clean"""
    src = os.path.join(ROOT, "tools", name + ".cpp")
    outs = []
    for tag, extra in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = tmp_path / f"{name}_{tag}"
        subprocess.check_call(["g++", "-std=c++17", *extra, *flags, "-o", str(exe), src])
        out = subprocess.run([str(exe)], capture_output=True, text=True)
        assert out.returncode == 0, (tag, out.stdout[-3000:] + out.stderr[-3000:])
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, (tag, out.stderr[-3000:])
        outs.append(out.stdout)
    return outs


def test_keyframe_store_slot_layout(tmp_path):
    for out in _build_and_run_tool(tmp_path, "check_kf_store_layout", ["-Wall", "-Werror"]):
        assert "every slot layout aligned, disjoint and large enough" in out
        assert out.count("slot_keypoints") == 7
