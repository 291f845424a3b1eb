"""dvm_slam_amd/csrc/update_local_map_lists.h (tools/check_update_local_map_lists.cpp): the host checks of dvm_update_local_map_keyframes and
_points against a brute-force restatement, at frames of 0, 1, 63, 64, 65, 257 and 1 025 keypoints, every offence planted in turn, and the
kernels' walk replayed on arrays of the reserved sizes.  The checker is a plain program with its own main, built once as it is and once
with AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_update_local_map_lists(tmp_path):
    src = os.path.join(ROOT, "tools", "check_update_local_map_lists.cpp")
    for tag, extra in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = tmp_path / f"check_update_local_map_lists_{tag}"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *extra, "-o", str(exe), src])
        out = subprocess.run([str(exe)], capture_output=True, text=True)
        assert out.returncode == 0, (tag, out.stdout[-3000:] + out.stderr[-3000:])
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, (tag, out.stderr[-3000:])
        assert "every verdict as the direct enumeration" in out.stdout
        assert out.stdout.count(" ok\n") == 7
