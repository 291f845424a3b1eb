"""dvm_slam_amd/csrc/ba_resident_lists.h (tools/check_ba_resident_lists.cpp): a point's edges in the caller's order and the ref_edge
checks of dvm_ba_resident_optimize against a brute-force restatement, at E and L of 0, 1, 63, 64, 65 and 257.  The checker is a plain
program with its own main, built once as it is and once with AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resident_lists(tmp_path):
    src = os.path.join(ROOT, "tools", "check_ba_resident_lists.cpp")
    for tag, extra in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = tmp_path / f"check_ba_resident_lists_{tag}"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *extra, "-o", str(exe), src])
        out = subprocess.run([str(exe)], capture_output=True, text=True)
        assert out.returncode == 0, (tag, out.stdout[-3000:] + out.stderr[-3000:])
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, (tag, out.stderr[-3000:])
        assert "every list as the direct enumeration" in out.stdout
        assert out.stdout.count(" ok\n") == 31
