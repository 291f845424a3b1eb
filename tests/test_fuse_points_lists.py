"""dvm_slam_amd/csrc/fuse_points_lists.h (tools/check_fuse_points_lists.cpp): the host checks of dvm_fuse_targets_run[_hits]_resident and
dvm_fuse_targets_run_hits_candidates against a brute-force restatement, at n of 0, 1, 63, 64, 65 and 257, every offence planted in turn,
and the kernels' walk replayed on arrays of the reserved sizes.  The checker is a plain program with its own main, built once as it is
and once with AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuse_points_lists(tmp_path):
    src = os.path.join(ROOT, "tools", "check_fuse_points_lists.cpp")
    for tag, extra in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = tmp_path / f"check_fuse_points_lists_{tag}"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *extra, "-o", str(exe), src])
        out = subprocess.run([str(exe)], capture_output=True, text=True)
        assert out.returncode == 0, (tag, out.stdout[-3000:] + out.stderr[-3000:])
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, (tag, out.stderr[-3000:])
        assert "every verdict as the direct enumeration" in out.stdout
        assert out.stdout.count(" ok\n") == 6
