"""Timing of PoseOptimization for one frame of 720 matches (the README's dense stream) through dvm_pose_optimize_cam with the pinhole model
and with the robomaster KannalaBrandt8 model: what the fisheye residual (a float atan2f, a square root, two divisions) and Jacobian
(a double atan2, the polynomial and its derivative, five divisions) cost inside k_pose_optimize.

The same 720 points in the camera frame (theta up to 60 deg, so that both cameras see them), observed through each camera with the same
pixel noise and the same planted outliers, from the same start pose.  In one process, after warm-up, alternating per repeat:
  host->host   capi.pose_optimize_cam(...) around the call (it ends in the stream's synchronisation): median and p95 in ms
Kernel time comes from a run of its own: this script starts itself once under `rocprofv3 --kernel-trace --output-format csv` (a fresh
child process, before this process opens the GPU) with --kernel-pass, which only calls each model warmup + repeats times, and takes the
median and p95 of the two kernels' durations (end - start of each dispatch, the warm-up dispatches left out) from the kernel trace.
Without rocprofv3, kernel_us is null ("not measured") and the reason goes to stderr.  One JSON line, written to profiles/kb8_pose_leg.json.
Usage: python tools/kb8_pose_leg.py [--repeats 200] [--warmup 20] [--out profiles/kb8_pose_leg.json]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_MATCHES = 720
PIN = (520.0, 520.0, 480.0, 270.0)


def _rot(axis, angle):
    ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _pose(R, t):
    """(t, q = (x, y, z, w)) of a rotation with positive trace."""
    w = 0.5 * np.sqrt(1.0 + np.trace(R))
    return np.r_[t, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w]


def scenes():
    """{name: (model, poses, Xw, obs, w, n)} for the pinhole and the robomaster camera: same points, noise, outliers and start."""
    from dvm_slam_amd import capi
    rng = np.random.default_rng(720)
    R = _rot(rng.normal(size=3), 0.3); t = rng.uniform(-1.0, 1.0, 3)
    th = np.deg2rad(60.0) * np.sqrt(rng.uniform(1e-4, 1.0, N_MATCHES)); psi = rng.uniform(-np.pi, np.pi, N_MATCHES)
    d = 1.0 / rng.uniform(1.0 / 40.0, 1.0 / 4.0, N_MATCHES)
    Xc = np.column_stack([d * np.sin(th) * np.cos(psi), d * np.sin(th) * np.sin(psi), d * np.cos(th)])
    Xw = np.ascontiguousarray((Xc - t) @ R)
    noise = rng.normal(0.0, 0.7, (N_MATCHES, 2))
    bad = rng.random(N_MATCHES) < 0.1
    noise[bad] += rng.choice([-1.0, 1.0], size=(int(bad.sum()), 2)) * 35.0
    w = 1.2 ** (-2.0 * rng.integers(0, 8, N_MATCHES))
    dR = _rot(rng.normal(size=3), 0.005)                       # the start: the true pose turned by 0.005 rad and moved by 0.02
    pose0 = _pose(dR @ R, dR @ t + rng.normal(0.0, 0.02, 3))
    n = np.array([N_MATCHES], np.int32)
    out = {}
    for name, model in (("pinhole", capi.CameraModel.pinhole(*PIN)), ("robomaster", capi.CameraModel.robomaster())):
        out[name] = (model, pose0[None], Xw[None], np.ascontiguousarray(model.project(Xc) + noise)[None], w[None], n)
    return out, int(bad.sum())


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


def kernel_pass(repeats, warmup):
    from dvm_slam_amd import capi
    sc, _ = scenes()
    for _ in range(warmup + repeats):
        for name in sc:
            m, *a = sc[name]
            capi.pose_optimize_cam(*a, m)


def kernel_times(repeats, warmup):
    """{name: median / p95 kernel time in us over the timed dispatches} from a rocprofv3 kernel trace of --kernel-pass; None where it cannot be taken."""
    prof = shutil.which("rocprofv3") or next((c for c in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3"),) if os.path.exists(c)), None)
    if prof is None:
        print("kb8_pose_leg: no rocprofv3: kernel time not measured", file=sys.stderr)
        return None
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", td, "--", sys.executable, os.path.abspath(__file__), "--kernel-pass",
                            "--repeats", str(repeats), "--warmup", str(warmup)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("kernel pass failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        dur = {"pinhole": [], "robomaster": []}
        for path in glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                row = {k.lower(): v for k, v in row.items()}
                name = row.get("kernel_name", "")
                if "k_pose_optimize" in name:
                    dur["robomaster" if "k_pose_optimize_kb8" in name else "pinhole"].append((int(row["start_timestamp"]), int(row["end_timestamp"])))
        out = {}
        for name, v in dur.items():
            us = np.array([(e - b) / 1e3 for b, e in sorted(v)][warmup:])
            if len(us):
                out[name] = dict(median_us=round(float(np.median(us)), 2), p95_us=round(float(np.percentile(us, 95)), 2), min_us=round(float(us.min()), 2), n=len(us))
        if len(out) < 2:
            print("kb8_pose_leg: the profiler's kernel trace does not name both kernels; files:",
                  [os.path.relpath(f, td) for f in glob.glob(os.path.join(td, "**", "*"), recursive=True)], r.stderr[-1500:], file=sys.stderr)
            return None
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kb8_pose_leg.json"))
    ap.add_argument("--kernel-pass", action="store_true")
    a = ap.parse_args()
    if a.kernel_pass:
        kernel_pass(a.repeats, a.warmup)
        return
    kern = kernel_times(a.repeats, a.warmup)        # first: a child of its own, finished before this process opens the GPU
    from dvm_slam_amd import capi
    if capi.device_count() < 1:
        raise RuntimeError("kb8_pose_leg needs an MI355X: no HIP device visible")
    sc, n_bad = scenes()
    res = {name: capi.pose_optimize_cam(*sc[name][1:], sc[name][0]) for name in sc}
    times = {name: [] for name in sc}
    for it in range(a.warmup + a.repeats):
        for name in sc:
            m, *args = sc[name]
            t0 = time.perf_counter()
            capi.pose_optimize_cam(*args, m)
            t1 = time.perf_counter()
            if it >= a.warmup:
                times[name].append(t1 - t0)
    line = dict(leg="kb8_pose", matches=N_MATCHES, planted_outliers=n_bad,
                inliers={name: int(res[name][2][0]) for name in sc},
                host_to_host={name: stats(times[name]) for name in sc},
                kernel_us=kern,
                kb8_over_pinhole=dict(host_to_host=round(float(np.median(times["robomaster"]) / np.median(times["pinhole"])), 3),
                                      kernel=None if not kern else round(kern["robomaster"]["median_us"] / kern["pinhole"]["median_us"], 3)))
    s = json.dumps(line)
    print(s, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
