"""Timing of bundle adjustment on the general solver (dvm_ba_set_problem / dvm_ba_set_problem_cam + dvm_ba_optimize) under the pinhole model
and under the robomaster KannalaBrandt8 model: what the fisheye residual (a float atan2f, a square root, two divisions) and Jacobian (a
double atan2, the polynomial and its derivative, five divisions) cost inside k_edge_eval, and what is left of that in a whole optimize().

Two problems, each with the geometry of synth.ba_problem kept to the observations at theta <= 60 deg (so that both cameras see them) and
the landmarks that keep at least three of them: one local-BA window (30 keyframes / 3 000 landmarks, 10 fixed, 10 iterations) and the
500-keyframe bench map (20 000 landmarks, 5 iterations).  Both cameras get the same geometry, pixel noise, outliers and start; the
pinhole camera has the fisheye's fx, fy, cx, cy.  In one process, after warm-up, alternating per repeat:
  host->host   around dvm_ba_optimize (dvm_ba_set_problem[_cam] before it, untimed, puts the start back): median and p95 in ms, and LM
               iterations per second of optimize() time
The pinhole rows go through dvm_ba_set_problem only, so --pinhole-only runs on a build that has no dvm_ba_set_problem_cam (--lib: another
build of libdvmslam_hip.so, for the A/B of the pinhole rows against the parent commit).
Kernel time comes from runs of their own: this script starts itself once per problem under `rocprofv3 --kernel-trace --output-format csv`
(a fresh child process, before this process opens the GPU) with --kernel-pass, and takes the median duration of the k_edge_eval dispatches
per instantiation from the kernel trace.  Without rocprofv3, kernel_us is null ("not measured") and the reason goes to stderr.
One JSON line, written to profiles/kb8_ba_leg.json.
Usage: python tools/kb8_ba_leg.py [--repeats-window 40] [--repeats-map 10] [--warmup 3] [--pinhole-only] [--lib PATH] [--no-kernel-trace] [--out FILE]"""
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

THETA_MAX = np.deg2rad(60.0)
PROBLEMS = {"window": dict(kw=dict(n_kf=30, n_pts=3000, k_obs=5, seed=0x1BA, radius=12.0), n_fixed=10, iterations=10),
            "map500": dict(kw=dict(), n_fixed=1, iterations=5)}


def _quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def problem(name):
    """dict(poses, fixed, points, iterations, edges = {camera: dvm_ba_edge records}, models = {camera: CameraModel}) of one problem."""
    from dvm_slam_amd import capi, synth
    spec = PROBLEMS[name]
    pr = synth.ba_problem(**spec["kw"])
    ep, el = pr["edge_pose"].astype(np.int64), pr["edge_point"].astype(np.int64)
    R = np.stack([_quat_to_R(T[3:]) for T in pr["poses_gt"]])
    Xc = np.einsum("nij,nj->ni", R[ep], pr["points_gt"][el]) + pr["poses_gt"][ep, :3]
    keep = (np.arctan2(np.hypot(Xc[:, 0], Xc[:, 1]), Xc[:, 2]) <= THETA_MAX)
    n_obs = np.bincount(el[keep], minlength=len(pr["points"]))
    keep &= n_obs[el] >= 3
    lm = np.flatnonzero(np.bincount(el[keep], minlength=len(pr["points"])) > 0)
    remap = np.full(len(pr["points"]), -1, np.int64); remap[lm] = np.arange(len(lm))
    ep, el, Xc, info = ep[keep], remap[el[keep]], Xc[keep], pr["inv_sigma2"][keep]
    rng = np.random.default_rng(len(ep))
    noise = rng.normal(0.0, 0.7, (len(ep), 2))
    bad = rng.random(len(ep)) < 0.05
    noise[bad] += rng.choice([-1.0, 1.0], size=(int(bad.sum()), 2)) * 35.0
    fish = capi.CameraModel.robomaster()
    models = {"pinhole": capi.CameraModel.pinhole(*[float(v) for v in fish.params[:4]]), "robomaster": fish}
    fixed = np.zeros(len(pr["poses"]), np.uint8); fixed[:spec["n_fixed"]] = 1
    poses = pr["poses"].copy(); poses[:spec["n_fixed"]] = pr["poses_gt"][:spec["n_fixed"]]
    edges = {cam: capi.make_edges(ep.astype(np.int32), el.astype(np.int32), m.project(Xc) + noise, info) for cam, m in models.items()}
    return dict(poses=poses, fixed=fixed, points=np.ascontiguousarray(pr["points"][lm]), iterations=spec["iterations"], edges=edges, models=models,
                shape=dict(keyframes=len(poses), fixed=int(fixed.sum()), landmarks=len(lm), edges=len(ep), planted_outliers=int(bad.sum())))


DELTA = float(np.sqrt(5.991))


def set_problem(ba, pb, cam):
    if cam == "pinhole":     # the entry every build has
        ba.set_problem(pb["poses"], pb["fixed"], pb["points"], pb["edges"][cam], [float(v) for v in pb["models"][cam].params[:4]], DELTA)
    else:
        ba.set_problem_cam(pb["poses"], pb["fixed"], pb["points"], pb["edges"][cam], pb["models"][cam], DELTA)


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), min_ms=round(float(a.min()), 4),
                max_ms=round(float(a.max()), 4), n=len(a))


def run(name, cams, repeats, warmup):
    """{camera: host->host statistics of optimize()} of one problem, the cameras alternating per repeat."""
    from dvm_slam_amd import capi
    pb = problem(name)
    ba = {cam: capi.BundleAdjuster() for cam in cams}
    times, iters, trials, last = {c: [] for c in cams}, {c: 0 for c in cams}, {c: None for c in cams}, {}
    for it in range(warmup + repeats):
        for cam in cams:
            set_problem(ba[cam], pb, cam)
            t0 = time.perf_counter()
            st = ba[cam].optimize(pb["iterations"])
            t1 = time.perf_counter()
            if it >= warmup:
                times[cam].append(t1 - t0); iters[cam] += st["iterations"]
            trials[cam] = list(st["trials"]); last[cam] = st
    out = dict(shape=pb["shape"], iterations_asked=pb["iterations"])
    for cam in cams:
        out[cam] = dict(stats(times[cam]), lm_iterations_per_s=round(iters[cam] / float(np.sum(times[cam])), 1), trials=trials[cam],
                        chi2_initial=last[cam]["chi2_initial"], chi2_final=last[cam]["chi2_final"])
        ba[cam].close()
    return out


def kernel_pass(name, cams, repeats, warmup):
    from dvm_slam_amd import capi
    pb = problem(name)
    ba = capi.BundleAdjuster()
    for _ in range(warmup + repeats):
        for cam in cams:
            set_problem(ba, pb, cam)
            ba.optimize(pb["iterations"])
    ba.close()


def kernel_times(name, cams, repeats, warmup, extra):
    """{camera: {"jac": median us of k_edge_eval<true>, "chi2": of <false>, n...}} from a rocprofv3 kernel trace; None where it cannot be taken."""
    prof = shutil.which("rocprofv3") or next((c for c in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3"),) if os.path.exists(c)), None)
    if prof is None:
        print("kb8_ba_leg: no rocprofv3: kernel time not measured", file=sys.stderr)
        return None
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", td, "--", sys.executable, os.path.abspath(__file__), "--kernel-pass", name,
                            "--repeats-window", str(repeats), "--repeats-map", str(repeats), "--warmup", str(warmup)] + extra,
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("kernel pass failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        dur = {}
        for path in glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                row = {k.lower(): v for k, v in row.items()}
                kn = row.get("kernel_name", "")
                if "k_edge_eval" in kn:
                    key = ("robomaster" if "KB8" in kn else "pinhole", "jac" if "<true" in kn else "chi2")
                    dur.setdefault(key, []).append((int(row["end_timestamp"]) - int(row["start_timestamp"])) / 1e3)
        if not dur:
            print("kb8_ba_leg: the profiler's kernel trace names no k_edge_eval; files:",
                  [os.path.relpath(f, td) for f in glob.glob(os.path.join(td, "**", "*"), recursive=True)], r.stderr[-1500:], file=sys.stderr)
            return None
        out = {}
        for (cam, kind), v in sorted(dur.items()):
            out.setdefault(cam, {})[kind] = dict(median_us=round(float(np.median(v)), 2), p95_us=round(float(np.percentile(v, 95)), 2), n=len(v))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats-window", type=int, default=40)
    ap.add_argument("--repeats-map", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pinhole-only", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--no-kernel-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kb8_ba_leg.json"))
    ap.add_argument("--kernel-pass", default=None)
    a = ap.parse_args()
    from dvm_slam_amd import capi
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    cams = ["pinhole"] if a.pinhole_only else ["pinhole", "robomaster"]
    reps = {"window": a.repeats_window, "map500": a.repeats_map}
    if a.kernel_pass:
        kernel_pass(a.kernel_pass, cams, reps[a.kernel_pass], a.warmup)
        return
    extra = (["--pinhole-only"] if a.pinhole_only else []) + (["--lib", a.lib] if a.lib else [])
    # first: children of their own, finished before this process opens the GPU
    kern = None if a.no_kernel_trace else {name: kernel_times(name, cams, max(2, reps[name] // 4), 1, extra) for name in PROBLEMS}
    if capi.device_count() < 1:
        raise RuntimeError("kb8_ba_leg needs an MI355X: no HIP device visible")
    line = dict(leg="kb8_ba", lib=a.lib or "this tree", theta_max_deg=60.0)
    for name in PROBLEMS:
        line[name] = run(name, cams, reps[name], a.warmup)
        line[name]["k_edge_eval_us"] = kern[name] if kern else None
        if not a.pinhole_only:
            line[name]["kb8_over_pinhole"] = round(line[name]["robomaster"]["median_ms"] / line[name]["pinhole"]["median_ms"], 3)
    s = json.dumps(line)
    print(s, flush=True)
    if a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
