"""Timing of 32 LocalBundleAdjustment windows on the cluster form (k_ba_window_cluster<CAM>) under the pinhole camera and under the robomaster
KannalaBrandt8 camera, against what a fisheye fleet had before: one dvm_ba_set_problem_cam + dvm_ba_optimize per window on the tile solver.

Windows: kb8_ba_leg.problem's local-BA window at 32 seeds -- 30 keyframes / 3 000 landmarks, 10 fixed, 10 iterations, the observations kept to
theta <= 60 deg, landmarks that keep at least three of them; both cameras get the same geometry, pixel noise, outliers and start; the pinhole
camera has the fisheye's fx, fy, cx, cy.  In one process, after warm-up, alternating per repeat, host to host (median and p5 - p95 in ms):
  a  the pinhole windows through dvm_ba_optimize_windows_fast
  b  the robomaster windows through dvm_ba_optimize_windows_fast_cam
  c  the robomaster windows as the loop of dvm_ba_set_problem_cam + dvm_ba_optimize on ONE handle (both calls timed: that is the loop)
Kernel time of a and b: dvm_ba_stats::kernel_us (HIP events around the launch).  b is reported as a ratio to a and to c; nothing is promised.
--lib PATH: a build of the parent commit.  Two fresh child processes, one after the other and finished before this one opens the GPU, run
leg a alone, on that library and on this tree's.  The gate is that this tree's median of a (the rotation's) lies inside the parent build's
own p5 - p95 interval ("pinhole_inside_parent_spread", host time and kernel time); the like-with-like pass -- a alone on this tree against
the same interval -- is reported beside it ("pinhole_alone_inside_parent_spread"; outside BELOW the interval is this tree being faster).
One JSON line, written to profiles/kb8_lba_fast_leg.json.
Usage: python tools/kb8_lba_fast_leg.py [--windows 32] [--repeats 40] [--warmup 3] [--lib PATH] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kb8_ba_leg as kl  # noqa: E402


def problems(K):
    out = []
    for k in range(K):
        name = f"window{k}"
        kl.PROBLEMS[name] = dict(kw=dict(kl.PROBLEMS["window"]["kw"], seed=0x1BA + k), n_fixed=10, iterations=10)
        out.append(kl.problem(name))
    return out


def window(pb, cam, with_model):
    w = dict(poses=pb["poses"], fixed=pb["fixed"], points=pb["points"], edges=pb["edges"][cam], huber_delta=kl.DELTA, iterations=pb["iterations"])
    if with_model:
        w["model"] = pb["models"][cam]
    else:
        w["intrinsics"] = [float(v) for v in pb["models"][cam].params[:4]]
    return w


def stats(v):
    a = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(a)), 4), p5=round(float(np.percentile(a, 5)), 4), p95=round(float(np.percentile(a, 95)), 4),
                min=round(float(a.min()), 4), max=round(float(a.max()), 4), n=len(a))


def measure(K, repeats, warmup, legs):
    from dvm_slam_amd import capi
    pbs = problems(K)
    batch = {}
    if "a" in legs:
        batch["a"] = capi.BaWindowBatch([window(pb, "pinhole", False) for pb in pbs])
    if "b" in legs:
        batch["b"] = capi.BaWindowBatch([window(pb, "robomaster", True) for pb in pbs])
    ba = capi.BundleAdjuster() if "c" in legs else None
    ms = {leg: [] for leg in legs}
    kus = {leg: [] for leg in legs if leg != "c"}
    iters = {leg: 0 for leg in legs}
    for it in range(warmup + repeats):
        for leg in legs:
            t0 = time.perf_counter()
            if leg == "c":
                n_it = 0
                for pb in pbs:
                    kl.set_problem(ba, pb, "robomaster")
                    n_it += ba.optimize(pb["iterations"])["iterations"]
            else:
                batch[leg].run(fast=True, collect=False)
            t1 = time.perf_counter()
            if it < warmup:
                continue
            ms[leg].append((t1 - t0) * 1e3)
            if leg != "c":
                kus[leg].append(batch[leg].stats[0].kernel_us / 1e3)
                n_it = sum(batch[leg].stats[k].iterations for k in range(K))
            iters[leg] += n_it
    out = {}
    for leg in legs:
        out[leg] = dict(host_ms=stats(ms[leg]), lm_iterations_per_s=round(iters[leg] / (float(np.sum(ms[leg])) / 1e3), 1), iterations_per_call=iters[leg] // repeats)
        if leg != "c":
            out[leg]["kernel_ms"] = stats(kus[leg])
    if ba is not None:
        ba.close()
    out["shape"] = dict(windows=K, **{k: int(np.median([pb["shape"][k] for pb in pbs])) for k in ("keyframes", "fixed", "landmarks", "edges")})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kb8_lba_fast_leg.json"))
    ap.add_argument("--pinhole-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.repeats < 40 and not a.pinhole_child:
        print("kb8_lba_fast_leg: fewer than 40 repeats: not the measurement the leg is for", file=sys.stderr)
    from dvm_slam_amd import capi
    if a.pinhole_child:      # leg a alone on another build of the library
        capi.LIB_PATH = os.path.abspath(a.lib)
        print(json.dumps(measure(a.windows, a.repeats, a.warmup, ["a"])), flush=True)
        return
    def alone(lib_path):     # leg a in a child of its own
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--pinhole-child", "--lib", lib_path, "--windows", str(a.windows), "--repeats", str(a.repeats),
                            "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"the pass on {lib_path} failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        return json.loads(r.stdout.strip().splitlines()[-1])["a"]
    parent = tree = None
    if a.lib:                # first: children of their own, finished before this process opens the GPU
        parent, tree = alone(a.lib), alone(capi.LIB_PATH)
    if capi.device_count() < 1:
        raise RuntimeError("kb8_lba_fast_leg needs an MI355X: no HIP device visible")
    m = measure(a.windows, a.repeats, a.warmup, ["a", "b", "c"])
    line = dict(leg="kb8_lba_fast", theta_max_deg=60.0, shape=m["shape"],
                a_pinhole_windows_fast=m["a"], b_robomaster_windows_fast_cam=m["b"], c_robomaster_set_problem_cam_loop=m["c"],
                b_over_a_host=round(m["b"]["host_ms"]["median"] / m["a"]["host_ms"]["median"], 3),
                b_over_a_kernel=round(m["b"]["kernel_ms"]["median"] / m["a"]["kernel_ms"]["median"], 3),
                b_over_c_host=round(m["b"]["host_ms"]["median"] / m["c"]["host_ms"]["median"], 3))
    if parent is not None:
        inside = lambda x: {k: bool(parent[k + "_ms"]["p5"] <= x[k + "_ms"]["median"] <= parent[k + "_ms"]["p95"]) for k in ("host", "kernel")}
        line["a_alone_on_parent_build"] = parent
        line["a_alone_on_this_tree"] = tree
        line["pinhole_inside_parent_spread"] = inside(m["a"])
        line["pinhole_alone_inside_parent_spread"] = inside(tree)
    else:
        line["a_alone_on_parent_build"] = "not measured (no --lib)"
    s = json.dumps(line)
    print(s, flush=True)
    if a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
