"""Timing of the first half of LocalMapping::SearchInNeighbors for one new keyframe: ORBmatcher::Fuse's search of about 900 map points
against T target keyframes of about 1 900 keypoints each (T = 30: the covisible neighbours alone; T = 120: with second and spatial
neighbours).  In one process, after warm-up, alternating per repeat:
  (a) chain   FuseTargets.set + FuseTargets.run (dvm_fuse_targets_set + dvm_fuse_targets_run): one upload of all targets, their grids in
              one launch, all searches in one launch, one synchronisation -- host->host
  (b) loop    the same work as the parent commit does it: capi.fuse (dvmh_fuse) once per target -- each call uploads the target, builds
              its grid, uploads the point table again, launches and synchronises
Both give the same rows (checked once, before timing).  Host-to-host medians and p95 in ms and their ratio; `kernels_ms` are HIP-event
times of the chain's two launches from a separate pass with the handle's profiling on (the timed pass runs with it off).  One JSON line
per T, all written to profiles/fuse_targets_leg.json.
Usage: python tools/fuse_targets_leg.py [--targets 30 120] [--repeats 100] [--warmup 10] [--out profiles/fuse_targets_leg.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dvm_slam_amd import capi  # noqa: E402
import fuse_targets_scene as fts  # noqa: E402


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


def measure(T, repeats, warmup):
    sc = fts.scene.__wrapped__(seed=7, T=T, n_cloud=900, n_keypoints=1900)
    pts, skip = sc["pts"], sc["skip"]
    n = len(pts["pos"])
    h = capi.FuseTargets()
    h.reserve(n, T, T * 1900)
    arr, keep = h.targets(sc["targets"])                           # (the loop's views are built once as well)
    views = [capi.keyframe_view(kf) for kf in sc["targets"]]
    P = capi.map_points_view(dict(pts, id=np.arange(n, dtype=np.int32), bad=1 - pts["valid"]))

    def chain():
        h.set_raw(arr, T)
        return h.run(pts, 3.0, skip, want_dist=False)[0]

    def loop():
        return np.stack([capi.fuse(views[t], P, skip[t], 3.0)[1] for t in range(T)])
    rows = chain()
    same = bool(np.array_equal(rows, loop()))
    times = dict(chain=[], loop=[])
    for it in range(warmup + repeats):
        t0 = time.perf_counter()
        chain()
        t1 = time.perf_counter()
        loop()
        t2 = time.perf_counter()
        if it >= warmup:
            times["chain"].append(t1 - t0); times["loop"].append(t2 - t1)
    h.profiling(True)
    km = []
    for _ in range(30):
        chain()
        km.append(h.last_kernel_ms())
    km = np.median(np.array(km), axis=0)
    h.close()
    c, lp = stats(times["chain"]), stats(times["loop"])
    return dict(leg="fuse_targets", targets=T, points=n, target_keypoints=1900, entries=T * n, hits=int((rows >= 0).sum()), same_as_loop=same,
                chain=c, loop=lp, loop_per_call_ms=round(lp["median_ms"] / T, 4), loop_over_chain=round(lp["median_ms"] / c["median_ms"], 2),
                kernels_ms=dict(grid_build=round(float(km[0]), 4), search=round(float(km[1]), 4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, nargs="+", default=[30, 120])
    ap.add_argument("--repeats", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_targets_leg.json"))
    a = ap.parse_args()
    lines = []
    for T in a.targets:
        lines.append(json.dumps(measure(T, a.repeats, a.warmup)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
