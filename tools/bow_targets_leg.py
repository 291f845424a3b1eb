"""Timing of the BoW searches of LoopClosing::DetectCommonRegionsFromBoW for one keyframe: ORBmatcher::SearchByBoW(mpCurrentKF, KF) against
T keyframes of about 1 150 keypoints each (T = 11: one candidate with its ten covisibles; 33: a candidate list; 66: loop and merge lists).
In one process, after warm-up, alternating per repeat:
  (a) chain   capi.search_by_bow_targets (dvmh_search_by_bow_targets over dvm_search_by_bow_targets): one packed upload of the current
              keyframe and all targets, two launches, one synchronisation -- host->host
  (b) loop    the same work as the parent commit does it: capi.search_by_bow_kf_kf (dvmh_search_by_bow_kf_kf) once per target -- each
              call builds the query lists on the host, uploads, launches dvm_match_lists, synchronises and replays the claims
Both give the same rows (checked once, before timing).  Host-to-host medians and p95 in ms and their ratio; `kernels_ms` are HIP-event
times of the chain's two launches (dvm_bow_targets_last_kernel_ms) from a separate pass on a handle of its own with profiling on (the
timed pass runs without it).  One JSON line per T, all written to profiles/bow_targets_leg.json.
Usage: python tools/bow_targets_leg.py [--targets 11 33 66] [--repeats 100] [--warmup 10] [--out profiles/bow_targets_leg.json]"""
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
import bow_targets_scene as bts  # noqa: E402


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


def measure(T, repeats, warmup):
    sc = bts.scene.__wrapped__(seed=2, T=T, n_pts=1000, n_clutter=250, n_nodes=300, dup=0.1, heavy_frac=0.1)
    cur, tg = sc["cur"], sc["targets"]
    KF1 = capi.keyframe_view(cur)
    views = [capi.keyframe_view(k) for k in tg]                    # (both sides' views are built once)

    def chain():
        return capi.search_by_bow_targets(KF1, views, 0.9, True, want_idx2=False)

    def loop():
        return [capi.search_by_bow_kf_kf(KF1, v, 0.9, True)[:2] for v in views]
    total, m12, _, nm = chain()
    rows = loop()
    same = bool(all(rows[t][0] == nm[t] and np.array_equal(rows[t][1], m12[t]) for t in range(T)))
    times = dict(chain=[], loop=[])
    for it in range(warmup + repeats):
        t0 = time.perf_counter()
        chain()
        t1 = time.perf_counter()
        loop()
        t2 = time.perf_counter()
        if it >= warmup:
            times["chain"].append(t1 - t0); times["loop"].append(t2 - t1)
    h = capi.BowTargets()
    h.reserve(len(cur["desc"]), T, sum(len(k["desc"]) for k in tg))
    h.profiling(True)
    run = h.prepare(cur, tg, 0.9, True)
    km = []
    for _ in range(30):
        run()
        km.append(h.last_kernel_ms())
    km = np.median(np.array(km), axis=0)
    h.close()
    c, lp = stats(times["chain"]), stats(times["loop"])
    return dict(leg="bow_targets", targets=T, cur_keypoints=len(cur["desc"]), target_keypoints=int(np.mean([len(k["desc"]) for k in tg])),
                cur_nodes=len(cur["fv"]["fv_nodes"]), matches=int(total), same_as_loop=same, chain=c, loop=lp,
                loop_per_call_ms=round(lp["median_ms"] / T, 4), loop_over_chain=round(lp["median_ms"] / c["median_ms"], 2),
                kernels_ms=dict(search=round(float(km[0]), 4), settle=round(float(km[1]), 4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, nargs="+", default=[11, 33, 66])
    ap.add_argument("--repeats", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bow_targets_leg.json"))
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
