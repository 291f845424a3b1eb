"""Timing of a whole tracked frame for K agents sharing one GPU (one camera tick): the batched first half (TrackerBatch.track,
dvmh_track_with_motion_model_batch) followed by the second half (Tracking::TrackLocalMap) of every agent, each agent on the dense bench
stream with a local map of ~3 000 points built as tools/track_local_map_leg.py builds one.  In one process, after warm-up, the three forms
alternate tick by tick:
  (a) batched   TrackerBatch.track + TrackerBatch.track_local_map (dvm_track_local_map_batch: one upload, one chain, one synchronisation)
  (b) singles   TrackerBatch.track + per agent a single-frame Tracker.track + Tracker.track_local_map (what a process without the batched
                second half has to do); `second_singles` is the sum of the K Tracker.track_local_map calls alone
  (c) second    TrackerBatch.track_local_map alone (the batched first half runs untimed in front of it)
Host-to-host medians and p95 in ms and frames/s, one JSON line per K.  DVM_TRACK_BATCH_TIMING=1 prints the host phases of both batched
halves (the second half's: pack + enqueue, wait, results out) on stderr.
Usage: python tools/track_tick_leg.py [--agents 8 32 64] [--ticks 30] [--warmup 5] [--th 1]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dvm_slam_amd import capi, synth  # noqa: E402
from track_local_map_leg import BOUNDS, KC, local_points  # noqa: E402


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


def build_cases(n_frames, ext, scale, rng):
    """per stream frame t >= 3: (image, LastFrame keypoints, their map points' table indices, the local map table, map points)"""
    stream = synth.frame_stream(n_frames)
    extracted = [ext.extract(f) for f in stream]
    cases = []
    for t in range(3, n_frames):
        tabs = []
        for f in (t - 3, t - 2, t - 1):
            _, k, d, _ = extracted[f]
            tabs.append(local_points(k, d, rng.uniform(3, 9, len(k)), scale, rng))
        pts = np.concatenate(tabs)
        nl = len(tabs[2])
        mps = np.zeros(len(pts), capi.MAP_POINT_DTYPE)
        mps["pos"], mps["desc"], mps["n_obs"] = pts["pos"], pts["desc"], pts["n_obs"]
        cases.append((stream[t], extracted[t - 1][1], np.arange(len(pts) - nl, len(pts), dtype=np.int32), pts, mps))
    return cases


def run(K, cases, ext1, scale, inv_s2, a):
    extB = capi.OrbExtractor(max_batch=K)
    trkB = capi.TrackerBatch(extB, K)
    trkB.reserve_local_map(K * 4096)
    singles = [capi.Tracker(ext1) for _ in range(K)]
    for s in singles:
        s.reserve_local_map(4096)
    Tcw = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
    times = dict(a_tick=[], a_second=[], b_tick=[], b_second_singles=[], c_second=[])
    mismatches, tracked, points = 0, [], []
    for tick in range(a.warmup + a.ticks):
        sel = [cases[(tick * 7 + 3 * b) % len(cases)] for b in range(K)]        # agent b's frame of this tick
        imgs = np.stack([c[0] for c in sel])
        ins = trkB.prepare([Tcw] * K, [(c[1], c[2], None, c[4]) for c in sel])
        tables = [c[3] for c in sel]
        timed = tick >= a.warmup
        # (a) both halves batched
        t0 = time.perf_counter()
        first = trkB.track(imgs, ins, KC, BOUNDS, scale, inv_s2, th=15.0)
        t1 = time.perf_counter()
        ra = trkB.track_local_map(tables, [f["mp"] for f in first], th=a.th)
        t2 = time.perf_counter()
        ra_mp = [r["mp"].copy() if r["status"] == 0 else None for r in ra]
        ra_pose = [r["pose"].copy() if r["status"] == 0 else None for r in ra]
        # (b) the batched first half, then per agent the whole frame again on a single-frame tracker
        t3 = time.perf_counter()
        first = trkB.track(imgs, ins, KC, BOUNDS, scale, inv_s2, th=15.0)
        sec = 0.0
        rb = []
        for b, c in enumerate(sel):
            f1 = singles[b].track(c[0], Tcw, KC, BOUNDS, scale, inv_s2, c[1], c[2], None, c[4], th=15.0)
            if not f1["tracked"]:
                rb.append(None)
                continue
            s0 = time.perf_counter()
            rb.append(singles[b].track_local_map(c[3], f1["mp"], th=a.th))
            sec += time.perf_counter() - s0
        t4 = time.perf_counter()
        # (c) the batched second half alone
        first = trkB.track(imgs, ins, KC, BOUNDS, scale, inv_s2, th=15.0)
        t5 = time.perf_counter()
        trkB.track_local_map(tables, [f["mp"] for f in first], th=a.th)
        t6 = time.perf_counter()
        for b in range(K):
            if (ra_mp[b] is None) != (rb[b] is None) or (rb[b] is not None and not (np.array_equal(ra_mp[b], rb[b]["mp"]) and
                                                                                     np.array_equal(ra_pose[b], rb[b]["pose"]))):
                mismatches += 1
        if timed:
            times["a_tick"].append(t2 - t0); times["a_second"].append(t2 - t1); times["b_tick"].append(t4 - t3)
            times["b_second_singles"].append(sec); times["c_second"].append(t6 - t5)
            tracked.append(sum(r["status"] == 0 for r in ra)); points.append(int(np.median([len(t) for t in tables])))
    out = dict(leg="track_tick", agents=K, th=a.th, table_points_median=int(np.median(points)), tracked_per_tick_median=float(np.median(tracked)),
               mismatches=mismatches, **{k: stats(v) for k, v in times.items()})
    out["a_frames_per_s"] = round(K / np.median(times["a_tick"]), 1)
    out["b_frames_per_s"] = round(K / np.median(times["b_tick"]), 1)
    for s in singles:
        s.close()
    trkB.close(); extB.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, nargs="+", default=[8, 32, 64])
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--th", type=float, default=1.0)
    a = ap.parse_args()
    ext1 = capi.OrbExtractor(max_batch=1)
    tab = ext1.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    cases = build_cases(40, ext1, scale, np.random.default_rng(1))
    for K in a.agents:
        print(json.dumps(run(K, cases, ext1, scale, inv_s2, a)), flush=True)
    ext1.close()


if __name__ == "__main__":
    main()
