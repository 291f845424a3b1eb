"""Timing of the second half of a tracked frame (Tracking::TrackLocalMap, dvm_track_local_map) on the dense bench stream with a realistic
local map (the back-projected keypoints of the three previous frames, ~3 000 points).  In one process, after warm-up, the three forms
alternate frame by frame:
  (a) fused     Tracker.track_local_map alone (the first half runs untimed in front of it)
  (b) separate  dvm_is_in_frustum + dvmh_search_by_projection_points + dvm_pose_optimize with their host bookkeeping in between
                (SearchLocalPoints' clearing / seen marks, the TRACKED_POINT table, the edge gather, mnMatchesInliers)
  (c) frame     the whole tracked frame: Tracker.track + Tracker.track_local_map
Host-to-host medians and p95 in ms, one JSON line.  Usage: python tools/track_local_map_leg.py [--frames 60] [--warmup 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dvm_slam_amd import capi, synth  # noqa: E402

KC = np.array([500.0, 500.0, 320.0, 240.0], np.float32)
BOUNDS = np.array([0, 640, 0, 480], np.float32)


def local_points(kps, desc, z, scale, rng):
    n = len(kps)
    pts = np.zeros(n, capi.LOCAL_POINT_DTYPE)
    X = np.column_stack([(kps["x"] - KC[2]) / KC[0] * z, (kps["y"] - KC[3]) / KC[1] * z, z])
    pts["pos"] = X.astype(np.float32)
    d = np.linalg.norm(X, axis=1)
    pts["normal"] = (X / d[:, None]).astype(np.float32)
    pts["max_dist"] = (d * scale[kps["octave"]]).astype(np.float32)
    pts["min_dist"] = (pts["max_dist"] / scale[-1]).astype(np.float32)
    pts["desc"] = desc
    pts["n_obs"] = np.where(rng.random(n) < 0.1, 0, 2)
    return pts


def separate(first, pts, scale, inv_s2, th):
    """TrackLocalMap over the separate calls, in the reference's order (Tracking.cc:3041-3106, 2668-2740)."""
    n = len(pts)
    mp = np.array(first["mp"], np.int32, copy=True)
    bad = pts["bad"] != 0
    mp[(mp >= 0) & bad[np.maximum(mp, 0)]] = -1
    seen = np.zeros(n, bool)
    seen[mp[mp >= 0]] = True
    R, t, Ow = capi.pose_matrices(first["Tcw"])
    F = capi.FrustumFrame()
    F.Rcw[:] = [float(v) for v in R.reshape(-1)]; F.tcw[:] = [float(v) for v in t]; F.Ow[:] = [float(v) for v in Ow]
    F.fx, F.fy, F.cx, F.cy = (float(v) for v in KC)
    F.min_x, F.max_x, F.min_y, F.max_y = (float(v) for v in BOUNDS)
    F.bf, F.log_scale_factor, F.n_levels = 0.0, float(np.float32(np.log(np.float64(scale[1])))), len(scale)
    tp = capi.is_in_frustum(F, pts["pos"], pts["normal"], pts["min_dist"], pts["max_dist"], 0.5)
    tp["in_view"][seen | bad] = 0
    tpts = np.zeros(n, capi.TRACKED_POINT_DTYPE)
    for f in ("proj_x", "proj_y", "depth", "view_cos", "level"):
        tpts[f] = tp[f]
    tpts["in_view"] = tp["in_view"] != 0
    tpts["bad"] = bad
    tpts["desc"], tpts["n_obs"] = pts["desc"], pts["n_obs"]
    claimed = ((mp >= 0) & (pts["n_obs"][np.maximum(mp, 0)] > 0)).astype(np.uint8)
    kps = first["kps_un"]
    nm, mp2, _ = capi.search_by_projection_points(kps, first["desc"], mp, claimed, BOUNDS, scale, tpts, th, 0.8, False, 0.0)
    sel = np.flatnonzero(mp2 >= 0)
    S = max(len(sel), 1)
    Xw = np.zeros((S, 3)); obs = np.zeros((S, 2)); w = np.zeros(S)
    Xw[:len(sel)] = pts["pos"][mp2[sel]]
    obs[:len(sel), 0], obs[:len(sel), 1] = kps["x"][sel], kps["y"][sel]
    w[:len(sel)] = inv_s2[kps["octave"][sel]]
    pose_in = np.concatenate([first["Tcw"][4:7], first["Tcw"][0:4]]).astype(np.float64)
    p, o, ni = capi.pose_optimize(pose_in[None], Xw[None], obs[None], w[None], [len(sel)], KC)
    outl = o[0][:len(sel)]
    inl = int((pts["n_obs"][mp2[sel[outl == 0]]] > 0).sum())
    return dict(nmatches=nm, mp=mp2, pose=p[0], n_inliers=int(ni[0]), matches_inliers=inl)


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--th", type=float, default=1.0)     # SearchLocalPoints' th of the monocular tracker (5 after a relocalisation, 15 when lost)
    a = ap.parse_args()
    total = a.frames + a.warmup
    stream = synth.frame_stream(total + 3)
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    rng = np.random.default_rng(1)
    # per frame: the local map of its three predecessors and the last frame's points (extracted up front: the timed loop extracts only
    # inside Tracker.track)
    extracted = [ext.extract(f) for f in stream]
    cases = []
    for t in range(3, total + 3):
        tabs = []
        for f in (t - 3, t - 2, t - 1):
            _, k, d, _ = extracted[f]
            tabs.append(local_points(k, d, rng.uniform(3, 9, len(k)), scale, rng))
        pts = np.concatenate(tabs)
        nl = len(tabs[2])
        mps = np.zeros(len(pts), capi.MAP_POINT_DTYPE)
        mps["pos"], mps["desc"], mps["n_obs"] = pts["pos"], pts["desc"], pts["n_obs"]
        cases.append((stream[t], extracted[t - 1][1], np.arange(len(pts) - nl, len(pts), dtype=np.int32), pts, mps))
    trk = capi.Tracker(ext)
    trk.reserve_local_map(max(len(c[3]) for c in cases))
    Tcw = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
    times = dict(fused=[], separate=[], frame=[])
    sizes, matches, requeried, mismatches = [], [], [], 0
    for i, (img, kl, ml, pts, mps) in enumerate(cases):
        first = trk.track(img, Tcw, KC, BOUNDS, scale, inv_s2, kl, ml, None, mps, th=15.0)
        if not first["tracked"]:
            continue
        t0 = time.perf_counter()
        r = trk.track_local_map(pts, first["mp"], th=a.th)
        t1 = time.perf_counter()
        first = trk.track(img, Tcw, KC, BOUNDS, scale, inv_s2, kl, ml, None, mps, th=15.0)
        t2 = time.perf_counter()
        s = separate(first, pts, scale, inv_s2, a.th)
        t3 = time.perf_counter()
        t4 = time.perf_counter()
        first = trk.track(img, Tcw, KC, BOUNDS, scale, inv_s2, kl, ml, None, mps, th=15.0)
        trk.track_local_map(pts, first["mp"], th=a.th)
        t5 = time.perf_counter()
        mismatches += int(not (np.array_equal(r["mp"], s["mp"]) and np.array_equal(r["pose"], s["pose"]) and r["nmatches"] == s["nmatches"]))
        if i >= a.warmup:
            times["fused"].append(t1 - t0); times["separate"].append(t3 - t2); times["frame"].append(t5 - t4)
            sizes.append(len(pts)); matches.append(r["nmatches"]); requeried.append(r["n_requeried"])
    out = dict(leg="track_local_map", table_points=int(np.median(sizes)), nmatches_median=int(np.median(matches)),
               n_requeried_median=int(np.median(requeried)), th=a.th,
               mismatches=mismatches, **{k: stats(v) for k, v in times.items()})
    print(json.dumps(out))
    trk.close(); ext.close()


if __name__ == "__main__":
    main()
