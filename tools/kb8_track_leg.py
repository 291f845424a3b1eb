"""Timing of one tracked frame of a fisheye agent (Frame::Frame + TrackWithMotionModel, then TrackLocalMap) on the dense bench stream:
about 700 matches in the first half, a local map of about 3 000 points (the points behind the keypoints of the three previous frames
through the KannalaBrandt8 model).  In one process, after warm-up, three forms alternate frame by frame:
  (a) kb8_chains    Tracker.track(model=kb8) + Tracker.track_local_map: the two device chains on the fisheye model
  (b) kb8_separate  the loop of separate calls a fisheye agent ran before: extraction, dvmh_search_by_projection_frames_cam,
                    dvm_pose_optimize_cam, dvm_is_in_frustum_cam, dvmh_search_by_projection_points, dvm_pose_optimize_cam, with the
                    edge gathering, the outlier drop and SearchLocalPoints' bookkeeping on the host in between
  (c) pinhole       the two chains of a pinhole agent on the same frames (map points behind the same keypoints through K)
Host to host, medians with p5 / p95 in ms, one JSON line.  --pinhole-only times (c) alone and calls nothing a build without the fisheye
chains lacks (the pinhole guard: the same script on two builds, DVM_HIP_LIB).
Usage: python tools/kb8_track_leg.py [--frames 60] [--warmup 10] [--pinhole-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dvm_slam_amd import capi, synth  # noqa: E402

P = np.array([300.0, 300.0, 320.0, 240.0, -0.027058405982580736, 0.025005319766890292, -0.02255121102967952, 0.006475379139360301], np.float32)
KC = np.array([500.0, 500.0, 320.0, 240.0], np.float32)
BOUNDS = np.array([0, 640, 0, 480], np.float32)
TCW = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)


def kb8_rays(kps):
    """KannalaBrandt8::unproject of the keypoints (camera_model.h's Newton iteration, vectorised): rays (X, Y, 1)."""
    mx = (kps["x"].astype(np.float64) - P[2]) / P[0]; my = (kps["y"].astype(np.float64) - P[3]) / P[1]
    ln = np.minimum(np.hypot(mx, my), np.pi / 2)
    th = ln.copy()
    for _ in range(10):
        t2 = th * th
        e = [P[4] * t2, P[5] * t2 ** 2, P[6] * t2 ** 3, P[7] * t2 ** 4]
        th = th - (th * (1 + e[0] + e[1] + e[2] + e[3]) - ln) / (1 + 3 * e[0] + 5 * e[1] + 7 * e[2] + 9 * e[3])
    gain = np.where(ln > 1e-8, np.tan(th) / np.maximum(ln, 1e-8), 1.0)
    return np.column_stack([mx * gain, my * gain, np.ones(len(kps))])


def pinhole_rays(kps):
    return np.column_stack([(kps["x"] - KC[2]) / KC[0], (kps["y"] - KC[3]) / KC[1], np.ones(len(kps))]).astype(np.float64)


def local_points(kps, desc, X, scale, rng):
    n = len(kps)
    pts = np.zeros(n, capi.LOCAL_POINT_DTYPE)
    pts["pos"] = X.astype(np.float32)
    d = np.linalg.norm(X, axis=1)
    pts["normal"] = (X / d[:, None]).astype(np.float32)
    pts["max_dist"] = (d * scale[kps["octave"]]).astype(np.float32)
    pts["min_dist"] = (pts["max_dist"] / scale[-1]).astype(np.float32)
    pts["desc"] = desc
    pts["n_obs"] = np.where(rng.random(n) < 0.1, 0, 2)
    return pts


def separate_frame(ext, model, img, kl, ml, mps, pts, scale, inv_s2, th_local):
    """The tracked frame of a fisheye agent over the separate calls, in the reference's order (Tracking.cc:2584-2667, 3041-3106, 2668-2740)."""
    n, kps, desc, _ = ext.extract(img)
    nm, mp, _ = capi.search_by_projection_frames_cam(kps, desc, np.full(n, -1, np.int32), TCW, model, BOUNDS, scale, kl, ml, None, mps, 15.0)
    if nm < 20:
        nm, mp, _ = capi.search_by_projection_frames_cam(kps, desc, np.full(n, -1, np.int32), TCW, model, BOUNDS, scale, kl, ml, None, mps, 30.0)
    sel = np.flatnonzero(mp >= 0)
    Xw = mps["pos"][mp[sel]].astype(np.float64); obs = np.column_stack([kps["x"][sel], kps["y"][sel]]).astype(np.float64)
    w = inv_s2[kps["octave"][sel]].astype(np.float64)
    pose_in = np.concatenate([TCW[4:7], TCW[0:4]]).astype(np.float64)
    p, o, _ = capi.pose_optimize_cam(pose_in[None], Xw[None], obs[None], w[None], [len(sel)], model)
    mp[sel[o[0][:len(sel)] != 0]] = -1
    Tcw = np.concatenate([p[0][3:7], p[0][0:3]]).astype(np.float32)
    # TrackLocalMap
    bad = pts["bad"] != 0
    mp[(mp >= 0) & bad[np.maximum(mp, 0)]] = -1
    seen = np.zeros(len(pts), bool)
    seen[mp[mp >= 0]] = True
    R, t, Ow = capi.pose_matrices(Tcw)
    F = capi.FrustumFrame()
    F.Rcw[:] = [float(v) for v in R.reshape(-1)]; F.tcw[:] = [float(v) for v in t]; F.Ow[:] = [float(v) for v in Ow]
    F.min_x, F.max_x, F.min_y, F.max_y = (float(v) for v in BOUNDS)
    F.bf, F.log_scale_factor, F.n_levels = 0.0, float(np.float32(np.log(np.float64(scale[1])))), len(scale)
    tp = capi.is_in_frustum_cam(F, model, pts["pos"], pts["normal"], pts["min_dist"], pts["max_dist"], 0.5)
    tp["in_view"][seen | bad] = 0
    tpts = np.zeros(len(pts), capi.TRACKED_POINT_DTYPE)
    for f in ("proj_x", "proj_y", "depth", "view_cos", "level"):
        tpts[f] = tp[f]
    tpts["in_view"] = tp["in_view"] != 0
    tpts["bad"] = bad
    tpts["desc"], tpts["n_obs"] = pts["desc"], pts["n_obs"]
    claimed = ((mp >= 0) & (pts["n_obs"][np.maximum(mp, 0)] > 0)).astype(np.uint8)
    nm2, mp2, _ = capi.search_by_projection_points(kps, desc, mp, claimed, BOUNDS, scale, tpts, th_local, 0.8, False, 0.0)
    sel = np.flatnonzero(mp2 >= 0)
    Xw = pts["pos"][mp2[sel]].astype(np.float64); obs = np.column_stack([kps["x"][sel], kps["y"][sel]]).astype(np.float64)
    w = inv_s2[kps["octave"][sel]].astype(np.float64)
    pose_in = np.concatenate([Tcw[4:7], Tcw[0:4]]).astype(np.float64)
    p, o, ni = capi.pose_optimize_cam(pose_in[None], Xw[None], obs[None], w[None], [len(sel)], model)
    return dict(nmatches_first=nm, mp=mp2, pose=p[0], nmatches=nm2)


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p5_ms=round(float(np.percentile(a, 5)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--th", type=float, default=1.0)
    ap.add_argument("--pinhole-only", action="store_true")
    a = ap.parse_args()
    total = a.frames + a.warmup
    stream = synth.frame_stream(total + 3)
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    rng = np.random.default_rng(1)
    extracted = [ext.extract(f) for f in stream]
    model = None if a.pinhole_only else capi.CameraModel.make(1, P)
    cases = []
    for t in range(3, total + 3):
        z = [rng.uniform(3, 9, len(extracted[f][1])) for f in (t - 3, t - 2, t - 1)]
        per = {}
        for name, rays in (("kb8", kb8_rays), ("pinhole", pinhole_rays)):
            tabs = [local_points(extracted[f][1], extracted[f][2], rays(extracted[f][1]) * z[i][:, None], scale, rng) for i, f in enumerate((t - 3, t - 2, t - 1))]
            pts = np.concatenate(tabs)
            mps = np.zeros(len(pts), capi.MAP_POINT_DTYPE)
            mps["pos"], mps["desc"], mps["n_obs"] = pts["pos"], pts["desc"], pts["n_obs"]
            per[name] = (pts, mps, np.arange(len(pts) - len(tabs[2]), len(pts), dtype=np.int32))
        cases.append((stream[t], extracted[t - 1][1], per))
    trk = capi.Tracker(ext)
    trk.reserve_local_map(max(len(c[2]["kb8"][0]) for c in cases))
    trk_p = capi.Tracker(ext)                     # the pinhole agent's tracker (an agent keeps its camera)
    trk_p.reserve_local_map(max(len(c[2]["pinhole"][0]) for c in cases))
    times = dict(kb8_chains=[], kb8_separate=[], pinhole=[])
    sizes, first_matches, matches, mismatches = [], [], [], 0
    for i, (img, kl, per) in enumerate(cases):
        if not a.pinhole_only:
            pts, mps, ml = per["kb8"]
            t0 = time.perf_counter()
            first = trk.track(img, TCW, None, BOUNDS, scale, inv_s2, kl, ml, None, mps, th=15.0, model=model)
            r = trk.track_local_map(pts, first["mp"], th=a.th) if first["tracked"] else None
            t1 = time.perf_counter()
            s = separate_frame(ext, model, img, kl, ml, mps, pts, scale, inv_s2, a.th)
            t2 = time.perf_counter()
            if r is None:
                continue
            mismatches += int(not (np.array_equal(r["mp"], s["mp"]) and np.array_equal(r["pose"], s["pose"]) and r["nmatches"] == s["nmatches"]))
        pts_p, mps_p, ml_p = per["pinhole"]
        t3 = time.perf_counter()
        first_p = trk_p.track(img, TCW, KC, BOUNDS, scale, inv_s2, kl, ml_p, None, mps_p, th=15.0)
        if first_p["tracked"]:
            trk_p.track_local_map(pts_p, first_p["mp"], th=a.th)
        t4 = time.perf_counter()
        if i >= a.warmup:
            times["pinhole"].append(t4 - t3)
            if not a.pinhole_only:
                times["kb8_chains"].append(t1 - t0); times["kb8_separate"].append(t2 - t1)
                sizes.append(len(pts)); first_matches.append(first["nmatches_search"]); matches.append(r["nmatches"])
    out = dict(leg="kb8_track", th=a.th, **{k: stats(v) for k, v in times.items() if v})
    if not a.pinhole_only:
        out.update(table_points=int(np.median(sizes)), first_half_matches_median=int(np.median(first_matches)), local_matches_median=int(np.median(matches)),
                   mismatches=mismatches)
    print(json.dumps(out))
    trk.close(); trk_p.close(); ext.close()


if __name__ == "__main__":
    main()
