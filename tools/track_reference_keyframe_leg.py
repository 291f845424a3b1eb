"""Timing of Tracking::TrackReferenceKeyFrame (dvm_track_reference_keyframe) on pixel-scene frames with 1 000 features, the keyframe an
earlier frame with its back-projected map points, a synthetic vocabulary of the reference's shape (k = 10, L = 6) whose node descriptors are
the scene's own.  In one process, after warm-up, the forms alternate call by call:
  (a) chain a    Tracker.track_reference_keyframe(img=...): dvm_track_begin + the chain (the no-motion-model case)
  (b) chain b    the chain alone behind a finished (untimed) first half (the motion-model-failed case)
  (c) separate   OrbExtractor.extract + vocab_transform_host + search_by_bow_kf_frame + pose_optimize with the host bookkeeping between them
Host-to-host medians and p95 in ms, one JSON line.  Usage: python tools/track_reference_keyframe_leg.py [--calls 200] [--warmup 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dvm_slam_amd import capi, synth  # noqa: E402
import pixel_scene as ps  # noqa: E402

BOUNDS = np.array([0, 640, 0, 480], np.float32)


def tcw7f(p):
    return np.concatenate([p[3:7], p[0:3]]).astype(np.float32)


def separate(ext, voc, KFv, kf, img, pose_last, inv_s2):
    """TrackReferenceKeyFrame over the separate calls (Tracking.cc:2461-2520)."""
    n, k, d, _ = ext.extract(img)
    fv = capi.vocab_transform_host(voc, d, 4)
    F = capi.frame_view(k, d, BOUNDS, np.ones(8, np.float32))
    nm, m, _ = capi.search_by_bow_kf_frame(KFv, F, fv, 0.7, True)
    if nm < 15:
        return nm
    sel = np.flatnonzero(m >= 0)
    S = max(len(sel), 1)
    Xp = np.zeros((S, 3)); Op = np.zeros((S, 2)); Wp = np.zeros(S)
    Xp[:len(sel)] = kf["pos"][m[sel]]
    Op[:len(sel), 0], Op[:len(sel), 1] = k["x"][sel], k["y"][sel]
    Wp[:len(sel)] = inv_s2[k["octave"][sel]]
    T = np.asarray(pose_last, np.float32)
    pose_in = np.concatenate([T[4:7], T[0:4]]).astype(np.float64)
    p, o, ni = capi.pose_optimize(pose_in[None], Xp[None], Op[None], Wp[None], [len(sel)], ps.K)
    outl = o[0][:len(sel)] != 0
    return int((kf["n_obs"][m[sel][~outl]] > 0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    frames, poses = ps.render(6)
    ext = capi.OrbExtractor(nfeatures=1000, max_batch=1)
    tab = ext.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    rng = np.random.default_rng(7)
    n0, k0, d0, _ = ext.extract(frames[0])
    R, t = poses[0]
    X = (ps.backproject(k0, R, t) + rng.normal(0, 0.01, (n0, 3))).astype(np.float32)
    voc = synth.vocabulary(k=10, L=6, ragged=False, seed=5)
    voc["desc"] = d0[rng.integers(0, n0, voc["n_nodes"])]
    vocd = capi.Vocabulary(voc)
    mp = np.arange(n0, dtype=np.int32)
    kf = dict(kps=k0, desc=d0, mp=mp, pos=X, n_obs=np.where(rng.random(n0) < 0.15, 0, 2).astype(np.int32), bad=np.zeros(n0, np.uint8),
              fv=capi.vocab_transform_host(voc, d0, 4))
    KFv = capi.keyframe_view(dict(kps=k0, desc=d0, mp=mp.copy(), bad=kf["bad"], fv=kf["fv"], bounds=BOUNDS))
    trk = capi.Tracker(ext)
    trk.reserve_reference_keyframe(n0)
    mps = np.zeros(n0, capi.MAP_POINT_DTYPE)
    mps["pos"], mps["desc"], mps["n_obs"] = X, d0, kf["n_obs"]
    times = {"chain_a": [], "chain_b": [], "separate": []}
    stats = {"nmatches": [], "nmatches_map": []}
    for i in range(a.warmup + a.calls):
        f = 1 + i % 4
        img = frames[f]
        pose_last = tcw7f(ps.pose7(*poses[f - 1]))
        t0 = time.perf_counter()
        r = trk.track_reference_keyframe(vocd, kf, pose_last, img=img, K=ps.K, bounds=BOUNDS, inv_sigma2=inv_s2)
        t1 = time.perf_counter()
        trk.track(img, pose_last, ps.K, BOUNDS, scale, inv_s2, k0, mp, None, mps, th=15.0)
        t2 = time.perf_counter()
        trk.track_reference_keyframe(vocd, kf, pose_last, K=ps.K, inv_sigma2=inv_s2)
        t3 = time.perf_counter()
        separate(ext, voc, KFv, kf, img, pose_last, inv_s2)
        t4 = time.perf_counter()
        if i >= a.warmup:
            times["chain_a"].append(t1 - t0); times["chain_b"].append(t3 - t2); times["separate"].append(t4 - t3)
            stats["nmatches"].append(r["nmatches"]); stats["nmatches_map"].append(r["nmatches_map"])
    out = {k: {"median_ms": round(1e3 * float(np.median(v)), 4), "p95_ms": round(1e3 * float(np.percentile(v, 95)), 4)} for k, v in times.items()}
    out.update(calls=a.calls, features=int(n0), nmatches_median=float(np.median(stats["nmatches"])),
               nmatches_map_median=float(np.median(stats["nmatches_map"])))
    print(json.dumps(out))
    trk.close(); ext.close(); vocd.close()


if __name__ == "__main__":
    main()
