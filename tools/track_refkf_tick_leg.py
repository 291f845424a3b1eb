"""Timing of the reference-keyframe fallback in a tick of K agents sharing one GPU: pixel-scene frames with 1 000 features, each agent's
keyframe an earlier frame with its back-projected map points, a synthetic vocabulary of the reference's shape (k = 10, L = 6) whose node
descriptors are the scene's own.  A share of the agents has no motion model (Nl = 0 to the batched first half, which then reports
DVM_TRACK_FEW_MATCHES); the others are tracked by theirs.  In one process, after warm-up, per tick:
  (a) fallback  TrackerBatch.track_reference_keyframe for the agents without a motion model (dvm_track_reference_keyframe_batch), host->host
  (b) tick      the whole mixed tick: the batched first half, the fallback, the batched second half (dvm_track_local_map_batch)
  (c) singles   what is available without the batched fallback: one single-tracker form (a) call (dvm_track_begin + the chain) per such agent
Host-to-host medians and p95 in ms, one JSON line per (K, share); `mismatches` counts fallback frames whose pose or map points differ from
the single call's.  DVM_TRACK_BATCH_TIMING=1 prints the batched calls' host phases on stderr.
Usage: python tools/track_refkf_tick_leg.py [--agents 8 32] [--shares 0.125 0.5 1] [--ticks 300] [--warmup 20]"""
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


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


def world():
    frames, poses = ps.render(6)
    ext = capi.OrbExtractor(nfeatures=1000, max_batch=1)
    tab = ext.tables()
    rng = np.random.default_rng(7)
    n0, k0, d0, _ = ext.extract(frames[0])
    R, t = poses[0]
    X = (ps.backproject(k0, R, t) + rng.normal(0, 0.01, (n0, 3))).astype(np.float32)
    voc = synth.vocabulary(k=10, L=6, ragged=False, seed=5)
    voc["desc"] = d0[rng.integers(0, n0, voc["n_nodes"])]
    n_obs = np.where(rng.random(n0) < 0.15, 0, 2).astype(np.int32)
    mp = np.arange(n0, dtype=np.int32)
    kf = dict(kps=k0, desc=d0, mp=mp, pos=X, n_obs=n_obs, bad=np.zeros(n0, np.uint8), fv=capi.vocab_transform_host(voc, d0, 4))
    mps = np.zeros(n0, capi.MAP_POINT_DTYPE)
    mps["pos"], mps["desc"], mps["n_obs"] = X, d0, n_obs
    pts = np.zeros(n0, capi.LOCAL_POINT_DTYPE)            # the local map: the keyframe's points (MapPoint::UpdateNormalAndDepth)
    v = X - (-R.T @ t)[None, :]
    d = np.linalg.norm(v, axis=1)
    pts["pos"], pts["normal"], pts["desc"], pts["n_obs"] = X, v / d[:, None], d0, n_obs
    pts["max_dist"] = d * tab["scale"][k0["octave"]]
    pts["min_dist"] = pts["max_dist"] / tab["scale"][-1]
    ext.close()
    return dict(frames=frames, poses=poses, scale=tab["scale"], inv_s2=tab["inv_sigma2"], voc=voc, kf=kf, mps=mps, pts=pts, n0=int(n0))


def run(K, share, W, a):
    nrun = max(1, int(round(K * share)))
    vocd = capi.Vocabulary(W["voc"])
    ext = capi.OrbExtractor(nfeatures=1000, max_batch=K)
    tb = capi.TrackerBatch(ext, K)
    tb.reserve_reference_keyframe(K * 8192)
    tb.reserve_local_map(K * 4096)
    ext1 = capi.OrbExtractor(nfeatures=1000, max_batch=1)
    single = capi.Tracker(ext1)
    single.reserve_reference_keyframe(8192)
    kf, k0 = W["kf"], W["kf"]["kps"]
    times = dict(fallback=[], tick=[], singles=[])
    mismatches, complete = 0, []
    for tick in range(a.warmup + a.ticks):
        ts = [1 + (tick + b) % 4 for b in range(K)]
        runs = [(b + tick) % K < nrun for b in range(K)]                  # which agents have no motion model this tick
        pose_last = [tcw7f(ps.pose7(*W["poses"][t - 1])) for t in ts]
        imgs = np.stack([W["frames"][t] for t in ts])
        lasts = [(k0[:0], np.zeros(0, np.int32), None, W["mps"]) if r else (k0, kf["mp"], None, W["mps"]) for r in runs]
        ins = tb.prepare(pose_last, lasts)
        kfs = [kf if r else None for r in runs]
        t0 = time.perf_counter()
        first = tb.track(imgs, ins, ps.K, BOUNDS, W["scale"], W["inv_s2"], th=15.0)
        t1 = time.perf_counter()
        rb = tb.track_reference_keyframe(vocd, kfs, pose_last, ps.K, W["inv_s2"])
        t2 = time.perf_counter()
        fms = [(rb[b]["mp"] if runs[b] and "mp" in rb[b] else first[b]["mp"]).astype(np.int32) for b in range(K)]
        tb.track_local_map([W["pts"]] * K, fms, th=1.0)
        t3 = time.perf_counter()
        sec = 0.0
        for b in range(K):
            if not runs[b]:
                continue
            s0 = time.perf_counter()
            r1 = single.track_reference_keyframe(vocd, kf, pose_last[b], img=W["frames"][ts[b]], K=ps.K, bounds=BOUNDS, inv_sigma2=W["inv_s2"])
            sec += time.perf_counter() - s0
            if not (np.array_equal(r1["pose"], rb[b]["pose"]) and np.array_equal(r1["mp"], rb[b]["mp"])):
                mismatches += 1
        if tick >= a.warmup:
            times["fallback"].append(t2 - t1); times["tick"].append(t3 - t0); times["singles"].append(sec)
            complete.append(sum(r["status"] == 0 for r in rb))
    out = dict(leg="track_refkf_tick", agents=K, share=share, fallback_frames=nrun, features=W["n0"], complete_per_tick_median=float(np.median(complete)),
               mismatches=mismatches, **{k: stats(v) for k, v in times.items()})
    single.close(); ext1.close(); tb.close(); ext.close(); vocd.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--shares", type=float, nargs="+", default=[0.125, 0.5, 1.0])
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    W = world()
    for K in a.agents:
        for share in a.shares:
            print(json.dumps(run(K, share, W, a)), flush=True)


if __name__ == "__main__":
    main()
