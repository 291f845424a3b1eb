"""Timing of LocalMapping::CreateNewMapPoints for a KannalaBrandt8 agent at the shape of tools/new_points_leg.py: one new keyframe with 30
neighbour keyframes of about 1 900 keypoints each, seen through the fisheye camera (tests/kb8_tri_scene.fisheye_of).  In one process, after
warm-up, alternating per repeat:
  (a) chain        one NewPoints.create_new_map_points_cam call (dvm_create_new_map_points_cam)
  (b) loop         per neighbour capi.search_for_triangulation_cam, then capi.triangulate_matches_cam, the current keyframe's table updated
                   in between -- two blocking round trips per neighbour
  (c) pinhole      the pinhole chain (dvm_create_new_map_points) on the pinhole scene of the same shape, in the same process
Both fisheye forms give the same records (checked once, before timing).  Host-to-host medians and p95 in ms; `kernels_ms` are HIP-event
times of the chain's launches from a separate pass with the handle's profiling on.  --parent takes
the JSON line tools/new_points_leg.py wrote on the parent commit in the same session and records it beside.  Nothing is asserted on the times.
One JSON line, also written to profiles/kb8_new_points_leg.json.
Usage: python tools/kb8_new_points_leg.py [--neighbours 30] [--repeats 200] [--warmup 20] [--parent FILE] [--out profiles/kb8_new_points_leg.json]"""
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
import kb8_tri_scene as kt  # noqa: E402
import new_points_scene as nps  # noqa: E402


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


def loop(sc, views, models, T, rf):
    """the two _cam calls per neighbour; returns (pairs, status, x3D) concatenated over the neighbours"""
    cur = sc["cur"]
    mp0 = cur["mp"].copy()
    T1, Ow1 = T[0]
    P, S, Xs = [], [], []
    for j, nb in enumerate(sc["neighbours"]):
        T2, Ow2 = T[j + 1]
        if float(nps.baseline_ratio(Ow1, Ow2, sc["median_depth"][j])) < 0.01:
            continue
        n, pairs = capi.search_for_triangulation_cam(views[0], views[j + 1], models[0], models[j + 1], False, False)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        X, st = capi.triangulate_matches_cam(models[0], models[j + 1], T1, T2, Ow1, Ow2, cur["kps"], nb["kps"], pairs, cur["level_sigma2"], nb["level_sigma2"],
                                             cur["scale_factors"], nb["scale_factors"], rf)
        cur["mp"][pairs[st == 0, 0]] = nps.NEW_POINT_ID
        P.append(pairs); S.append(st); Xs.append(X)
    cur["mp"][:] = mp0                                             # the next repeat starts from the same table
    return np.concatenate(P), np.concatenate(S), np.concatenate(Xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--neighbours", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kb8_new_points_leg.json"))
    a = ap.parse_args()
    pin = nps.prefix(nps.scene.__wrapped__(seed=5, n_neighbours=a.neighbours, n_pts=2300, n_clutter=250, n_nodes=300, nb_vis=0.95), a.neighbours)
    sc = kt.fisheye_of(pin)
    sc["cur"]["mp"] = sc["cur"]["mp"].copy()
    cur = sc["cur"]
    kfs = [cur] + list(sc["neighbours"])
    views = [capi.keyframe_view(kf) for kf in kfs]
    models = [capi.CameraModel.make(capi.CameraModel.KANNALA_BRANDT8, kf["cam"]) for kf in kfs]
    T = [nps.pose_3x4(kf["Tcw"]) for kf in kfs]
    rf = np.float32(1.5) * np.float32(cur["scale_factors"][1])
    h = capi.NewPoints()
    h.reserve(len(cur["kps"]), a.neighbours, sum(len(nb["kps"]) for nb in sc["neighbours"]))
    chain = h.prepare_cam(cur, sc["neighbours"], sc["median_depth"], models[0], models[1:])
    pin_chain = h.prepare(pin["cur"], pin["neighbours"], pin["median_depth"])
    r = chain()
    lp = loop(sc, views, models, T, rf)
    same = bool(np.array_equal(r["pairs"], lp[0]) and np.array_equal(r["status"], lp[1]) and np.array_equal(r["x3D"].view(np.uint32), lp[2].view(np.uint32)))
    rp = pin_chain()
    times = dict(chain=[], loop=[], pinhole=[])
    for it in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        chain()
        t1 = time.perf_counter()
        loop(sc, views, models, T, rf)
        t2 = time.perf_counter()
        pin_chain()
        t3 = time.perf_counter()
        if it >= a.warmup:
            times["chain"].append(t1 - t0); times["loop"].append(t2 - t1); times["pinhole"].append(t3 - t2)
    h.profiling(True)
    km = {}
    for name, run in (("chain", chain), ("pinhole", pin_chain)):
        v = []
        for _ in range(50):
            run()
            v.append(h.last_kernel_ms())
        v = np.median(np.array(v), axis=0)
        km[name] = dict(search=round(float(v[0]), 4), geometry=round(float(v[1]), 4), settle=round(float(v[2]), 4))
    out = dict(leg="kb8_new_points", neighbours=a.neighbours, neighbours_run=int((r["nb_status"] == 0).sum()), kf1_keypoints=len(cur["kps"]),
               kf1_without_point=int((cur["mp"] < 0).sum()), neighbour_keypoints_mean=float(np.mean([len(nb["kps"]) for nb in sc["neighbours"]])),
               shared_nodes=len(cur["fv"]["fv_nodes"]), records=len(r["pairs"]), accepted=int((r["status"] == 0).sum()), same_as_loop=same,
               pinhole_records=len(rp["pairs"]), pinhole_accepted=int((rp["status"] == 0).sum()),
               chain=stats(times["chain"]), loop=stats(times["loop"]), pinhole_chain=stats(times["pinhole"]),
               kernels_ms=km)
    if a.parent:
        with open(a.parent) as f:
            p = json.loads(f.readline())
        out["parent_pinhole_chain"] = dict(chain=p["chain"], loop=p["loop"], kernels_ms=p["kernels_ms"], records=p["records"])
    h.close()
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
