"""Timing of LocalMapping::CreateNewMapPoints for one new keyframe with 30 neighbour keyframes of about 2 000 keypoints each (about half
of them without a map point, a few hundred shared vocabulary nodes): the monocular agent's per-keyframe load.  In one process, after
warm-up, alternating per repeat:
  (a) chain   one NewPoints.create_new_map_points call (dvm_create_new_map_points), host->host
  (b) loop    the same work as the parent commit does it: per neighbour capi.search_for_triangulation (dvmh_search_for_triangulation), then
              capi.triangulate_matches (dvm_triangulate_matches), the current keyframe's table updated in between -- two blocking round
              trips per neighbour
Both give the same records (checked once, before timing).  Host-to-host medians and p95 in ms; `kernels_ms` are HIP-event times of the
chain's three launches from a separate pass with the handle's profiling on (the timed pass runs with it off).  One JSON line, also written to
profiles/new_points_leg.json.
Usage: python tools/new_points_leg.py [--neighbours 30] [--repeats 200] [--warmup 20] [--out profiles/new_points_leg.json]"""
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
import new_points_scene as nps  # noqa: E402


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


def loop(sc, views, T, rf):
    """the parent's way; returns (pairs, status, x3D) concatenated over the neighbours"""
    cur = sc["cur"]
    mp0 = cur["mp"].copy()
    T1, Ow1 = T[0]
    P, S, Xs = [], [], []
    for j, nb in enumerate(sc["neighbours"]):
        T2, Ow2 = T[j + 1]
        if float(nps.baseline_ratio(Ow1, Ow2, sc["median_depth"][j])) < 0.01:
            continue
        n, pairs = capi.search_for_triangulation(views[0], views[j + 1], False, False)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        X, st = capi.triangulate_matches(cur["K"], nb["K"], T1, T2, Ow1, Ow2, cur["kps"], nb["kps"], pairs, cur["level_sigma2"], nb["level_sigma2"],
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "new_points_leg.json"))
    a = ap.parse_args()
    # about 2 000 keypoints a keyframe (the visible points + clutter), 300 vocabulary nodes
    sc = nps.prefix(nps.scene.__wrapped__(seed=5, n_neighbours=a.neighbours, n_pts=2300, n_clutter=250, n_nodes=300, nb_vis=0.95), a.neighbours)
    cur = sc["cur"]
    views = [capi.keyframe_view(cur)] + [capi.keyframe_view(nb) for nb in sc["neighbours"]]
    T = [nps.pose_3x4(cur["Tcw"])] + [nps.pose_3x4(nb["Tcw"]) for nb in sc["neighbours"]]
    rf = np.float32(1.5) * np.float32(cur["scale_factors"][1])
    h = capi.NewPoints()
    h.reserve(len(cur["kps"]), a.neighbours, sum(len(nb["kps"]) for nb in sc["neighbours"]))
    chain = h.prepare(cur, sc["neighbours"], sc["median_depth"])     # (the loop's views are built once as well)
    r = chain()
    lp = loop(sc, views, T, rf)
    same = bool(np.array_equal(r["pairs"], lp[0]) and np.array_equal(r["status"], lp[1]) and np.array_equal(r["x3D"].view(np.uint32), lp[2].view(np.uint32)))
    times = dict(chain=[], loop=[])
    for it in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        chain()
        t1 = time.perf_counter()
        loop(sc, views, T, rf)
        t2 = time.perf_counter()
        if it >= a.warmup:
            times["chain"].append(t1 - t0); times["loop"].append(t2 - t1)
    h.profiling(True)
    km = []
    for _ in range(50):
        chain()
        km.append(h.last_kernel_ms())
    km = np.median(np.array(km), axis=0)
    out = dict(leg="new_points", neighbours=a.neighbours, neighbours_run=int((r["nb_status"] == 0).sum()), kf1_keypoints=len(cur["kps"]),
               kf1_without_point=int((cur["mp"] < 0).sum()), neighbour_keypoints_mean=float(np.mean([len(nb["kps"]) for nb in sc["neighbours"]])),
               shared_nodes=len(cur["fv"]["fv_nodes"]), records=len(r["pairs"]), accepted=int((r["status"] == 0).sum()), same_as_loop=same,
               chain=stats(times["chain"]), loop=stats(times["loop"]),
               kernels_ms=dict(search=round(float(km[0]), 4), geometry=round(float(km[1]), 4), settle=round(float(km[2]), 4)))
    h.close()
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
