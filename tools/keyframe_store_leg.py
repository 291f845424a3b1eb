"""Timing of the two LocalMapping chains on keyframes resident in a dvm_keyframe_store against the same chains carrying the keyframes up
on every call.  Shapes: the Fuse chain at 30 and 120 targets x 1 900 keypoints x 900 points (tools/fuse_targets_leg.py's scene) and
CreateNewMapPoints at 30 neighbours of about 2 000 keypoints (tools/new_points_leg.py's scene).  In one process, after warm-up,
alternating per repeat, host->host:
  uploaded   FuseTargets.set + run / NewPoints.create_new_map_points: what the library did before the store
  resident   FuseTargets.set_resident + run / NewPoints.create_new_map_points_resident on keyframes put once, before the loop
Both give the same rows / records (checked once, before timing).  The put of the keyframes is timed apart: the host's share of the call
(validate, pack, queue) and the call up to the device having finished.  Every row carries p5, median and p95 in ms and the upload byte
counters of both forms.
--uploaded-only measures the uploaded forms alone and touches no store entry point, so it also runs on a library built from the commit
before the store (DVM_HIP_LIB=<that library>): that run is the baseline.  --baseline <its json> adds the baseline's rows to the output
and the verdict the store was asked for, per shape: `resident_below_baseline_p5` (the resident median lies below the baseline's p5) and
`uploaded_within_baseline_band` (this build's uploaded median lies inside the baseline's p5 .. p95).
Usage: python tools/keyframe_store_leg.py [--targets 30 120] [--neighbours 30] [--repeats 200] [--warmup 20] [--uploaded-only]
                                          [--baseline FILE] [--out profiles/keyframe_store_leg.json]"""
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
import new_points_scene as nps  # noqa: E402


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(p5_ms=round(float(np.percentile(a, 5)), 4), median_ms=round(float(np.median(a)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


def device_idle():
    import torch
    torch.cuda.synchronize()


def time_put(store, slots, arr, repeats):
    """(host share of put, put until the device has finished), per call"""
    host, done = [], []
    for _ in range(repeats):
        device_idle()
        t0 = time.perf_counter()
        store.put_raw(slots, arr)
        t1 = time.perf_counter()
        device_idle()
        t2 = time.perf_counter()
        host.append(t1 - t0); done.append(t2 - t0)
    return stats(host), stats(done)


def alternate(calls, repeats, warmup):
    times = {k: [] for k in calls}
    for it in range(warmup + repeats):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            if it >= warmup:
                times[k].append(t1 - t0)
    return {k: stats(v) for k, v in times.items()}


def fuse_leg(T, repeats, warmup, uploaded_only):
    sc = fts.scene.__wrapped__(seed=7, T=T, n_cloud=900, n_keypoints=1900)
    pts, skip = sc["pts"], sc["skip"]
    n = len(pts["pos"])
    h = capi.FuseTargets()
    h.reserve(n, T, T * 1900)
    arr, keep = h.targets(sc["targets"])

    def uploaded():
        h.set_raw(arr, T)
        return h.run(pts, 3.0, skip, want_dist=False)[0]
    calls = dict(uploaded=uploaded)
    out = dict(leg="fuse_targets", targets=T, points=n, target_keypoints=1900)
    rows = uploaded()
    if not uploaded_only:
        up_set, up_run = h.last_upload_bytes()
        store = capi.KeyframeStore(T, 1900)
        recs, keep2 = store.records(sc["targets"])
        slots = np.arange(T, dtype=np.int32)
        store.put_raw(slots, recs)
        hr = capi.FuseTargets()
        hr.reserve(n, T, 0)
        res = hr.resident_targets(slots, [kf["Tcw"] for kf in sc["targets"]])

        def resident():
            hr.set_resident_raw(store, res, T)
            return hr.run(pts, 3.0, skip, want_dist=False)[0]
        calls["resident"] = resident
        out["same_rows"] = bool(np.array_equal(rows, resident()))
        res_set, res_run = hr.last_upload_bytes()
        out["upload_bytes"] = dict(uploaded_set=up_set, uploaded_run=up_run, resident_set=res_set, resident_run=res_run)
    out.update(alternate(calls, repeats, warmup))
    if not uploaded_only:
        host, done = time_put(store, slots, recs, 20)
        out["put"] = dict(keyframes=T, host=host, until_done=done, until_done_per_keyframe_ms=round(done["median_ms"] / T, 5))
        hr.profiling(True)
        km = []
        for _ in range(30):
            resident()
            km.append(hr.last_kernel_ms())
        out["resident_kernels_ms"] = dict(search=round(float(np.median(np.array(km), axis=0)[1]), 4))
        hr.close(); store.close()
    h.close()
    return out


def new_points_leg(n_nb, repeats, warmup, uploaded_only):
    sc = nps.prefix(nps.scene.__wrapped__(seed=5, n_neighbours=n_nb, n_pts=2300, n_clutter=250, n_nodes=300, nb_vis=0.95), n_nb)
    cur, nbs = sc["cur"], sc["neighbours"]
    h = capi.NewPoints()
    h.reserve(len(cur["kps"]), n_nb, sum(len(nb["kps"]) for nb in nbs))
    uploaded = h.prepare(cur, nbs, sc["median_depth"])
    calls = dict(uploaded=uploaded)
    r = uploaded()
    out = dict(leg="new_points", neighbours=n_nb, neighbours_run=int((r["nb_status"] == 0).sum()), kf1_keypoints=len(cur["kps"]),
               neighbour_keypoints_mean=float(np.mean([len(nb["kps"]) for nb in nbs])), records=len(r["pairs"]))
    if not uploaded_only:
        up_bytes = h.last_upload_bytes()
        K = max(len(kf["kps"]) for kf in [cur] + list(nbs))
        store = capi.KeyframeStore(n_nb + 1, K)
        recs, keep = store.records([cur] + list(nbs))
        slots = np.arange(n_nb + 1, dtype=np.int32)
        store.put_raw(slots, recs)
        resident = h.prepare_resident(store, 0, cur, list(range(1, n_nb + 1)), nbs, sc["median_depth"])
        calls["resident"] = resident
        q = resident()
        out["same_records"] = bool(all(np.array_equal(r[k], q[k]) for k in nps.RESULT_KEYS) and np.array_equal(r["x3D"].view(np.uint32), q["x3D"].view(np.uint32)))
        out["upload_bytes"] = dict(uploaded=up_bytes, resident=h.last_upload_bytes())
    out.update(alternate(calls, repeats, warmup))
    if not uploaded_only:
        host, done = time_put(store, slots, recs, 20)
        out["put"] = dict(keyframes=n_nb + 1, host=host, until_done=done, until_done_per_keyframe_ms=round(done["median_ms"] / (n_nb + 1), 5))
        store.close()
    h.close()
    return out


def shape_of(row):
    return (row["leg"], row.get("targets", row.get("neighbours")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, nargs="+", default=[30, 120])
    ap.add_argument("--neighbours", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--uploaded-only", action="store_true")
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_store_leg.json"))
    a = ap.parse_args()
    base = {}
    if a.baseline:
        with open(a.baseline) as f:
            base = {shape_of(r): r for r in map(json.loads, filter(None, (ln.strip() for ln in f)))}
    rows = [fuse_leg(T, a.repeats, a.warmup, a.uploaded_only) for T in a.targets] + [new_points_leg(a.neighbours, a.repeats, a.warmup, a.uploaded_only)]
    lines = []
    for row in rows:
        b = base.get(shape_of(row))
        if b and "resident" in row:
            row["baseline"] = b["uploaded"]
            row["resident_below_baseline_p5"] = bool(row["resident"]["median_ms"] < b["uploaded"]["p5_ms"])
            row["uploaded_within_baseline_band"] = bool(b["uploaded"]["p5_ms"] <= row["uploaded"]["median_ms"] <= b["uploaded"]["p95_ms"])
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
