"""Timing of LocalBundleAdjustment on the resident stores (capi.BaResident) against the uploaded form (dvm_ba_optimize_windows_fast on the
host-gathered windows), under the protocol of the other store legs: host to host, p5 / median / p95 of --repeats after --warmup, the forms
alternating per repeat in ONE process.  Shapes: 1, 8 and 32 windows of 30 keyframes (10 fixed) / 3 000 landmarks / 5 observations each,
10 iterations; the windows of a call are the same scene at different slots (a window's result does not depend on its batch).
Forms:
  parent     --parent-lib: the library built from the parent commit, loaded beside this build's, running dvm_ba_optimize_windows_fast
  uploaded   this build's untouched dvm_ba_optimize_windows_fast
  resident   dvm_ba_resident_optimize
Two spans per shape:
  call          the optimising call alone
  store_current "LBA until the store is current".  uploaded: the call, then the records rebuilt on the host -- positions cast to float,
                UpdateNormalAndDepth for every local point (vectorised numpy here: a C++ loop over the observations does the same work in
                less time, so this span flatters the resident form by what numpy costs above C++; the call span does not) --, then
                dvm_map_store_update of every record.  resident: optimize, then commit.  Both end with a one-record read of the store, so
                that the queued write lies inside the span.
Every row carries same_as_uploaded (the resident call's poses, points, edge_chi2 and depth_positive equal the uploaded call's bit for
bit, and so do the parent's), the bytes of the resident call from dvm_ba_resident_last_bytes, and uploaded_within_parent_band (this
build's uploaded median of the call span lies inside the parent's p5 .. p95).
Usage: python tools/lba_resident_leg.py --parent-lib PATH [--windows 1 8 32] [--repeats 200] [--warmup 20] [--out profiles/lba_resident_leg.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dvm_slam_amd import capi  # noqa: E402
import ba_resident_scene as brs  # noqa: E402


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(p5_ms=round(float(np.percentile(a, 5)), 4), median_ms=round(float(np.median(a)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


def alternate(calls, repeats, warmup):
    times = {k: [] for k in calls}
    order = list(calls.items())
    for it in range(warmup + repeats):
        for k, f in order[it % len(order):] + order[:it % len(order)]:       # (the first place of a repeat goes round)
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            if it >= warmup:
                times[k].append(t1 - t0)
    return {k: stats(v) for k, v in times.items()}


def rebuilt_records(sc, before, out):
    """what the host does behind the uploaded call (Optimizer.cc:1357-1384 + UpdateNormalAndDepth), vectorised: every record of the window"""
    o = sc["obs"]
    centres = brs.camera_centres(sc["poses"], out["poses"], sc["fixed"])
    pos = out["points"].astype(np.float32)
    d = pos[o["point"]] - centres[o["pose"]]
    n = np.sqrt((d * d).sum(axis=1, dtype=np.float32))
    normal = np.zeros_like(pos)
    np.add.at(normal, o["point"], d / n[:, None])
    cnt = np.bincount(o["point"], minlength=len(pos)).astype(np.float32)
    rec = before.copy()
    used = cnt > 0
    rec["pos"][used] = pos[used]
    rec["normal"][used] = normal[used] / cnt[used, None]
    ref = o[np.maximum(sc["ref_edge"], 0)]
    dr = pos - centres[ref["pose"]]
    sf = sc["sf_of_edge"][np.maximum(sc["ref_edge"], 0)]
    mx = np.sqrt((dr * dr).sum(axis=1, dtype=np.float32)) * sf
    rec["max_dist"][used] = mx[used]; rec["min_dist"][used] = (mx / sc["sf_last_of_edge"][np.maximum(sc["ref_edge"], 0)])[used]
    return rec


def shape(K, sc, parent, repeats, warmup):
    scenes = [sc] * K
    pl = brs.Placed(scenes, use_model=False)
    wins = capi.BaWindowBatch([brs.host_window(sc, use_model=False) for _ in range(K)])
    rb = capi.BaResidentBatch([dict(p, want_geometry=False) for p in pl.problems()])     # what a LocalMapping thread fetches: flags and edges, no geometry
    h = capi.BaResident()
    before = sc["records"]
    slots_all = np.concatenate(pl.mp_slots)
    one = slots_all[:1].copy()
    fn_parent = parent.dvm_ba_optimize_windows_fast
    fn_parent.restype = C.c_int32; fn_parent.argtypes = None
    pwins = capi.BaWindowBatch([brs.host_window(sc, use_model=False) for _ in range(K)])

    def call_parent():
        rc = fn_parent(C.c_int32(0), pwins.wins, C.c_int32(K), None, pwins.stats)
        assert rc == 0, rc

    def call_uploaded():
        wins.run(fast=True, collect=False)

    def call_resident():
        h.run(rb, collect=False)

    def current_uploaded():
        wins.run(fast=True, collect=False)
        recs = np.concatenate([rebuilt_records(sc, before, o) for o in wins.outs])
        pl.map_store.update(slots_all, recs)
        pl.map_store.read(one)

    def current_resident():
        # (the resident form starts from what the store holds: the records are put back outside the span, below)
        h.run(rb, collect=False)
        h.commit()
        pl.map_store.read(one)
    call_parent(); call_uploaded(); call_resident()
    keys = ("poses", "points", "edge_chi2", "depth_positive")
    same = all(r[k].tobytes() == u[k].tobytes() == p[k].tobytes() for r, u, p in zip(rb.outs, wins.outs, pwins.outs) for k in keys)
    up, down = h.last_bytes()
    row = dict(leg="lba_resident", windows=K, keyframes=sc["P"], landmarks=sc["L"], edges=sc["E"], iterations=sc["iterations"], same_as_uploaded=bool(same),
               resident_bytes=dict(host_to_device=up, device_to_host=down), uploaded_payload_bytes_per_window=32 * sc["E"] + 24 * sc["L"],
               resident_payload_bytes_per_window=12 * sc["E"] + 8 * sc["L"] + 4 * sc["E"] + 4 * (sc["L"] + 1))
    row["call"] = alternate(dict(parent=call_parent, uploaded=call_uploaded, resident=call_resident), repeats, warmup)

    # the resident span changes the records it then reads: both forms start every repeat from the original records (restored outside the spans)
    times = dict(uploaded=[], resident=[])
    for it in range(warmup + repeats):
        for k, f in (("uploaded", current_uploaded), ("resident", current_resident))[::1 if it % 2 == 0 else -1]:
            pl.map_store.update(slots_all, np.concatenate([before] * K)); pl.map_store.read(one)
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            if it >= warmup:
                times[k].append(t1 - t0)
    row["store_current"] = {k: stats(v) for k, v in times.items()}
    b = row["call"]["parent"]
    row["uploaded_within_parent_band"] = bool(b["p5_ms"] <= row["call"]["uploaded"]["median_ms"] <= b["p95_ms"])
    h.close(); pl.kf_store.close(); pl.map_store.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--windows", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lba_resident_leg.json"))
    a = ap.parse_args()
    capi.lib()
    parent = C.CDLL(os.path.abspath(a.parent_lib))
    sc = brs.make_window(38, 30, 3000, 15000, 10, iterations=10)
    o = sc["obs"]
    sc["sf_of_edge"] = np.array([sc["kfs"][p]["scale_factors"][sc["kfs"][p]["kps"]["octave"][k]] for p, k in zip(o["pose"], o["kp"])], np.float32)
    sc["sf_last_of_edge"] = np.array([sc["kfs"][p]["scale_factors"][-1] for p in o["pose"]], np.float32)
    lines = []
    for K in a.windows:
        lines.append(json.dumps(shape(K, sc, parent, a.repeats, a.warmup)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
