"""Timing of the Fuse runs of LocalMapping::SearchInNeighbors with the map points named as map-store slots (capi.FuseTargets.run_resident,
run_hits_resident, run_hits_candidates) against the uploaded runs, under the protocol of the other store legs: ONE process on one GPU,
host to host, p5 / median / p95 of --repeats after --warmup, the forms alternating.  The targets are resident (set once, outside the
span): what is timed is a run.
Shapes: 900 points x 30 targets of 1 900 keypoints (run); 8 000 x 120 (run_hits); the second direction: the 30 lists of 1 900 entries of
30 target keyframes against one target (run_hits_candidates).
Forms:
  parent     --parent-lib: the library built from the parent commit, loaded beside this build's, running the uploaded form
  uploaded   the host builds the point table from its records (five arrays and the valid flag; vectorised numpy here -- the reference
             walks mutex-guarded getters and clones a cv::Mat per point: its share is reported on its own as host_numpy) and uploads
             it: run / run_hits.  Second direction: the host walks the lists (numpy: fuse_points_scene.candidates), builds the table of
             the candidates and the exclude mask, run_hits.
  resident   run_resident / run_hits_resident / run_hits_candidates: slot numbers only.
Every row carries same_rows (the three forms return the same rows or hits; the second direction also the same list), the bytes up
(dvm_fuse_targets_last_upload_bytes) and down (the payload of what comes back) and uploaded_within_parent_band (this build's uploaded
median lies inside the parent's p5 .. p95).  Nothing is asserted on the times.
Usage: python tools/fuse_points_leg.py --parent-lib PATH [--repeats 200] [--warmup 20] [--out profiles/fuse_points_leg.json]"""
import argparse
import contextlib
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
import fuse_points_scene as fps  # noqa: E402
import fuse_targets_scene as fts  # noqa: E402

KP = 1900


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(p5_ms=round(float(np.percentile(a, 5)), 4), median_ms=round(float(np.median(a)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


def alternate(calls, repeats, warmup):
    times = {k: [] for k in calls}
    order = list(calls.items())
    for it in range(warmup + repeats):
        for k, f in order[it % len(order):] + order[:it % len(order)]:      # the first place goes round
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            if it >= warmup:
                times[k].append(t1 - t0)
    return {k: stats(v) for k, v in times.items()}


@contextlib.contextmanager
def library(L):
    """capi's handle classes bound to another build of the library (each keeps the library it was made on)"""
    old, capi._LIB = capi._LIB, L
    try:
        yield
    finally:
        capi._LIB = old


def resident_chain(L, sc, T, max_points, max_hits):
    """(store, chain): the scene's first T targets in a keyframe store of library L, set once on a chain of L"""
    with library(L):
        store = capi.KeyframeStore(T, KP)
        h = capi.FuseTargets()
    store.put(np.arange(T, dtype=np.int32), sc["targets"][:T])
    h.reserve(max_points, T, 0)
    h.reserve_hits(max_hits)
    h.set_resident(store, range(T), [kf["Tcw"] for kf in sc["targets"][:T]])
    return store, h


class HostTable:
    """the uploaded form's host work: the table of rows `idx` of the host's records, and its time"""

    def __init__(self, recs):
        self.recs, self.numpy_s = recs, []

    def __call__(self, idx):
        t0 = time.perf_counter()
        r = self.recs[idx]
        tab = dict(pos=np.ascontiguousarray(r["pos"]), normal=np.ascontiguousarray(r["normal"]), min_dist=np.ascontiguousarray(r["min_dist"]),
                   max_dist=np.ascontiguousarray(r["max_dist"]), desc=np.ascontiguousarray(r["desc"]), valid=(r["bad"] == 0).astype(np.uint8))
        self.numpy_s.append(time.perf_counter() - t0)
        return tab


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def run_shape(name, sc, T, hits_form, parent, repeats, warmup):
    pts, skip = sc["pts"], sc["skip"][:T]
    n = len(pts["pos"])
    recs = fps.records(pts, (pts["valid"] == 0).astype(np.int32))           # (the scene's masked points are the map's bad ones)
    store = capi.MapStore(n)
    slots = np.arange(n, dtype=np.int32)
    store.update(slots, recs)
    idx = np.arange(n)
    chains = {}
    for k, L in (("parent", parent), ("uploaded", capi.lib()), ("resident", capi.lib())):
        chains[k] = resident_chain(L, sc, T, n, T * n)
    tables = {k: HostTable(recs) for k in ("parent", "uploaded")}
    out = {}

    def uploaded(k):
        h = chains[k][1]
        tab = tables[k](idx)
        out[k] = h.run_hits(tab, 3.0, skip) if hits_form else h.run(tab, 3.0, skip, want_dist=False)[:1]

    def resident():
        h = chains["resident"][1]
        out["resident"] = h.run_hits_resident(store, slots, 3.0, skip) if hits_form else h.run_resident(store, slots, 3.0, skip, want_dist=False)[:1]
    calls = dict(parent=lambda: uploaded("parent"), uploaded=lambda: uploaded("uploaded"), resident=resident)
    for f in calls.values():
        f()
    ok = same(out["parent"], out["uploaded"]) and same(out["uploaded"], out["resident"])
    n_hits = int(len(out["resident"][1])) if hits_form else int((out["resident"][0] >= 0).sum())
    up = {k: chains[k][1].last_upload_bytes()[1] for k in chains}
    down = (4 * (T + 1) + 12 * n_hits) if hits_form else 4 * T * n
    for t in tables.values():
        t.numpy_s = []
    times = alternate(calls, repeats, warmup)
    ok = ok and same(out["parent"], out["uploaded"]) and same(out["uploaded"], out["resident"])
    row = dict(leg="fuse_points", shape=name, call="run_hits" if hits_form else "run", points=n, targets=T, target_keypoints=KP, hits=n_hits, same_rows=bool(ok),
               bytes_up=up, bytes_down=dict(parent=down, uploaded=down, resident=down), call_span=times,
               host_numpy={k: stats(t.numpy_s[-repeats:]) for k, t in tables.items()})
    b = times["parent"]
    row["uploaded_within_parent_band"] = bool(b["p5_ms"] <= times["uploaded"]["median_ms"] <= b["p95_ms"])
    for st, h in chains.values():
        h.close(); st.close()
    store.close()
    return row


def second_direction(sc, n_lists, parent, repeats, warmup):
    """the current keyframe = target 0, the target keyframes = targets 1 .. n_lists: their keypoints' points as slots (clutter: -1); the current
    keyframe holds the points of half of its keypoints (the exclude list), the other half is what a candidate can fuse into"""
    pts = sc["pts"]
    n = len(pts["pos"])
    bad = (pts["valid"] == 0)
    recs = fps.records(pts, bad.astype(np.int32))
    store = capi.MapStore(n)
    slots = np.arange(n, dtype=np.int32)
    store.update(slots, recs)
    lists = [np.where(kf["pt_of_kp"] >= 0, kf["pt_of_kp"], -1).astype(np.int32) for kf in sc["targets"][1:1 + n_lists]]
    own = sc["targets"][0]["pt_of_kp"]                                      # the current keyframe holds the point of every second keypoint
    exclude = np.where((own >= 0) & (np.arange(len(own)) % 2 == 0), own, -1).astype(np.int32)
    total = sum(len(a) for a in lists)
    chains = {}
    for k, L in (("parent", parent), ("uploaded", capi.lib()), ("resident", capi.lib())):
        chains[k] = resident_chain(L, sc, 1, total, total)
    chains["resident"][1].reserve_candidates(total, n)
    tables = {k: HostTable(recs) for k in ("parent", "uploaded")}
    walk_s = {k: [] for k in tables}
    out = {}

    def uploaded(k):
        h = chains[k][1]
        t0 = time.perf_counter()
        cand = fps.candidates(lists, bad)                                    # the walk of LocalMapping.cc:826-846
        mask = np.isin(cand, exclude[exclude >= 0]).astype(np.uint8)[None, :]
        walk_s[k].append(time.perf_counter() - t0)
        out[k] = (cand, *h.run_hits(tables[k](cand), 3.0, mask))

    def resident():
        out["resident"] = chains["resident"][1].run_hits_candidates(store, lists, 3.0, exclude)
    calls = dict(parent=lambda: uploaded("parent"), uploaded=lambda: uploaded("uploaded"), resident=resident)
    for f in calls.values():
        f()
    ok = same(out["parent"], out["uploaded"]) and same(out["uploaded"], out["resident"])
    n_cand, n_hits = len(out["resident"][0]), len(out["resident"][2])
    up = {k: chains[k][1].last_upload_bytes()[1] for k in chains}
    down = dict(parent=8 + 12 * n_hits, uploaded=8 + 12 * n_hits, resident=4 * ((total + 255) // 256 + 1) + 4 * n_cand + 8 + 12 * n_hits)
    for t in tables.values():
        t.numpy_s = []
    for v in walk_s.values():
        v.clear()
    times = alternate(calls, repeats, warmup)
    ok = ok and same(out["parent"], out["uploaded"]) and same(out["uploaded"], out["resident"])
    row = dict(leg="fuse_points", shape=f"{n_lists} lists x {KP}", call="run_hits_candidates", lists=n_lists, entries=total, candidates=n_cand, map_points=n, targets=1,
               target_keypoints=KP, hits=n_hits, same_rows=bool(ok), bytes_up=up, bytes_down=down, call_span=times,
               host_numpy={k: stats(t.numpy_s[-repeats:]) for k, t in tables.items()}, host_numpy_list_walk={k: stats(v[-repeats:]) for k, v in walk_s.items()})
    b = times["parent"]
    row["uploaded_within_parent_band"] = bool(b["p5_ms"] <= times["uploaded"]["median_ms"] <= b["p95_ms"])
    for st, h in chains.values():
        h.close(); st.close()
    store.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="toy shapes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_points_leg.json"))
    a = ap.parse_args()
    capi.lib()
    parent = C.CDLL(os.path.abspath(a.parent_lib))
    parent.dvm_last_error.restype = C.c_char_p
    shapes = ((60, 3, 200, 12, 3), ) if a.small else ((900, 30, 8000, 120, 30), )
    lines = []
    for n1, T1, n2, T2, n_lists in shapes:
        sc1 = fts.scene.__wrapped__(seed=7, T=T1, n_cloud=n1, n_keypoints=KP)
        lines.append(json.dumps(run_shape(f"{n1} x {T1}", sc1, T1, False, parent, a.repeats, a.warmup)))
        print(lines[-1], flush=True)
        sc2 = fts.scene.__wrapped__(seed=7, T=T2, n_cloud=n2, n_keypoints=KP)
        lines.append(json.dumps(run_shape(f"{n2} x {T2}", sc2, T2, True, parent, a.repeats, a.warmup)))
        print(lines[-1], flush=True)
        lines.append(json.dumps(second_direction(sc2, n_lists, parent, a.repeats, a.warmup)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not all(json.loads(l)["same_rows"] for l in lines):
        sys.exit("a row whose forms differ")


if __name__ == "__main__":
    main()
