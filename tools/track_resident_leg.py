"""Timing of a whole tracked frame for K agents sharing one GPU with the agents' map points RESIDENT on the device (capi.MapStore) against
the same tick with the map points uploaded, on the dense stream and tables of tools/track_tick_leg.py (~3 000 points per agent).  In one
process, after warm-up, three ticks alternate tick by tick on the same frames:
  (u1) uploaded   TrackerBatch.track + TrackerBatch.track_local_map
  (r)  resident   TrackerBatch.track_resident + TrackerBatch.track_local_map_resident (entry lists and slot lists up, no records)
  (u2) uploaded   again -- two copies of the same call: |median(u1) - median(u2)| is the spread the resident tick is judged against
The stores are filled once, outside the clock; every fifth tick an update of 5 % of each agent's records is timed on its own (K calls,
until the last one has returned -- the copies themselves run behind).  Times are host to host around calls that end in their one
synchronisation.  One JSON line per K: medians and p95 in ms, upload bytes per tick (dvm_tracker_last_upload_bytes) of both forms, and
`mismatches` (resident against uploaded: mp, outlier and pose of every agent), which must be 0.  DVM_TRACK_BATCH_TIMING=1 prints the host
phases of both forms on stderr.
Usage: python tools/track_resident_leg.py [--agents 8 32 64] [--ticks 30] [--warmup 5] [--th 1]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dvm_slam_amd import capi  # noqa: E402
from track_local_map_leg import BOUNDS, KC  # noqa: E402
from track_tick_leg import build_cases, stats  # noqa: E402


def run(K, cases, stores, slot_of, scale, inv_s2, a):
    extB = capi.OrbExtractor(max_batch=K)
    trkB = capi.TrackerBatch(extB, K)
    trkB.reserve_local_map(K * 4096)
    Tcw = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
    times = dict(u1_tick=[], r_tick=[], u2_tick=[], u1_first=[], r_first=[], u1_second=[], r_second=[], update_5pct=[])
    up_bytes = dict(uploaded_first=[], uploaded_second=[], resident_first=[], resident_second=[])
    mismatches, tracked = 0, []
    rng = np.random.default_rng(2)

    def uploaded(sel, imgs, ins):
        t0 = time.perf_counter()
        first = trkB.track(imgs, ins, KC, BOUNDS, scale, inv_s2, th=15.0)
        t1 = time.perf_counter()
        b1 = trkB.last_upload_bytes()[0]
        fms = [f["mp"].copy() for f in first]
        t2 = time.perf_counter()
        sec = trkB.track_local_map([c[3] for c in sel], fms, th=a.th)
        t3 = time.perf_counter()
        return (t1 - t0) + (t3 - t2), t1 - t0, t3 - t2, sec, (b1, trkB.last_upload_bytes()[1])

    def resident(ci, sel, imgs, rins, inv):
        t0 = time.perf_counter()
        first = trkB.track_resident(imgs, rins, KC, BOUNDS, scale, inv_s2, th=15.0)
        t1 = time.perf_counter()
        b1 = trkB.last_upload_bytes()[0]
        # the frame's points as table positions (the stores hold table entry i at slot slot_of[i])
        fms = [np.where(f["mp"] >= 0, inv[c][np.maximum(f["mp"], 0)], -1).astype(np.int32) for c, f in zip(ci, first)]
        t2 = time.perf_counter()
        sec = trkB.track_local_map_resident([stores[c] for c in ci], [slot_of[c] for c in ci], fms, th=a.th)
        t3 = time.perf_counter()
        return (t1 - t0) + (t3 - t2), t1 - t0, t3 - t2, sec, (b1, trkB.last_upload_bytes()[1])

    inv = []
    for c in range(len(cases)):
        v = np.full(stores[c].capacity, -1, np.int32); v[slot_of[c]] = np.arange(len(slot_of[c]), dtype=np.int32)
        inv.append(v)
    for tick in range(a.warmup + a.ticks):
        ci = [(tick * 7 + 3 * b) % len(cases) for b in range(K)]                 # agent b's frame of this tick
        sel = [cases[c] for c in ci]
        imgs = np.stack([c[0] for c in sel])
        ins = trkB.prepare([Tcw] * K, [(c[1], c[2], None, c[4]) for c in sel])
        rins = trkB.prepare_resident([Tcw] * K, [(cases[c][1], slot_of[c][cases[c][2]], None, stores[c]) for c in ci])
        timed = tick >= a.warmup
        u1 = uploaded(sel, imgs, ins)
        r = resident(ci, sel, imgs, rins, inv)
        u2 = uploaded(sel, imgs, ins)
        for b in range(K):
            x, y = u1[3][b], r[3][b]
            if x["status"] != y["status"] or (x["status"] == 0 and not (np.array_equal(x["mp"], y["mp"]) and np.array_equal(x["outlier"], y["outlier"]) and
                                                                         np.array_equal(x["pose"], y["pose"]))):
                mismatches += 1
        if timed:
            times["u1_tick"].append(u1[0]); times["r_tick"].append(r[0]); times["u2_tick"].append(u2[0])
            times["u1_first"].append(u1[1]); times["r_first"].append(r[1]); times["u1_second"].append(u1[2]); times["r_second"].append(r[2])
            up_bytes["uploaded_first"].append(u1[4][0]); up_bytes["uploaded_second"].append(u1[4][1])
            up_bytes["resident_first"].append(r[4][0]); up_bytes["resident_second"].append(r[4][1])
            tracked.append(sum(x["status"] == 0 for x in r[3]))
        if tick % 5 == 4:      # LocalMapping's write: 5 % of each agent's records (the same values: the results stay comparable)
            picks = [rng.permutation(len(slot_of[c]))[:max(1, len(slot_of[c]) // 20)] for c in ci]
            t0 = time.perf_counter()
            for c, pk in zip(ci, picks):
                stores[c].update(slot_of[c][pk], cases[c][3][pk])
            if timed:
                times["update_5pct"].append(time.perf_counter() - t0)
    out = dict(leg="track_resident", agents=K, th=a.th, table_points_median=int(np.median([len(cases[c][3]) for c in range(len(cases))])),
               tracked_per_tick_median=float(np.median(tracked)), mismatches=mismatches, **{k: stats(v) for k, v in times.items() if v},
               upload_bytes_per_tick={k: int(np.median(v)) for k, v in up_bytes.items()})
    m = {k: np.median(times[k]) * 1e3 for k in ("u1_tick", "u2_tick", "r_tick")}
    out["uploaded_spread_ms"] = round(float(abs(m["u1_tick"] - m["u2_tick"])), 4)
    out["resident_minus_uploaded_ms"] = round(float(m["r_tick"] - 0.5 * (m["u1_tick"] + m["u2_tick"])), 4)
    lo, hi = min(m["u1_tick"], m["u2_tick"]), max(m["u1_tick"], m["u2_tick"])
    out["verdict"] = "faster" if m["r_tick"] < lo - out["uploaded_spread_ms"] else "slower" if m["r_tick"] > hi + out["uploaded_spread_ms"] else "within the spread"
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
    rng = np.random.default_rng(1)
    cases = build_cases(40, ext1, scale, rng)
    stores, slot_of = [], []
    for c in cases:                                  # one store per stream frame's map, filled once
        n = len(c[3])
        st = capi.MapStore(n + 64)
        so = rng.permutation(n + 64)[:n].astype(np.int32)
        st.update(so, c[3])
        stores.append(st); slot_of.append(so)
    for K in a.agents:
        print(json.dumps(run(K, cases, stores, slot_of, scale, inv_s2, a)), flush=True)
    for st in stores:
        st.close()
    ext1.close()


if __name__ == "__main__":
    main()
