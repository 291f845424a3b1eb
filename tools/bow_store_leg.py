"""Timing of the two chains that name keyframes resident in a dvm_keyframe_store (their map points in a dvm_map_store) against the same
chains carrying the keyframes up on every call, tools/keyframe_store_leg.py's protocol: in one process, after warm-up, alternating per
repeat, host->host, p5 / median / p95 in ms of 200 calls after 20.
  bow_targets   dvm_search_by_bow_targets[_resident], the shapes of profiles/bow_targets_leg.json: one current keyframe against 11, 33
                and 66 targets of about 1 149 keypoints.  The argument structs are built once; the keyframes are put before the loop.
                `kernels_ms`: HIP-event medians of search, settle and the resident call's prologue (dvm_bow_targets_profiling) from a
                separate pass; `upload_bytes`: dvm_bow_targets_last_upload_bytes of both forms; `same_as_uploaded`: equal rows.
  refkf (--refkf)  dvm_track_reference_keyframe_batch[_resident] on 1, 8 and 32 frames of a tick that all fall back
                (tools/track_refkf_tick_leg.py's world: frames of 1 000 features, the keyframe of the extractor's size).  Every timed
                call follows a batched first half of its own, which is not timed; the argument structs are built once.
--uploaded-only measures the uploaded forms alone and touches no new entry point, so it also runs on a library built from the parent
commit (DVM_HIP_LIB=<that library>, its libdvmslam_host.so beside it: the first half of the refkf leg goes through it): that run is the baseline.  --baseline <its json> adds the baseline's rows and, per shape,
`uploaded_within_baseline_band` (this build's uploaded median inside the baseline's p5 .. p95) and `resident_below_baseline_p5`.
Usage: python tools/bow_store_leg.py [--targets 11 33 66] [--refkf] [--frames 1 8 32] [--repeats 200] [--warmup 20] [--uploaded-only]
                                     [--baseline FILE] [--out profiles/bow_store_leg.json]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dvm_slam_amd import capi  # noqa: E402
import bow_targets_scene as bts  # noqa: E402
import pixel_scene as ps  # noqa: E402

SF = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
LEVELS = dict(K=np.array([500.0, 500.0, 320.0, 240.0], np.float32), scale_factors=SF, level_sigma2=(SF * SF).astype(np.float32),
              inv_level_sigma2=(np.float32(1.0) / (SF * SF)).astype(np.float32), log_scale_factor=float(np.log(np.float32(1.2))))


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(p5_ms=round(float(np.percentile(a, 5)), 4), median_ms=round(float(np.median(a)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


def alternate(calls, repeats, warmup, before=None):
    """calls: name -> function, timed in turn per repeat; before: name -> function run untimed in front of each timed call"""
    times = {k: [] for k in calls}
    for it in range(warmup + repeats):
        for k, f in calls.items():
            if before:
                before[k]()
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            if it >= warmup:
                times[k].append(t1 - t0)
    return {k: stats(v) for k, v in times.items()}


def bow_leg(T, repeats, warmup, uploaded_only):
    sc = bts.scene.__wrapped__(seed=2, T=T, n_pts=1000, n_clutter=250, n_nodes=300, dup=0.1, heavy_frac=0.1)   # (tools/bow_targets_leg.py's scene)
    kfs = [sc["cur"]] + list(sc["targets"])
    ns = [len(k["desc"]) for k in kfs]
    # a map point's slot: the keyframes' points back to back; the uploaded call sees mp = mp_slot and bad = the record's bad
    mps, base = [], 0
    for k in kfs:
        has = k["mp"] >= 0
        mp = np.full(len(has), -1, np.int32); mp[has] = base + np.arange(int(has.sum()), dtype=np.int32)
        base += int(has.sum())
        mps.append(mp)
    up = [dict(k, mp=m) for k, m in zip(kfs, mps)]
    h = capi.BowTargets()
    h.reserve(ns[0], T, sum(ns[1:]))
    uploaded = h.prepare(up[0], up[1:], 0.9, True)
    calls = dict(uploaded=uploaded)
    ri, rn = (x.copy() for x in uploaded())
    out = dict(leg="bow_targets", targets=T, cur_keypoints=ns[0], target_keypoints=int(np.mean(ns[1:])), matches=int(rn.sum()))
    if not uploaded_only:
        up_bytes = h.last_upload_bytes()
        store = capi.KeyframeStore(T + 1, max(ns))
        store.put(np.arange(T + 1, dtype=np.int32), [dict(k, **LEVELS) for k in kfs])
        pts = capi.MapStore(base)
        rec = np.zeros(base, capi.LOCAL_POINT_DTYPE)
        for k, m in zip(kfs, mps):
            rec["bad"][m[m >= 0]] = k["bad"][m >= 0]
        rec["n_obs"] = 1
        pts.update(np.arange(base, dtype=np.int32), rec)
        resident = h.prepare_resident(store, (0, pts, mps[0]), [(1 + t, pts, mps[1 + t]) for t in range(T)], 0.9, True)
        calls["resident"] = resident
        gi, gn = resident()
        out["same_as_uploaded"] = bool(np.array_equal(gi, ri) and np.array_equal(gn, rn))
        out["upload_bytes"] = dict(uploaded=up_bytes, resident=h.last_upload_bytes())
    out.update(alternate(calls, repeats, warmup))
    h.profiling(True)
    km = {k: [] for k in calls}
    for _ in range(30):
        for k, f in calls.items():
            f()
            km[k].append(list(h.last_kernel_ms()) + ([h.last_prologue_ms()] if not uploaded_only else []))
    out["kernels_ms"] = {k: dict(zip(("search", "settle", "prologue"), (round(float(x), 4) for x in np.median(np.array(v), axis=0)))) for k, v in km.items()}
    h.profiling(False)
    if not uploaded_only:
        store.close(); pts.close()
    h.close()
    return out


def refkf_world():
    import track_refkf_tick_leg as leg
    return leg.world()


def refkf_leg(Kf, W, repeats, warmup, uploaded_only):
    """Kf frames of a tick, none with a motion model: all fall back to the reference keyframe"""
    import track_refkf_tick_leg as leg
    vocd = capi.Vocabulary(W["voc"])
    ext = capi.OrbExtractor(nfeatures=1000, max_batch=Kf)
    tb = capi.TrackerBatch(ext, Kf)
    tb.reserve_reference_keyframe(Kf * 8192)
    kf, k0 = W["kf"], W["kf"]["kps"]
    n = len(k0)
    ts = [1 + b % 4 for b in range(Kf)]
    pose_last = [leg.tcw7f(ps.pose7(*W["poses"][t - 1])) for t in ts]
    imgs = np.stack([W["frames"][t] for t in ts])
    ins = tb.prepare(pose_last, [(k0[:0], np.zeros(0, np.int32), None, W["mps"])] * Kf)

    def first_half():
        tb.track(imgs, ins, ps.K, leg.BOUNDS, W["scale"], W["inv_s2"], th=15.0)

    def structs(resident):
        """the argument arrays of one call, built once: (call, results, keepalive)"""
        kfp = (C.POINTER(capi.KfResident if resident else capi.RefKeyframe) * Kf)(); prs = (capi.TrackRefKfParams * Kf)(); outs = (capi.TrackRefKfOut * Kf)()
        res = (capi.TrackRefKfResult * Kf)(); status = np.zeros(Kf, np.int32)
        keep = []
        for b in range(Kf):
            if resident:
                rk, ka = capi.KfResident(), []
                capi._kf_resident((b % 2, pts, kf["mp"]), rk, ka)
            else:
                rk, ka = capi._ref_keyframe(kf)
            pr, s2 = capi._refkf_params(pose_last[b], ps.K, W["inv_s2"], 0.7, True, 50, 15, 10, 4)
            o, arrs = capi._refkf_out(ext.cap)
            kfp[b] = C.pointer(rk); prs[b] = pr; outs[b] = o
            keep.append((rk, ka, s2, arrs))
        if resident:
            def call():
                capi.check(tb.L.dvm_track_reference_keyframe_batch_resident(tb.t, ext.h, vocd.h, store.h, Kf, kfp, prs, outs, res, status))
        else:
            def call():
                capi.check(tb.L.dvm_track_reference_keyframe_batch(tb.t, ext.h, vocd.h, Kf, kfp, prs, outs, res, status))
        return call, (res, keep), status

    def snapshot(r):
        res, keep = r
        return [(bytes(res[b]),) + tuple(keep[b][3][k][:res[b].n].copy() for k in ("mp", "outlier", "dropped")) for b in range(Kf)]

    up_call, up_res, up_status = structs(False)
    calls = dict(uploaded=up_call)
    first_half(); up_call()
    want = snapshot(up_res)
    out = dict(leg="track_reference_keyframe", frames=Kf, keyframe_keypoints=n, complete=int((up_status == 0).sum()))
    if not uploaded_only:
        up_bytes = tb.last_refkf_upload_bytes()
        store = capi.KeyframeStore(2, n)
        put = dict(kps=k0, desc=kf["desc"], fv=kf["fv"], K=np.asarray(ps.K, np.float32), bounds=leg.BOUNDS, scale_factors=W["scale"],
                   level_sigma2=(W["scale"] ** 2).astype(np.float32), inv_level_sigma2=W["inv_s2"], log_scale_factor=float(np.log(W["scale"][1])))
        store.put(np.arange(2, dtype=np.int32), [put, put])
        pts = capi.MapStore(n)
        rec = np.zeros(n, capi.LOCAL_POINT_DTYPE)
        rec["pos"], rec["n_obs"], rec["bad"] = kf["pos"], kf["n_obs"], kf["bad"]
        pts.update(np.arange(n, dtype=np.int32), rec)
        res_call, res_res, _ = structs(True)
        calls["resident"] = res_call
        first_half(); res_call()
        got = snapshot(res_res)
        out["same_as_uploaded"] = bool(all(a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])) for a, b in zip(got, want)))
        out["upload_bytes"] = dict(uploaded=up_bytes, resident=tb.last_refkf_upload_bytes())
    out.update(alternate(calls, repeats, warmup, before={k: first_half for k in calls}))
    ext.sync()
    if not uploaded_only:
        store.close(); pts.close()
    tb.close(); ext.close(); vocd.close()
    return out


def shape_of(row):
    return (row["leg"], row.get("targets", row.get("frames")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, nargs="*", default=[11, 33, 66])
    ap.add_argument("--refkf", action="store_true")
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--uploaded-only", action="store_true")
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bow_store_leg.json"))
    a = ap.parse_args()
    base = {}
    if a.baseline:
        with open(a.baseline) as f:
            base = {shape_of(r): r for r in map(json.loads, filter(None, (ln.strip() for ln in f)))}
    rows = [bow_leg(T, a.repeats, a.warmup, a.uploaded_only) for T in a.targets]
    if a.refkf:
        W = refkf_world()
        rows += [refkf_leg(Kf, W, a.repeats, a.warmup, a.uploaded_only) for Kf in a.frames]
    lines = []
    for row in rows:
        b = base.get(shape_of(row))
        if b and "resident" in row:
            row["baseline"] = b["uploaded"]
            row["uploaded_within_baseline_band"] = bool(b["uploaded"]["p5_ms"] <= row["uploaded"]["median_ms"] <= b["uploaded"]["p95_ms"])
            row["resident_below_baseline_p5"] = bool(row["resident"]["median_ms"] < b["uploaded"]["p5_ms"])
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
