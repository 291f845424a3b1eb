"""Timing of LoopClosing::SearchAndFuse (LoopClosing.cc:2132-2205): Fuse(pKFi, Scw, vpMapPoints, 4, vpReplacePoints) for T corrected keyframes
of 1 900 keypoints against n loop / merge points, th = 4, every keyframe under an Scw of scale 0.7 .. 1.4.  One process alternates per
repeat, on the same inputs (every keyframe's mvpMapPoints restored before each variant, outside the timed region):
  (a)  loop      dvmh_fuse_sim3 once per keyframe: one upload, one grid build, one synchronisation each (what the parent commit has)
  (b)  dense     the chain with the dense result: the already-found mask in numpy, dvm_fuse_targets_set_cam (DVM_FT_FORM_SCW) +
                 dvm_fuse_targets_run, the hits taken from the T x n rows on the host, dvmh_fuse_sim3_apply per keyframe
  (c)  hits      dvmh_fuse_sim3_targets (mask in C++, set_cam + dvm_fuse_targets_run_hits) + dvmh_fuse_sim3_apply per keyframe
  (a2) loop      (a) again: the spread of (a) against its second copy is the yardstick for every other difference
`mismatches` counts what (b) and (c) give otherwise than (a): replace, nFused and every keyframe's mvpMapPoints; it must be 0.
`result_forms` times the two result forms alone on the resident targets with the mask already built: dvm_fuse_targets_run (best_idx and
best_dist, T x n int32 each, copied back) against dvm_fuse_targets_run_hits.  One more row: a robomaster (KannalaBrandt8) agent's
SearchInNeighbors -- 30 targets, 900 points, LocalMapping form, th = 3 -- the chain against the loop of dvm_project_search_cam (grid build
and search per neighbour).  Host to host, `repeats` timed after `warmup`; median and p5 - p95 in ms.  One JSON line per row, all written to
profiles/search_and_fuse_leg.json.
Usage: python tools/search_and_fuse_leg.py [--targets 30 120] [--points 3000 8000] [--repeats 30] [--warmup 5] [--out ...]"""
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
import fuse_cam_scene as fcs  # noqa: E402
import kb8_scene as ks  # noqa: E402

TH = 4.0


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p5_ms=round(float(np.percentile(a, 5)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


def timed(variants, repeats, warmup, before=lambda: None):
    """Alternates the variants per repeat; `before` runs ahead of each one, outside the timed region."""
    times = {k: [] for k, _ in variants}
    for it in range(warmup + repeats):
        for k, fn in variants:
            before()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if it >= warmup:
                times[k].append(t1 - t0)
    return {k: stats(v) for k, v in times.items()}


def measure(T, n, repeats, warmup):
    sc = fcs.scw_scene.__wrapped__(T, n, seed=7, n_cloud=n, n_keypoints=1900)
    pts = sc["pts"]
    P = capi.map_points_view(pts)
    mp0 = [kf["mp"].copy() for kf in sc["targets"]]
    kfs = [dict(kf, mp=kf["mp"].copy()) for kf in sc["targets"]]
    views = [capi.keyframe_view(d) for d in kfs]
    Scws = np.stack([kf["Scw"] for kf in sc["targets"]])
    cpts = {k: pts[k] for k in ("pos", "normal", "min_dist", "max_dist", "desc")}
    h = capi.FuseTargets()
    h.reserve(n, T, T * 1900)
    h.reserve_hits(T * n)
    arr, keep = h.targets([fcs.chain_target(kf) for kf in sc["targets"]])
    for t, kf in enumerate(sc["targets"]):
        arr[t].Ow = (C.c_float * 3)(*kf["Ow_s"])
    forms = np.ones(T, np.uint8)
    n_hits = int((fcs.scw_rows(sc["targets"], pts, fcs.already_found_mask(sc["targets"], pts))[0] >= 0).sum())   # (the oracle's count: sizes hit_cap)
    cap = n_hits + n_hits // 4 + 64

    def restore():
        for d, m in zip(kfs, mp0):
            d["mp"][:] = m

    def result(nf, rep):
        return dict(nFused=list(nf), replace=np.stack(rep), mp=[d["mp"].copy() for d in kfs])

    def loop():
        out = [capi.fuse_sim3(views[t], Scws[t], P, TH) for t in range(T)]
        return [o[0] for o in out], [o[1] for o in out]

    def set_scw():
        capi.check(h.L.dvm_fuse_targets_set_cam(h.h, T, C.addressof(arr), None, forms.ctypes.data))
        h.n_targets = T

    def apply(off, hits):
        out = [capi.fuse_sim3_apply(views[t], P, hits[off[t]:off[t + 1]]) for t in range(T)]
        return [o[0] for o in out], [o[1] for o in out]

    def dense():
        skip = np.stack([(pts["bad"] != 0) | np.isin(pts["id"], d["mp"]) for d in kfs]).astype(np.uint8)
        set_scw()
        bi, bd = h.run(cpts, TH, skip)
        return apply(*fcs.hits_of(bi, bd))

    def hits():
        off, hh = capi.fuse_sim3_targets(views, Scws, P, TH, hit_cap=cap)
        return apply(off, hh)
    # ---- the results, once
    res = {}
    for k, fn in (("loop", loop), ("dense", dense), ("hits", hits)):
        restore()
        res[k] = result(*fn())
    ref = res["loop"]
    mism = {k: int(sum(a != b for a, b in zip(res[k]["nFused"], ref["nFused"])) + (res[k]["replace"] != ref["replace"]).sum() +
                   sum((a != b).sum() for a, b in zip(res[k]["mp"], ref["mp"]))) for k in ("dense", "hits")}
    # ---- the timing
    tm = timed([("loop", loop), ("dense", dense), ("hits", hits), ("loop2", loop)], repeats, warmup, restore)
    # ---- the two result forms alone
    restore()
    skip = fcs.already_found_mask(kfs, pts)
    set_scw()
    assert int(h.run_hits(cpts, TH, skip, hit_cap=cap)[0][-1]) == n_hits
    forms_tm = timed([("run", lambda: h.run(cpts, TH, skip)), ("run_hits", lambda: h.run_hits(cpts, TH, skip, hit_cap=n_hits)),
                      ("run2", lambda: h.run(cpts, TH, skip))], repeats, warmup)
    h.close()
    a, a2 = tm["loop"]["median_ms"], tm["loop2"]["median_ms"]
    return dict(leg="search_and_fuse", targets=T, points=n, target_keypoints=1900, th=TH, entries=T * n, hits=n_hits, nFused=int(sum(ref["nFused"])),
                replaced=int((ref["replace"] >= 0).sum()), mismatches=mism["dense"] + mism["hits"], mismatches_dense=mism["dense"], mismatches_hits=mism["hits"],
                loop=tm["loop"], dense=tm["dense"], hits_chain=tm["hits"], loop_again=tm["loop2"],
                loop_spread=round(abs(a - a2) / min(a, a2), 4), loop_over_dense=round(a / tm["dense"]["median_ms"], 2),
                loop_over_hits=round(a / tm["hits"]["median_ms"], 2), dense_over_hits=round(tm["dense"]["median_ms"] / tm["hits"]["median_ms"], 3),
                result_forms=dict(run=forms_tm["run"], run_hits=forms_tm["run_hits"], run_again=forms_tm["run2"], dense_bytes=2 * 4 * T * n,
                                  hit_bytes=12 * n_hits + 4 * (T + 1),
                                  run_spread=round(abs(forms_tm["run"]["median_ms"] - forms_tm["run2"]["median_ms"]) /
                                                   min(forms_tm["run"]["median_ms"], forms_tm["run2"]["median_ms"]), 4),
                                  run_over_run_hits=round(forms_tm["run"]["median_ms"] / forms_tm["run_hits"]["median_ms"], 3)))


def measure_robomaster(repeats, warmup, T=30, n=900, th=3.0):
    sc = fcs.kb8_scene.__wrapped__("robomaster", T, n, seed=7, n_kp=1900)
    mdl = capi.CameraModel.robomaster()
    tg = [fcs.kb8_chain_target(x) for x in sc["targets"]]
    pts = {k: sc["pts"][k] for k in ("pos", "normal", "min_dist", "max_dist", "desc", "valid")}
    skip = sc["skip"]
    valid = ((skip == 0) & (pts["valid"][None, :] != 0)).astype(np.uint8)
    h = capi.FuseTargets()
    h.reserve(n, T, T * 1900)
    arr, keep = h.targets(tg)
    for t, x in enumerate(tg):
        arr[t].Ow = (C.c_float * 3)(*x["Ow"])
    models = (capi.CameraModel * T)(*([mdl] * T))
    grid = capi.FrameGrid(2048)
    cams = [dict(Tcw=x["Tcw"], Ow=x["Ow"], bounds=x["bounds"], log_scale_factor=x["log_scale_factor"]) for x in tg]
    spts = {k: v for k, v in pts.items() if k != "valid"}

    def chain():
        capi.check(h.L.dvm_fuse_targets_set_cam(h.h, T, C.addressof(arr), C.addressof(models), None))
        h.n_targets = T
        return h.run(pts, th, skip, want_dist=False)[0]

    def loop():
        rows = []
        for t, x in enumerate(tg):
            grid.build(x["kps"], x["desc"], tuple(float(v) for v in x["bounds"]))
            m, _ = capi.project_search_cam(grid, cams[t], mdl, spts, th, ks.SCALE, gate_inv_sigma2=ks.INV_SIGMA2, gate=5.99, valid=valid[t])
            rows.append(np.where(m["best_dist"] <= 50, m["best_idx"], -1))
        return np.stack(rows)
    rows = chain()
    mism = int((rows != loop()).sum())
    tm = timed([("loop", loop), ("chain", chain), ("loop2", loop)], repeats, warmup)
    h.close(); grid.close()
    a, a2 = tm["loop"]["median_ms"], tm["loop2"]["median_ms"]
    return dict(leg="search_in_neighbors_robomaster", camera="KannalaBrandt8 (robomaster)", targets=T, points=n, target_keypoints=1900, th=th, entries=T * n,
                hits=int((rows >= 0).sum()), mismatches=mism, loop=tm["loop"], chain=tm["chain"], loop_again=tm["loop2"],
                loop_spread=round(abs(a - a2) / min(a, a2), 4), loop_over_chain=round(a / tm["chain"]["median_ms"], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, nargs="+", default=[30, 120])
    ap.add_argument("--points", type=int, nargs="+", default=[3000, 8000])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_and_fuse_leg.json"))
    a = ap.parse_args()
    lines = []
    for T in a.targets:
        for n in a.points:
            lines.append(json.dumps(measure(T, n, a.repeats, a.warmup)))
            print(lines[-1], flush=True)
    lines.append(json.dumps(measure_robomaster(a.repeats, a.warmup)))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
