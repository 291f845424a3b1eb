"""The unchanged tracked-frame calls on the resident stores (TrackerBatch.track_resident, .track_local_map_resident) on this build and on
the parent commit's build: p5 / median / p95 of --repeats after --warmup per call, host to host, for 1 and 8 frames of a tick on the
scene of tests/test_gpu_track_resident.py (a local map of about 3 000 points).
libdvmslam_host.so names libdvmslam_hip.so by its soname, so two builds of the pair cannot be loaded beside each other in one process:
each measurement is a process of its own with DVM_HIP_LIB naming the build, and the driver alternates them -- parent, this, parent,
this.  A row per (frames, call) carries every run, and within_parent_band: this build's medians lie inside the span of the parent runs'
p5 .. p95.  Nothing is asserted.
Usage: python tools/track_resident_band.py --parent-lib PATH/libdvmslam_hip.so [--repeats 200] [--warmup 20] [--out FILE (appended)]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def child(repeats, warmup):
    import numpy as np
    from dvm_slam_amd import capi
    import pixel_scene as ps
    from test_gpu_track_frame import BOUNDS, _tcw7f
    from test_gpu_track_local_map import _scene_table
    from test_gpu_track_resident import Slots, _ids, _r64

    def stats(v):
        a = np.asarray(v) * 1e3
        return dict(p5_ms=round(float(np.percentile(a, 5)), 4), median_ms=round(float(np.median(a)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))
    frames, poses = ps.render(12)
    ext1 = capi.OrbExtractor(max_batch=1)
    tab = ext1.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    rng = np.random.default_rng(17)
    pts, (k0, n0) = _scene_table(capi, ext1, frames, poses, scale, rng)
    S = Slots(capi, pts, rng)
    K = ps.K.astype(np.float32)
    mp_l = np.arange(n0, dtype=np.int32)
    out = {}
    for B in (1, 8):
        ext = capi.OrbExtractor(max_batch=B)
        trk = capi.TrackerBatch(ext, B)
        trk.reserve_local_map(B * _r64(len(pts)))
        Ts = [_tcw7f(ps.pose7(*poses[0]))] * B
        imgs = np.stack([frames[1]] * B)
        ins, keep = trk.prepare_resident(Ts, [(k0, S.to_slots(mp_l), None, S.store)] * B)
        r = trk.track_resident(imgs, ins, K, BOUNDS, scale, inv_s2, th=15.0)
        fms = [_ids(S, x["mp"]) for x in r]
        t1, t2 = [], []
        for it in range(warmup + repeats):
            a = time.perf_counter()
            trk.track_resident(imgs, ins, K, BOUNDS, scale, inv_s2, th=15.0)
            b = time.perf_counter()
            trk.track_local_map_resident([S.store] * B, [S.slot_of] * B, fms, th=1.0)
            c = time.perf_counter()
            if it >= warmup:
                t1.append(b - a); t2.append(c - b)
        out[str(B)] = dict(track_resident=stats(t1), track_local_map_resident=stats(t2), local_points=len(pts))
        trk.close(); ext.close()
    print("BAND " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_local_map_leg.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.repeats, a.warmup)
    runs = []
    for which in ("parent", "this", "parent", "this"):
        env = dict(os.environ)
        if which == "parent":
            env["DVM_HIP_LIB"] = os.path.abspath(a.parent_lib)
        else:
            env.pop("DVM_HIP_LIB", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(a.repeats), "--warmup", str(a.warmup)], env=env,
                           capture_output=True, text=True, timeout=600)
        line = [l for l in r.stdout.splitlines() if l.startswith("BAND ")]
        if r.returncode != 0 or not line:
            sys.exit(f"the {which} run failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        runs.append((which, json.loads(line[0][5:])))
    rows = []
    for B in ("1", "8"):
        for call in ("track_resident", "track_local_map_resident"):
            par = [r[B][call] for w, r in runs if w == "parent"]
            own = [r[B][call] for w, r in runs if w == "this"]
            lo, hi = min(x["p5_ms"] for x in par), max(x["p95_ms"] for x in par)
            rows.append(dict(leg="track_resident_band", frames=int(B), call=call, local_points=runs[0][1][B]["local_points"], parent=par, this_build=own,
                             order="parent, this, parent, this: one process each", within_parent_band=bool(all(lo <= x["median_ms"] <= hi for x in own))))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for row in rows:
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
