"""Timing of Tracking::CreateNewKeyFrame's way into a dvm_keyframe_store for 1, 8 and 32 frames of a tick promoted at once
(tools/track_refkf_tick_leg.py's world: 640 x 480 frames of 1 000 features), tools/keyframe_store_leg.py's protocol: in one process,
after warm-up, the forms alternating per repeat, host -> host, p5 / median / p95 in ms of 200 calls after 20.  Every timed call follows a
batched first half of its own, which is not timed.
  host    the frames downloaded (dvm_orb_download), dvmh_vocab_transform per frame, dvm_keyframe_store_put of all
  device  dvm_keyframe_store_put_tracked of all
`same_as_put`: every field dvm_keyframe_store_debug_read returns is equal between the two forms' slots; `upload_bytes`:
dvm_keyframe_store_last_put_bytes of both; `kernels_ms`: HIP-event medians of check / transform / bow / put from a separate pass
(dvm_keyframe_store_profile).
--host-only measures the host form alone and touches no new entry point, so it also runs on a library built from the parent commit
(DVM_HIP_LIB=<that library>, its libdvmslam_host.so beside it): that run is the baseline.  --baseline <its json> adds the baseline's rows
and, per shape, `host_within_baseline_band` (this build's host median inside the baseline's p5 .. p95).
Usage: python tools/keyframe_put_leg.py [--frames 1 8 32] [--repeats 200] [--warmup 20] [--host-only] [--baseline FILE]
                                        [--out profiles/keyframe_put_leg.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dvm_slam_amd import capi  # noqa: E402
import pixel_scene as ps  # noqa: E402
import track_refkf_tick_leg as leg  # noqa: E402
from bow_store_leg import alternate  # noqa: E402

LEVELSUP = 4


def put_leg(Kf, W, repeats, warmup, host_only):
    vocd = capi.Vocabulary(W["voc"])
    ext = capi.OrbExtractor(nfeatures=1000, max_batch=Kf)
    tb = capi.TrackerBatch(ext, Kf)
    k0 = W["kf"]["kps"]
    ts = [1 + b % 4 for b in range(Kf)]
    imgs = np.stack([W["frames"][t] for t in ts])
    ins = tb.prepare([leg.tcw7f(ps.pose7(*W["poses"][t - 1])) for t in ts], [(k0[:0], np.zeros(0, np.int32), None, W["mps"])] * Kf)
    tab = dict(K=np.asarray(ps.K, np.float32), bounds=leg.BOUNDS, scale_factors=W["scale"], level_sigma2=(W["scale"] ** 2).astype(np.float32),
               inv_level_sigma2=W["inv_s2"], log_scale_factor=float(np.log(W["scale"][1])))
    store = capi.KeyframeStore(2 * Kf, ext.cap)
    frames = np.arange(Kf, dtype=np.int32)
    slots_h, slots_d = np.arange(Kf, dtype=np.int32), np.arange(Kf, 2 * Kf, dtype=np.int32)

    def first_half():
        tb.track(imgs, ins, ps.K, leg.BOUNDS, W["scale"], W["inv_s2"], th=15.0)

    def host():
        kfs = []
        for b in range(Kf):
            n, kps, desc, _ = ext.download(b)
            kfs.append(dict(tab, kps=kps, desc=desc, fv=capi.vocab_transform_host(W["voc"], desc, LEVELSUP)))
        store.put(slots_h, kfs)
        return kfs

    def device():
        return store.put_tracked(tb, ext, vocd, frames, slots_d, [tab] * Kf, levelsup=LEVELSUP)

    calls = dict(host=host)
    first_half()
    kfs = host()
    up_host = None if not hasattr(store.L, "dvm_keyframe_store_last_put_bytes") else store.last_put_bytes()
    out = dict(leg="keyframe_put", frames=Kf, keypoints_mean=float(np.mean([len(k["kps"]) for k in kfs])))
    if not host_only:
        calls["device"] = device
        device()
        same = True
        for a, b in zip(slots_h, slots_d):
            ra, rb = store.read(int(a)), store.read(int(b))
            same = same and set(ra) == set(rb) and all(np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])) for k in ra if k != "generation")
        out["same_as_put"] = bool(same)
        out["upload_bytes"] = dict(host=up_host, device=store.last_put_bytes())
    out.update(alternate(calls, repeats, warmup, before={k: first_half for k in calls}))
    if not host_only:
        store.profile(True)
        km = []
        for _ in range(30):
            first_half(); device()
            km.append(store.last_put_ms())
        store.profile(False)
        out["kernels_ms"] = dict(zip(("check", "transform", "bow", "put"), (round(float(x), 4) for x in np.median(np.array(km), axis=0))))
        out["device_faster"] = bool(out["device"]["median_ms"] < out["host"]["median_ms"])
    ext.sync()
    store.close(); tb.close(); ext.close(); vocd.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_put_leg.json"))
    a = ap.parse_args()
    base = {}
    if a.baseline:
        with open(a.baseline) as f:
            base = {r["frames"]: r for r in map(json.loads, filter(None, (ln.strip() for ln in f)))}
    W = leg.world()
    lines = []
    for Kf in a.frames:
        row = put_leg(Kf, W, a.repeats, a.warmup, a.host_only)
        b = base.get(Kf)
        if b and "device" in row:
            row["baseline"] = b["host"]
            row["host_within_baseline_band"] = bool(b["host"]["p5_ms"] <= row["host"]["median_ms"] <= b["host"]["p95_ms"])
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
