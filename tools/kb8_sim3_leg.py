"""Timing of the two Sim3 steps of a merge attempt -- Sim3Solver's hypotheses and OptimizeSim3 -- on pinhole and on fisheye cameras: what
the KannalaBrandt8 projections (a float atan2f and a square root in each of the four projections of CheckInliers; a float atan2f in each
residual and a double atan2 in each of the 28 central-difference projections per pair of OptimizeSim3) cost the one-wave-per-hypothesis
kernel and the one-workgroup kernel.

Shapes of a merge attempt: the correspondences merge.solve_against_candidate gathers on tests/merge_scene.py (seed 0), 300 hypotheses.
The fisheye run takes the same two agents through the robot's camera (tests/sim3_cam_scene.two_agent_scene_kb8): SearchByBoW reads no
camera, so both runs have the same pairs.  Host to host through the binding, in one process, alternating per repeat
  pinhole      dvm_sim3_hypotheses / dvm_optimize_sim3 (the yardstick: the code of before the camera models)
  cam_pinhole  the _cam entry with model 0 on both sides
  cam_fisheye  the _cam entry with two robomaster models
  pinhole_b    the pinhole entry again: its spread against its own first copy is the noise floor
median and p5 - p95 of `repeats` after `warmup`.  One JSON line, written to profiles/kb8_sim3_leg.json.
Usage: python tools/kb8_sim3_leg.py [--repeats 30] [--warmup 5] [--out profiles/kb8_sim3_leg.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_HYPOTHESES = 300


def gather(capi, fisheye):
    """(hypothesis arguments, OptimizeSim3 arguments) of the merge flow on the two-agent scene, as merge.GpuOps receives them."""
    from dvm_slam_amd import merge, synth
    from oracle import pyoracle as po
    import sim3_cam_scene as cs
    from merge_scene import make_two_agent_scene

    class Ops(merge.GpuOps):
        def sim3_hypotheses(self, *a):
            self.hyp = a
            return super().sim3_hypotheses(*a)

        def optimize_sim3(self, *a):
            self.opt = a
            return super().optimize_sim3(*a)

        def sim3_hypotheses_cam(self, *a):
            self.hyp = a
            return super().sim3_hypotheses_cam(*a)

        def optimize_sim3_cam(self, *a):
            self.opt = a
            return super().optimize_sim3_cam(*a)
    sc = cs.two_agent_scene_kb8(po, 0, n_distract=12) if fisheye else make_two_agent_scene(po, 0)
    models = (capi.CameraModel.robomaster(), capi.CameraModel.robomaster()) if fisheye else None
    tr = np.random.default_rng(0).integers(0, 1 << 30, (N_HYPOTHESES, 3)).astype(np.int64)
    tr[:, 1] += (tr[:, 1] == tr[:, 0]); tr[:, 2] += 2 * ((tr[:, 2] == tr[:, 0]) | (tr[:, 2] == tr[:, 1]))
    ops = Ops(synth.vocabulary(k=10, L=4, seed=5))
    peers = [dict(p) for p in sc["peers"]]
    db = merge.fill_database(ops, peers, levelsup=2)
    r = merge.merge_with_peer(ops, sc["a"], sc["pa"], peers, sc["peer_pts"], db, 2, tr, models=models)
    assert r["candidate"] == sc["true_idx"] and r["n_sim3_inliers"] >= 20
    return ops.hyp, ops.opt, r


def stats(v):
    a = np.asarray(v) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p5_ms=round(float(np.percentile(a, 5)), 4), p95_ms=round(float(np.percentile(a, 95)), 4), n=len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kb8_sim3_leg.json"))
    a = ap.parse_args()
    from dvm_slam_amd import capi
    if capi.device_count() < 1:
        raise RuntimeError("kb8_sim3_leg needs an MI355X: no HIP device visible")
    hyp_p, opt_p, res_p = gather(capi, False)
    hyp_f, opt_f, res_f = gather(capi, True)
    K1, K2 = hyp_p[4], hyp_p[5]
    pin = (capi.CameraModel.pinhole(*K1), capi.CameraModel.pinhole(*K2))
    legs = {
        "hypotheses": dict(
            pinhole=lambda: capi.sim3_hypotheses(*hyp_p, False),
            cam_pinhole=lambda: capi.sim3_hypotheses_cam(*hyp_p[:4], pin[0], pin[1], hyp_p[6], False),
            cam_fisheye=lambda: capi.sim3_hypotheses_cam(*hyp_f, False),
            pinhole_b=lambda: capi.sim3_hypotheses(*hyp_p, False)),
        "optimize_sim3": dict(
            pinhole=lambda: capi.optimize_sim3(opt_p[0], False, *opt_p[1:]),
            cam_pinhole=lambda: capi.optimize_sim3_cam(opt_p[0], False, *opt_p[1:7], pin[0], pin[1], opt_p[9]),
            cam_fisheye=lambda: capi.optimize_sim3_cam(opt_f[0], False, *opt_f[1:]),
            pinhole_b=lambda: capi.optimize_sim3(opt_p[0], False, *opt_p[1:])),
    }
    out = dict(leg="kb8_sim3", pairs=dict(pinhole=len(hyp_p[0]), fisheye=len(hyp_f[0])), hypotheses=N_HYPOTHESES,
               sim3_inliers=dict(pinhole=int(res_p["n_sim3_inliers"]), fisheye=int(res_f["n_sim3_inliers"])), repeats=a.repeats, warmup=a.warmup)
    for leg, calls in legs.items():
        times = {k: [] for k in calls}
        for it in range(a.warmup + a.repeats):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                if it >= a.warmup:
                    times[k].append(t1 - t0)
        med = {k: float(np.median(v)) for k, v in times.items()}
        out[leg] = dict(host_to_host={k: stats(v) for k, v in times.items()},
                        cam_pinhole_over_pinhole=round(med["cam_pinhole"] / med["pinhole"], 3),
                        cam_fisheye_over_pinhole=round(med["cam_fisheye"] / med["pinhole"], 3),
                        noise_floor=round(abs(med["pinhole_b"] / med["pinhole"] - 1.0), 3))
    s = json.dumps(out)
    print(s, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
