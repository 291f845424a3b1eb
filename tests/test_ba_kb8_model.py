"""CPU tests behind dvm_ba_set_problem_cam (bundle adjustment on a KannalaBrandt8 camera):

  1. the restatement: ba_f64 (tests/ba_kb8_scene.py) on a PINHOLE camera against the oracle (oracle/ba_oracle.cpp) on cases a-e rebuilt with
     a pinhole projection -- identical trial counts and stop reason, poses and landmarks within the project's 1e-6 contract for differing
     summation orders.  This pins the Levenberg control of the restatement, which the GPU test then runs under the fisheye camera;
  2. the scenes hold what they are described to hold, every KannalaBrandt8 case has an admissible seed, and the measured tolerance lies
     between half the recorded constants and the constants;
  3. the library exports dvm_ba_set_problem_cam and capi.BundleAdjuster has set_problem_cam.
tests/test_gpu_ba_kb8.py runs the device on the same scenes."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import ba_kb8_scene as bs  # noqa: E402
import kb8_scene as ks  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement against the oracle, pinhole
@pytest.mark.parametrize("case", list(bs.CASES))
def test_ba_f64_pinhole_is_the_oracle(oracle, case):
    sc = bs.ba_scene("pinhole", case, 0)
    pj, jac = bs.pinhole_camera(bs.PINHOLE_K)
    T, X, trials, stop, chi = bs.ba_f64(sc["poses0"], sc["fixed"], sc["points0"], sc["edges"], pj, jac, bs.HUBER, bs.ITERATIONS)
    To, Xo, st, chio = oracle.ba_optimize(sc["poses0"], sc["fixed"], sc["points0"], sc["edges"], bs.PINHOLE_K, bs.HUBER, bs.ITERATIONS)
    dT, dX = float(np.abs(T - To).max()), float(np.abs(X - Xo).max())
    print(f"case {case}: trials {trials} / {st['trials']}, stop {stop} / {st['stop_reason']}, |dpose| {dT:.2e}, |dpoint| {dX:.2e}")
    assert trials == list(st["trials"]) and stop == st["stop_reason"] and len(trials) == st["iterations"]
    assert dT < bs.PINHOLE_TOL and dX < bs.PINHOLE_TOL
    assert np.allclose(chi, chio, rtol=1e-6, atol=1e-6)


# ---- 2. scenes, admission, tolerance
@pytest.mark.parametrize("model,case", bs.all_cases())
def test_scene_holds_what_it_says(model, case):
    sc, ref, seed = bs.ba_case(model, case)
    P, n_fixed, L, E = bs.CASES[case]
    e = sc["edges"]
    assert (len(sc["poses0"]), int(sc["fixed"].sum()), len(sc["points0"]), len(e)) == (P, n_fixed, L, E)
    assert np.array_equal(sc["fixed"][:n_fixed], np.ones(n_fixed, np.uint8)) and np.array_equal(sc["poses0"][:n_fixed], sc["poses_gt"][:n_fixed])
    assert len(set(zip(e["pose"].tolist(), e["point"].tolist()))) == E                 # one edge per (camera, landmark)
    n_obs = np.bincount(e["point"], minlength=L)
    assert n_obs.min() >= 3
    Xc = bs._camera_frame_points(sc["poses_gt"], sc["points_gt"], e)
    theta = np.arctan2(np.hypot(Xc[:, 0], Xc[:, 1]), Xc[:, 2])
    assert theta.min() >= bs.THETA_MIN and theta.max() <= bs.THETA_MAX
    d = np.linalg.norm(sc["points_gt"], axis=1)
    assert d.min() >= 5.0 and d.max() <= 14.0
    # outliers: at most one per landmark, only on landmarks with at least six observations
    bad_l = e["point"][sc["bad"]]
    assert len(set(bad_l.tolist())) == len(bad_l) and np.all(n_obs[bad_l] >= 6)
    if P >= 6:
        assert sc["bad"].any()
    # the admitted draw: same trials under the ulp, chi2 far from the threshold, nothing near the axis
    assert ref["trials"] == ref["trials_n"] and ref["stop"] == ref["stop_n"]
    assert float(np.min(np.abs(ref["chi2"] - bs.CHI2_MONO))) >= bs.BAND_FACTOR * ref["dchi2"]
    assert ref["dchi2"] > 0.0                                                        # the ulp did reach the residuals
    print(f"{model} {case}: seed {seed}, trials {ref['trials']}, stop {ref['stop']}, ulp moves poses {ref['dpose']:.2e} points {ref['dpoint']:.2e} chi2 {ref['dchi2']:.2e}")


def test_theta_ulp_tolerance_matches_the_record():
    dp, dx = bs.theta_ulp_ba_diff()
    print(f"theta ulp: poses {dp:.3e} (recorded {bs.THETA_ULP_BA_POSE_DIFF:.3e}), points {dx:.3e} (recorded {bs.THETA_ULP_BA_POINT_DIFF:.3e})")
    assert 0.5 * bs.THETA_ULP_BA_POSE_DIFF <= dp <= bs.THETA_ULP_BA_POSE_DIFF
    assert 0.5 * bs.THETA_ULP_BA_POINT_DIFF <= dx <= bs.THETA_ULP_BA_POINT_DIFF


def test_two_round_draw_is_admissible():
    for model in bs.MODELS:
        sc, tr, seed = bs.two_round_case(model, "d")
        assert tr["round1"][2] == tr["round1_n"][2] and tr["round2"][2] == tr["round2_n"][2] and tr["round2"][3] == tr["round2_n"][3]
        assert 0 < int((tr["flags"] == 0).sum()) < len(tr["flags"])                 # the second round does drop edges
        assert len(tr["round1"][2]) == 5


def test_kb8_residual_differs_from_pinhole():
    """The two cameras are different problems: the pinhole reading of a fisheye scene's observations is off by many pixels."""
    sc = bs.ba_case("robomaster", "b")[0]
    Xc = bs._camera_frame_points(sc["poses_gt"], sc["points_gt"], sc["edges"])
    uv_pin = bs.pinhole_camera(ks.MODELS["robomaster"][:4])[0](Xc)
    uv_kb8 = bs.kb8_camera(ks.MODELS["robomaster"])[0](Xc)
    assert float(np.abs(uv_pin - uv_kb8).max()) > 10.0


# ---- 3. the entry exists
def test_library_exports_set_problem_cam(capi):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dvm_slam_amd", "lib", "libdvmslam_hip.so")], capture_output=True, text=True).stdout
    assert " T dvm_ba_set_problem_cam\n" in out
    assert hasattr(capi.lib(), "dvm_ba_set_problem_cam")
    assert callable(getattr(capi.BundleAdjuster, "set_problem_cam", None))
    hdr = open(os.path.join(ROOT, "include", "dvmslam_hip.h")).read()
    assert "int dvm_ba_set_problem_cam(dvm_ba* h" in hdr
